#!/opt/conda/bin/python3.9
"""Reference answers for whole-buffer frame searches on small seeded buffers:
what `locate_frames(..., forward=True, maximum=len(buffer))` of the reference
returns from position 0 (base/base.py:181-335; Mark 4: mark4/base.py:110-166;
Mark 5B additionally gated by the time-code CRC as `find_header` does,
mark5b/base.py:136-155).

The buffers come from oracle/bb_index_np.build_whole_case (seeded; two to five
frames, frame starts at every residue mod 4, byte slips between frames, headers
damaged in place, the end cut inside a following header).  Per case the file
records the builder's parameters, the buffer's SHA-256 and the sorted answers:

* VDIF: `check=(1,)`, `check=(2,)` and `check=(-1,)` separately -- bb_vdif_locate's
  contract (include/bbdecode.h) is a stated combination of the three
  (bb_index_np.vdif_combine);
* Mark 5B, Mark 4: `check=1`, which the contracts follow as it stands.

The end is cut at EVERY length from 0 to header_nbytes + 4 bytes into the
following header for VDIF and Mark 5B.  A Mark 4 header is 320-1280 bytes: there
the cuts are 0-5 and everything within two bytes of each place where the
answer can change (stream words 63, 64 and 96, the header's end), which keeps
the file at a few hundred cases.

Run in the development container, next to the reference:

    /opt/conda/bin/python3.9 oracle/gen_golden_locate_whole.py

writes tests/golden/locate_whole_cases.json (data only)."""
import io
import json
import os
import sys

import numpy as np
np.asscalar = getattr(np, 'asscalar', lambda a: a.item())
np.alen = getattr(np, 'alen', len)
sys.path.insert(0, '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(os.path.dirname(HERE), 'tests', 'golden')

from baseband import vdif, mark5b, mark4                    # noqa: E402
from baseband.mark5b.header import crc16                    # noqa: E402
import bb_index_np as ix                                    # noqa: E402


def vdif_pattern(spec):
    H = spec['header_nbytes']
    pat = ix.vdif_header_words(spec['frame_nbytes'], H, seconds=100, edv=spec.get('edv', 0),
                               station=spec.get('station', 0x4142))
    pat += [0] * (8 - len(pat))
    msk = list(ix.VDIF_MASKS[spec['mask']])
    return pat, msk


def answers(spec, blob):
    n = len(blob)
    if spec['fmt'] == 'vdif':
        pat, msk = vdif_pattern(spec)
        nw = spec['header_nbytes'] // 4
        out = {}
        with vdif.open(io.BytesIO(blob), 'rb') as fh:
            for name, check in (('check_1', (1,)), ('check_2', (2,)), ('check_m1', (-1,))):
                out[name] = sorted(fh.locate_frames(pat[:nw], mask=msk[:nw], frame_nbytes=spec['frame_nbytes'],
                                                    maximum=n, check=check))
        return out
    if spec['fmt'] == 'mark5b':
        with mark5b.open(io.BytesIO(blob), 'rb', kday=56000) as fh:
            if spec.get('w1_mask'):
                locs = fh.locate_frames([ix.M5B_SYNC, spec['w1_pattern'], 0, 0],
                                        mask=[0xffffffff, spec['w1_mask'], 0, 0],
                                        frame_nbytes=ix.M5B_FRAME, maximum=n)
            else:
                locs = fh.locate_frames(maximum=n)
            good = []
            for loc in locs:
                fh.seek(loc)
                try:
                    header = fh.read_header()
                except Exception:
                    continue
                if crc16.check((int(header.words[2]) << 32) | int(header.words[3])):
                    good.append(loc)
        return {'ref': sorted(good)}
    with mark4.open(io.BytesIO(blob), 'rb', ntrack=spec['ntrack']) as fh:
        return {'ref': sorted(fh.locate_frames(maximum=n))}


def specs():
    seed = [20261016]

    def add(lst, **kw):
        seed[0] += 1
        kw.setdefault('slips', [0] * (kw['nframes'] - 1))
        kw.setdefault('damaged', [])
        kw.setdefault('cut', None)
        kw['seed'] = seed[0]
        lst.append(kw)

    out = []
    vd = [dict(fmt='vdif', frame_nbytes=5032, header_nbytes=32, mask='edv0'),
          dict(fmt='vdif', frame_nbytes=1032, header_nbytes=16, mask='legacy'),
          dict(fmt='vdif', frame_nbytes=40, header_nbytes=32, mask='edv3', edv=3)]
    m5 = [dict(fmt='mark5b'), dict(fmt='mark5b', w1_pattern=0xf00f0000, w1_mask=0xffff0000)]
    m4 = [dict(fmt='mark4', ntrack=nt) for nt in (16, 32, 64)]

    def m4_cuts(nt):
        isz = nt // 8
        s = set(range(6))
        for c in (63 * isz, 64 * isz, 96 * isz, 160 * isz, 160 * isz + 4):
            s.update(range(c - 2, c + 3))
        return sorted(s)

    # the end cut inside the following header, frame starts at every residue mod 4
    for base in vd[:2] + m5[:1]:
        H = base.get('header_nbytes', 16)
        for start in range(4):
            for cut in range(H + 5):
                add(out, nframes=2, start=start, cut=cut, **base)
    for cut in range(37):
        add(out, nframes=3, start=1, cut=cut, **vd[2])
    for cut in range(21):
        add(out, nframes=2, start=3, cut=cut, **m5[1])
    for base in m4:
        for start in (range(4) if base['ntrack'] == 16 else (1,)):
            for cut in m4_cuts(base['ntrack']):
                add(out, nframes=2, start=start, cut=cut, **base)
    # ... and with that following header damaged in place
    for base in vd[:1] + m5:
        H = base.get('header_nbytes', 16)
        for start in (0, 1):
            for cut in range(H + 5):
                add(out, nframes=2, start=start, cut=cut, damaged=[2], **base)
    for cut in m4_cuts(16):
        add(out, nframes=2, start=2, cut=cut, damaged=[2], **m4[0])
    # the last frame ending exactly at the end, and 1-3 bytes short of it; a lone frame
    for base in vd + m5 + m4:
        for short in range(4):
            add(out, nframes=3, start=short, cut_short=short, **base)
        add(out, nframes=1, start=5, **base)
        add(out, nframes=1, start=0, cut=3, **base)
    # slips between frames walk the residues; headers damaged in place
    for base in vd + m5 + m4:
        add(out, nframes=5, start=0, slips=[1, 1, 1, 1], **base)
        add(out, nframes=5, start=2, slips=[-1, 2, -3, 5], cut=2, **base)
        add(out, nframes=4, start=1, slips=[0, -2, 0], cut=base.get('header_nbytes', 16) + 1, **base)
        add(out, nframes=5, start=0, damaged=[2], **base)
        add(out, nframes=5, start=3, damaged=[2, 3], cut=1, **base)
        add(out, nframes=5, start=1, damaged=[1], slips=[0, 0, 3, 0], **base)
        add(out, nframes=4, start=0, damaged=[3], cut=0, **base)
        add(out, nframes=4, start=2, damaged=[2], cut=9, **base)
        add(out, nframes=3, start=0, damaged=[0], slips=[0, -1], **base)
    return out


def main():
    cases = []
    for spec in specs():
        full, nbytes = ix.build_whole_case(spec)
        blob = full[:nbytes].tobytes()
        case = dict(spec)
        case['nbytes'] = nbytes
        case['sha256'] = ix.sha256(full[:nbytes])
        case['sha256_full'] = ix.sha256(full)
        case['answers'] = answers(spec, blob)
        cases.append(case)
    with open(os.path.join(GOLD, 'locate_whole_cases.json'), 'w') as f:
        json.dump({"made_by": "oracle/gen_golden_locate_whole.py", "cases": cases}, f, separators=(',', ':'))
    print(len(cases), 'cases')


if __name__ == '__main__':
    main()
