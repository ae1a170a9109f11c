"""Brute-force CPU restatements of the frame-search, header-scan and index
entry points of include/bbdecode.h (bb_*_locate, bb_*_scan, bb_*_scan_at,
bb_build_index, bb_verify_records), NumPy only.

Written from the contracts in the header and on BYTES: every byte position of a
buffer is a candidate, a masked pattern either stands at a position or it does
not, and a position is reported exactly when the contract's conditions hold for
the bytes inside ``buf`` (nothing behind ``len(buf)`` exists).  No sweep, probe,
confirm, lanes or aligned dwords: none of the kernels' structure is restated.
Header fields come from bb_oracle_np.{vdif,mark5b,mark4}_header_fields, which
are pinned to the reference.

Also here, because the generator of tests/golden/locate_whole_cases.json and the
tests have to build the SAME bytes: makers of valid headers and
``build_whole_case`` (seeded; the tests check the recorded SHA-256 first).

Pinned by tests/test_index_oracle.py; used by tests/test_index_kernels_gpu.py.
"""
import hashlib

import numpy as np

import bb_oracle_np as orc

FRAME_OK, FRAME_INVALID = 1, 2
M5B_FRAME = 10016
M5B_SYNC = 0xABADDEED
M5B_FILL = 0x11223344
TIDX_MAX = 0x7fffffff


# --------------------------------------------------------------------------
# bytes
# --------------------------------------------------------------------------
def _bytes(buf):
    return np.ascontiguousarray(np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf,
                                dtype=np.uint8)


def words_to_bytes(words):
    return np.asarray([int(w) & 0xffffffff for w in words], dtype='<u4').view(np.uint8)


def match_positions(buf, pattern, mask):
    """All positions p (sorted int64) with ``(buf[p + k] ^ pattern[k]) & mask[k] == 0``
    for every k, the whole pattern inside the buffer."""
    buf = _bytes(buf)
    pattern, mask = np.asarray(pattern, np.uint8), np.asarray(mask, np.uint8)
    npos = len(buf) - len(pattern) + 1
    if npos <= 0:
        return np.zeros(0, np.int64)
    pos = None
    # (the bytes with the most mask bits first: the fewest survivors to carry on)
    order = sorted(np.nonzero(mask)[0].tolist(), key=lambda k: -bin(int(mask[k])).count('1'))
    for k in order:
        if pos is None:
            pos = np.nonzero(((buf[k:k + npos] ^ pattern[k]) & mask[k]) == 0)[0].astype(np.int64)
        else:
            pos = pos[((buf[pos + k] ^ pattern[k]) & mask[k]) == 0]
    return np.arange(npos, dtype=np.int64) if pos is None else pos


def u32_at(buf, pos):
    """Little-endian dword at any byte position; zero unless its four bytes lie inside the buffer."""
    if pos < 0 or pos + 4 > len(buf):
        return 0
    return int(buf[pos]) | int(buf[pos + 1]) << 8 | int(buf[pos + 2]) << 16 | int(buf[pos + 3]) << 24


# --------------------------------------------------------------------------
# searches
# --------------------------------------------------------------------------
def vdif_locate(buf, frame_nbytes, header_nbytes, pattern, mask):
    """bb_vdif_locate.  With M the positions where a whole header lies inside the
    buffer and agrees with `pattern` under `mask`: p is reported when p is in M,
    p + frame_nbytes <= nbytes, and
      * if the header one frame later lies wholly inside the buffer: it is in M, or
        the one two frames later lies wholly inside the buffer and is in M;
      * else (last frame): p < frame_nbytes, or p - frame_nbytes is in M."""
    buf = _bytes(buf)
    n, F, H = len(buf), int(frame_nbytes), int(header_nbytes)
    if F < 32 or n < F:
        return np.zeros(0, np.int64)
    nw = H // 4
    M = match_positions(buf, words_to_bytes(pattern[:nw]), words_to_bytes(mask[:nw]))
    inM = set(M.tolist())
    out = []
    for p in M.tolist():
        if p + F > n:
            continue
        nxt = p + F
        if nxt + H <= n:
            ok = nxt in inM or (nxt + F + H <= n and nxt + F in inM)
        else:
            ok = p < F or (p - F) in inM
        if ok:
            out.append(p)
    return np.asarray(out, np.int64)


def vdif_combine(answers, nbytes, frame_nbytes, header_nbytes):
    """bb_vdif_locate's contract as a combination of the reference's locate_frames answers
    for check=(1,), (2,) and (-1,) (tests/golden/locate_whole_cases.json).  Each of the three
    holds the positions where the pattern matches and the frame fits, less those where the
    header at its check point could be looked at and did not match.  p is reported when
      * the header one frame later lies wholly inside the buffer and p is in check_1, or
        the header two frames later does so too and p is in check_2;
      * the header one frame later does not lie wholly inside the buffer and p is in check_m1.
    (The reference looks at a check point when the masked part of the pattern lies inside the
    buffer with at least one byte to spare: whenever the whole header does, unless the mask
    reaches the header's last byte and the buffer ends exactly there.  The recorded cases with
    such a mask -- 'edv3' -- have an intact header at that place, so either reading agrees.)"""
    a1, a2, am = (set(answers[k]) for k in ('check_1', 'check_2', 'check_m1'))
    F, H = frame_nbytes, header_nbytes
    out = []
    for p in sorted(a1 | a2 | am):
        if p + F + H <= nbytes:
            ok = p in a1 or (p + 2 * F + H <= nbytes and p in a2)
        else:
            ok = p in am
        if ok:
            out.append(p)
    return out


def crc16_mark5b_ok(w2, w3):
    """CRC-16 (x^16 + x^15 + x^2 + 1) of the 48 time-code bits -- word 2 and the upper half
    of word 3, most significant bit first -- equals the lower half of word 3: long division."""
    bits = [(w2 >> (31 - i)) & 1 for i in range(32)] + [(w3 >> (31 - i)) & 1 for i in range(16)]
    bits += [0] * 16
    poly = [1, 1] + [0] * 12 + [1, 0, 1]          # x^16 x^15 ... x^2 . 1
    for i in range(48):
        if bits[i]:
            for k in range(17):
                bits[i + k] ^= poly[k]
    rem = 0
    for b in bits[48:]:
        rem = rem << 1 | b
    return rem == (w3 & 0xffff)


def crc16_mark5b(w2, frac16):
    """The 16 CRC bits that make (w2, frac16 << 16 | crc) pass crc16_mark5b_ok."""
    bits = [(w2 >> (31 - i)) & 1 for i in range(32)] + [(frac16 >> (15 - i)) & 1 for i in range(16)]
    bits += [0] * 16
    poly = [1, 1] + [0] * 12 + [1, 0, 1]
    for i in range(48):
        if bits[i]:
            for k in range(17):
                bits[i + k] ^= poly[k]
    rem = 0
    for b in bits[48:]:
        rem = rem << 1 | b
    return rem


def mark5b_locate(buf, w1_pattern=0, w1_mask=0):
    """bb_mark5b_locate / bb_mark5b_locate_stream.  p is reported when the sync word stands
    at p, p + 10016 <= nbytes, word 1 agrees with w1_pattern under w1_mask, the time code
    passes its CRC, and -- when MORE than plen bytes lie behind the frame, plen = 4 without
    and 8 with a word-1 mask -- the sync word (and word 1 under the mask) stands one frame
    later as well."""
    buf = _bytes(buf)
    n = len(buf)
    w1_pattern, w1_mask = int(w1_pattern) & 0xffffffff, int(w1_mask) & 0xffffffff
    plen = 8 if w1_mask else 4
    S = match_positions(buf, words_to_bytes([M5B_SYNC]), words_to_bytes([0xffffffff]))
    inS = set(S.tolist())
    out = []
    for p in S.tolist():
        if p + M5B_FRAME > n:
            continue
        if (u32_at(buf, p + 4) ^ w1_pattern) & w1_mask:
            continue
        if not crc16_mark5b_ok(u32_at(buf, p + 8), u32_at(buf, p + 12)):
            continue
        nxt = p + M5B_FRAME
        if nxt + plen < n:
            if nxt not in inS or (u32_at(buf, nxt + 4) ^ w1_pattern) & w1_mask:
                continue
        out.append(p)
    return np.asarray(out, np.int64)


def mark4_sync_pattern(ntrack):
    """Bytes of stream words 63 .. 95 of a frame: word 63 all zero, words 64-95 all ones."""
    isz = ntrack // 8
    return np.concatenate([np.zeros(isz, np.uint8), np.full(32 * isz, 0xff, np.uint8)])


def mark4_locate(buf, ntrack):
    """bb_mark4_locate.  p is reported when stream word 63 of the frame at p is zero and words
    64..95 are all ones, p + ntrack*2500 <= nbytes, and -- when more than the first 96 stream
    words of the following frame lie inside the buffer -- that frame shows the same."""
    buf = _bytes(buf)
    n, isz, F = len(buf), ntrack // 8, ntrack * 2500
    pat = mark4_sync_pattern(ntrack)
    M = match_positions(buf, pat, np.full(len(pat), 0xff, np.uint8)) - 63 * isz
    M = M[M >= 0]
    inM = set(M.tolist())
    out = [p for p in M.tolist()
           if p + F <= n and (not (p + F + 96 * isz < n) or (p + F) in inM)]
    return np.asarray(out, np.int64)


# --------------------------------------------------------------------------
# records
# --------------------------------------------------------------------------
def _clamp(t):
    return max(-TIDX_MAX, min(TIDX_MAX, int(t)))


def _recs(rows):
    r = np.asarray(rows, np.int64).reshape(-1, 4)
    return dict(payload_offset=r[:, 0].copy(), time_index=r[:, 1].astype(np.int32),
                thread_id=r[:, 2].astype(np.int16), flags=r[:, 3].astype(np.uint16))


def _offsets(where):
    if isinstance(where, tuple):
        first, nframes, stride = where
        return [first + k * stride for k in range(nframes)]
    return [int(x) for x in np.asarray(where).tolist()]


def vdif_records(buf, where, frame_nbytes, header_nbytes, pattern, mask,
                 ref_seconds=0, ref_frame_nr=0, frame_rate=0, set_nframes=0):
    """bb_vdif_scan (`where` = (first_offset, nframes)) or bb_vdif_scan_at (`where` = offsets).
    A header word whose four bytes do not all lie inside the buffer reads as zero.  OK: the whole
    header lies inside the buffer and agrees with the pattern under the mask, and the frame fits.
    Time index: (seconds - ref_seconds) * frame_rate + frame_nr - ref_frame_nr, or the frame's
    number in the call when frame_rate = 0; fixed stride with set_nframes > 1: a frame whose
    frame_nr equals that of the first frame of its group of set_nframes takes that frame's seconds."""
    buf = _bytes(buf)
    n, F, H = len(buf), int(frame_nbytes), int(header_nbytes)
    fixed = isinstance(where, tuple)
    offs = _offsets((where[0], where[1], F) if fixed else where)
    nw = H // 4
    rows = []
    for i, off in enumerate(offs):
        w = [u32_at(buf, off + 4 * k) for k in range(nw)] + [0] * (8 - nw)
        f = orc.vdif_header_fields(w)
        inside = 0 <= off and off + H <= n
        ok = inside and all(((w[k] ^ (int(pattern[k]) & 0xffffffff)) & (int(mask[k]) & 0xffffffff)) == 0
                            for k in range(nw)) and off + F <= n
        seconds = f['seconds']
        if fixed and set_nframes > 1 and frame_rate > 0:
            lead = i - i % set_nframes
            loff = offs[lead]
            if lead != i and loff + 8 <= n and (u32_at(buf, loff + 4) & 0xffffff) == f['frame_nr']:
                seconds = u32_at(buf, loff) & 0x3fffffff
        tidx = (seconds - ref_seconds) * frame_rate + f['frame_nr'] - ref_frame_nr if frame_rate > 0 else i
        rows.append([off + H, _clamp(tidx), f['thread_id'],
                     (FRAME_OK if ok else 0) | (FRAME_INVALID if f['invalid_data'] else 0)])
    return _recs(rows)


def _bcd(v, ndigit):
    """Digits at face value (a nibble above 9 counts as that many units of its power of ten)
    and whether all of them are decimal."""
    r, m, ok = 0, 1, True
    for i in range(ndigit):
        d = (v >> (4 * i)) & 0xf
        ok = ok and d <= 9
        r += d * m
        m *= 10
    return r, ok


def mark5b_records(buf, where, ref_seconds=0, ref_frame_nr=0, frame_rate=0, by_position=0):
    """bb_mark5b_scan (`where` = (first_offset, nframes)) / bb_mark5b_scan_at (offsets).  A frame
    that does not lie wholly inside the buffer has no header (its words read as zero) and is not OK.
    OK: sync word (by_position: the frame is whole).  INVALID: whole and every payload word is the fill
    pattern.  Time index: ((jday * 86400 + seconds) - ref_seconds, plus 1000 days when below -500 days)
    * frame_rate + frame_nr - ref_frame_nr; the frame's number in the call with frame_rate = 0 or
    by_position."""
    buf = _bytes(buf)
    n = len(buf)
    offs = _offsets((where[0], where[1], M5B_FRAME) if isinstance(where, tuple) else where)
    rows = []
    for i, off in enumerate(offs):
        whole = 0 <= off and off + M5B_FRAME <= n
        w = [u32_at(buf, off + 4 * k) if whole else 0 for k in range(4)]
        try:
            f = orc.mark5b_header_fields(w)
            frame_nr, jday, secs = f['frame_nr'], f['jday'], f['seconds']
        except ValueError:      # a nibble above 9: at face value (the reference raises; not tested)
            frame_nr, jday, secs = w[1] & 0x7fff, _bcd(w[2] >> 20, 3)[0], _bcd(w[2] & 0xfffff, 5)[0]
        fill = whole and bool(np.all(buf[off + 16:off + M5B_FRAME].view('<u4') == M5B_FILL))
        if frame_rate > 0 and not by_position:
            ds = jday * 86400 + secs - ref_seconds
            if ds < -500 * 86400:
                ds += 1000 * 86400
            tidx = ds * frame_rate + frame_nr - ref_frame_nr
        else:
            tidx = i
        ok = whole if by_position else (whole and w[0] == M5B_SYNC)
        rows.append([off + 16, _clamp(tidx), 0, (FRAME_OK if ok else 0) | (FRAME_INVALID if fill else 0)])
    return _recs(rows)


def _leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def mark4_records(buf, where, ntrack, ref_year, ref_qms, frame_qms, by_position=0):
    """bb_mark4_scan (`where` = (first_offset, nframes)) / bb_mark4_scan_at (offsets).  A frame that
    does not lie wholly inside the buffer has an all-zero header and is not OK.  payload_offset is the
    frame start.  INVALID: any error flag of any track.  Time q of track 0 in quarter-ms since the
    start of the year (last ms digit d = d * 1.25 ms); a unit-year digit that is the one after
    ref_year's adds the length of ref_year, any third digit is not OK.  Time index: (q - ref_qms) /
    frame_qms rounded half away from zero, not OK unless exact; the frame's number in the call with
    frame_qms = 0 or by_position.  OK further needs the sync pattern and decimal BCD digits;
    by_position: OK = whole, nothing else looked at."""
    buf = _bytes(buf)
    n, isz, F = len(buf), ntrack // 8, ntrack * 2500
    offs = _offsets((where[0], where[1], F) if isinstance(where, tuple) else where)
    dt = orc.MARK4_DTYPES[ntrack]
    rows = []
    for i, off in enumerate(offs):
        whole = 0 <= off and off + F <= n
        stream = (buf[off:off + 160 * isz].copy().view(dt) if whole else np.zeros(160, dt))
        words = orc.mark4_stream2words(stream)
        f = orc.mark4_header_fields(words)
        ok = whole and bool(np.all(f['sync_pattern'] == 0xffffffff)) and not np.any(words[1] & 1)
        day, d1 = _bcd(int(f['bcd_day'][0]), 3)
        hour, d2 = _bcd(int(f['bcd_hour'][0]), 2)
        minute, d3 = _bcd(int(f['bcd_minute'][0]), 2)
        sec, d4 = _bcd(int(f['bcd_second'][0]), 2)
        ms, d5 = _bcd(int(f['bcd_fraction'][0]), 3)
        ok = ok and d1 and d2 and d3 and d4 and d5
        q = (((day * 24 + hour) * 60 + minute) * 60 + sec) * 4000 + 4 * ms + ms % 5
        uyear = int(f['bcd_unit_year'][0])
        if uyear == (ref_year + 1) % 10 and uyear != ref_year % 10:
            q += (366 if _leap(ref_year) else 365) * 86400 * 4000
        elif uyear != ref_year % 10:
            ok = False
        if by_position:
            ok, tidx = whole, i
        elif frame_qms > 0:
            dq = q - ref_qms
            tidx = (abs(dq) + frame_qms // 2) // frame_qms * (1 if dq >= 0 else -1)
            if tidx * frame_qms != dq:
                ok = False
        else:
            tidx = i
        rows.append([off, _clamp(tidx), 0, (FRAME_OK if ok else 0) | (0 if f['valid'] else FRAME_INVALID)])
    return _recs(rows)


# --------------------------------------------------------------------------
# index
# --------------------------------------------------------------------------
def build_index(recs, nframes_out, nslot=1, thread_slot=None):
    """bb_build_index: src[time_index * nslot + slot] = payload_offset for records that are OK, not
    INVALID, with 0 <= time_index < nframes_out and (with a thread map) 0 <= slot < nslot; -1 elsewhere."""
    src = np.full(nframes_out * nslot, -1, np.int64)
    for off, t, th, fl in zip(recs['payload_offset'], recs['time_index'], recs['thread_id'], recs['flags']):
        if not fl & FRAME_OK or fl & FRAME_INVALID or not 0 <= t < nframes_out:
            continue
        slot = 0 if thread_slot is None else int(thread_slot[int(th) & 0x3ff])
        if 0 <= slot < nslot:
            src[int(t) * nslot + slot] = off
    return src


def verify_count(recs, first_index, recs_per_index, nstrict):
    """bb_verify_records: the records that are not OK or, among the first nstrict, whose time index
    is not first_index + i // recs_per_index."""
    bad = 0
    for i, (t, fl) in enumerate(zip(recs['time_index'], recs['flags'])):
        if not fl & FRAME_OK or (i < nstrict and int(t) != first_index + i // recs_per_index):
            bad += 1
    return bad


def pack_recs(recs):
    """Host (n, 4) int32 image of bb_frame_rec records."""
    n = len(recs['payload_offset'])
    r = np.zeros((n, 4), np.int32)
    r[:, :2] = np.asarray(recs['payload_offset'], np.int64).reshape(-1, 1).view(np.int32)
    r[:, 2] = recs['time_index']
    r[:, 3] = (np.asarray(recs['thread_id']).astype(np.int16).view(np.uint16).astype(np.uint32)
               | np.asarray(recs['flags']).astype(np.uint32) << 16).astype(np.uint32).view(np.int32)
    return r


# --------------------------------------------------------------------------
# makers of valid headers and frames
# --------------------------------------------------------------------------
def vdif_header_words(frame_nbytes, header_nbytes=32, seconds=0, frame_nr=0, thread_id=0, invalid=0,
                      ref_epoch=28, lg2_nchan=0, bps=2, complex_data=0, station=0x4142, edv=0, w4_low=0,
                      w6=0, w7=0, version=1):
    legacy = header_nbytes == 16
    w = [(invalid & 1) << 31 | (1 if legacy else 0) << 30 | seconds & 0x3fffffff,
         (ref_epoch & 0x3f) << 24 | frame_nr & 0xffffff,
         (version & 7) << 29 | (lg2_nchan & 0x1f) << 24 | frame_nbytes // 8 & 0xffffff,
         (complex_data & 1) << 31 | (bps - 1 & 0x1f) << 26 | (thread_id & 0x3ff) << 16 | station & 0xffff]
    if not legacy:
        w += [(edv & 0xff) << 24 | w4_low & 0xffffff, 0xACABFEED if edv in (1, 3) else 0, w6, w7]
    return w


# masks under which a stream's headers agree (1-bits compared), by name
VDIF_MASKS = {
    'edv0': [0x40000000, 0x3f000000, 0xffffffff, 0xfc00ffff, 0xff000000, 0, 0, 0],
    'edv0_1thread': [0x40000000, 0x3f000000, 0xffffffff, 0xffffffff, 0xffffffff, 0, 0, 0],
    'edv3': [0x40000000, 0x3f000000, 0xffffffff, 0xfc00ffff, 0xffffffff, 0xffffffff, 0, 0xff000000],
    'legacy': [0x40000000, 0x3f000000, 0xffffffff, 0xfc00ffff, 0, 0, 0, 0],
    'word2_only': [0, 0, 0xffffffff, 0, 0, 0, 0, 0],
}


def mark5b_header_words(frame_nr=0, jday=0, seconds=0, user=0, tvg=0, frac=0, w2=None):
    def enc(v, nd):
        return sum((v // 10 ** i % 10) << 4 * i for i in range(nd))
    if w2 is None:
        w2 = enc(jday, 3) << 20 | enc(seconds, 5)
    return [M5B_SYNC, (user & 0xffff) << 16 | (tvg & 1) << 15 | frame_nr & 0x7fff, w2,
            (frac & 0xffff) << 16 | crc16_mark5b(w2, frac & 0xffff)]


def mark4_words2stream(words, ntrack):
    """(5, ntrack) header words -> 160 stream words: bit t of stream word 32 j + i is bit 31 - i of
    header word j of track t (inverse of bb_oracle_np.mark4_stream2words)."""
    words = np.asarray(words, np.uint32)
    dt = np.dtype(orc.MARK4_DTYPES[ntrack])
    stream = np.zeros(160, dt)
    for j in range(5):
        for i in range(32):
            bits = (words[j] >> np.uint32(31 - i)) & np.uint32(1)
            v = 0
            for t in np.nonzero(bits)[0]:
                v |= 1 << int(t)
            stream[32 * j + i] = v
    return stream


def mark4_header_stream(ntrack, uyear=0, day=1, hour=0, minute=0, sec=0, ms=0, flags=0, w0=0,
                        bcd=None):
    """Header bytes of one Mark 4 frame, the same time on every track.  `flags`: the four error-flag
    bits (word 1 bits 15..12) of track 3; `bcd` overrides the raw (w3, w4 >> 12) time-code fields."""
    def enc(v, nd):
        return sum((v // 10 ** i % 10) << 4 * i for i in range(nd))
    w = np.zeros((5, ntrack), np.uint32)
    w[0] = w0
    w[1] = 0x00c10000 | np.arange(ntrack, dtype=np.uint32) << np.uint32(24) & np.uint32(0x3f000000)
    w[1] &= np.uint32(0xfffffffe)
    w[1, 3 % ntrack] |= np.uint32((flags & 0xf) << 12)
    w[2] = 0xffffffff
    w3 = uyear << 28 | enc(day, 3) << 16 | enc(hour, 2) << 8 | enc(minute, 2)
    w4h = enc(sec, 2) << 12 | enc(ms, 3)
    if bcd is not None:
        w3, w4h = bcd
    w[3] = w3
    w[4] = (w4h & 0xfffff) << 12
    return mark4_words2stream(w, ntrack).view(np.uint8)


# --------------------------------------------------------------------------
# the small buffers of tests/golden/locate_whole_cases.json
# --------------------------------------------------------------------------
def build_whole_case(spec):
    """Seeded buffer of a few frames for one recorded case -> (full, nbytes): the case is
    full[:nbytes]; behind it the file goes on (the rest of the following frame and one more).

    spec: fmt ('vdif' | 'mark5b' | 'mark4'), seed, nframes, start (junk bytes in front), slips
    (per gap between frames: > 0 junk bytes inserted, < 0 bytes dropped from the end of the frame in
    front), damaged (frames whose header is damaged in place), cut (bytes of the header that follows
    the last whole frame that are still inside; None: the buffer ends with a whole frame ... or with
    cut_short bytes missing from it), and the format's parameters."""
    rng = np.random.default_rng(spec['seed'])
    fmt = spec['fmt']
    if fmt == 'vdif':
        F, H = spec['frame_nbytes'], spec['header_nbytes']
    elif fmt == 'mark5b':
        F, H = M5B_FRAME, 16
    else:
        F, H = spec['ntrack'] * 2500, spec['ntrack'] * 20
    nfr = spec['nframes']
    parts = [rng.integers(0, 256, spec['start'], dtype=np.uint8)]
    bounds = []
    for k in range(nfr + 2):
        frame = rng.integers(0, 256, F, dtype=np.uint8)
        if fmt == 'vdif':
            w = vdif_header_words(F, H, seconds=100 + k // 4, frame_nr=k % 4, thread_id=k % 2,
                                  edv=spec.get('edv', 0), station=spec.get('station', 0x4142))
            frame[:H] = words_to_bytes(w)
        elif fmt == 'mark5b':
            w = mark5b_header_words(frame_nr=k, jday=123, seconds=4567, user=spec.get('user', 0xf00f))
            frame[:16] = words_to_bytes(w)
        else:
            frame[:H] = mark4_header_stream(spec['ntrack'], uyear=4, day=200, sec=k % 60)
        if k in spec.get('damaged', []):
            if fmt == 'vdif':
                frame[10] ^= 0x55                   # word 2 (frame length)
            elif fmt == 'mark5b':
                frame[2] ^= 0x55                    # sync word
            else:
                frame[70 * spec['ntrack'] // 8] ^= 0x10    # one of the ones
        slip = spec['slips'][k - 1] if 0 < k <= len(spec['slips']) else 0
        if k and slip > 0:
            parts.append(rng.integers(0, 256, slip, dtype=np.uint8))
        elif k and slip < 0:
            parts[-1] = parts[-1][:slip]
        if k == nfr:
            bounds.append(sum(len(p) for p in parts))
        parts.append(frame)
    full = np.concatenate(parts)
    end = bounds[0]
    nbytes = end + spec['cut'] if spec.get('cut') is not None else end - spec.get('cut_short', 0)
    return full, int(nbytes)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
