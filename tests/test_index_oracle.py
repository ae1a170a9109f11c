"""Pins the brute-force restatements of the frame search and header scan
(oracle/bb_index_np.py, written from include/bbdecode.h) to the reference's
recorded answers (tests/golden/locate_whole_cases.json, made by
oracle/gen_golden_locate_whole.py) and to what the suite already knows about the
sample files.  No GPU: tests/test_index_kernels_gpu.py compares the kernels with
these restatements."""
import json

import numpy as np
import pytest

from conftest import golden_path, load_file

import bb_index_np as ix
import bb_oracle_np as orc

with open(golden_path('locate_whole_cases.json')) as _f:
    WHOLE = json.load(_f)['cases']


def whole_case_pattern(c):
    pat = ix.vdif_header_words(c['frame_nbytes'], c['header_nbytes'], seconds=100, edv=c.get('edv', 0))
    return pat + [0] * (8 - len(pat)), ix.VDIF_MASKS[c['mask']]


def whole_case_want(c):
    """The reference's recorded answer (VDIF: combined as include/bbdecode.h states)."""
    if c['fmt'] == 'vdif':
        return ix.vdif_combine(c['answers'], c['nbytes'], c['frame_nbytes'], c['header_nbytes'])
    return c['answers']['ref']


def whole_case_oracle(c, buf):
    if c['fmt'] == 'vdif':
        pat, msk = whole_case_pattern(c)
        return ix.vdif_locate(buf, c['frame_nbytes'], c['header_nbytes'], pat, msk).tolist()
    if c['fmt'] == 'mark5b':
        return ix.mark5b_locate(buf, c.get('w1_pattern', 0), c.get('w1_mask', 0)).tolist()
    return ix.mark4_locate(buf, c['ntrack']).tolist()


@pytest.mark.parametrize('fmt', ['vdif', 'mark5b', 'mark4'])
def test_restatement_equals_recorded_reference(fmt):
    """Every recorded case, exact lists.  The buffer is rebuilt from its seed and its digest
    checked first: a NumPy whose generator differs is noticed."""
    cases = [c for c in WHOLE if c['fmt'] == fmt]
    assert len(cases) > 100
    for c in cases:
        full, nbytes = ix.build_whole_case(c)
        assert nbytes == c['nbytes'] and ix.sha256(full[:nbytes]) == c['sha256'], c['seed']
        assert ix.sha256(full) == c['sha256_full'], c['seed']
        assert whole_case_oracle(c, full[:nbytes]) == whole_case_want(c), c


def test_recorded_cases_tell_the_rules_apart():
    """The file holds the cases in which the edges matter: a Mark 5B frame with an unaligned
    start whose successor's sync word is cut by the end (kept), one followed by exactly four
    bytes that are no sync word (kept: the reference's test is strict), by five (dropped)."""
    def find(**kw):
        return [c for c in WHOLE if all(c.get(k) == v for k, v in kw.items())]
    for start, cut in ((1, 4), (1, 5), (1, 6), (2, 4), (2, 5), (3, 4)):
        c, = find(fmt='mark5b', nframes=2, start=start, cut=cut, damaged=[], w1_mask=None)
        assert c['answers']['ref'] == [start, start + 10016]
    c, = find(fmt='mark5b', nframes=2, start=1, cut=4, damaged=[2], w1_mask=None)
    assert c['answers']['ref'] == [1, 10017]
    c, = find(fmt='mark5b', nframes=2, start=1, cut=5, damaged=[2], w1_mask=None)
    assert c['answers']['ref'] == [1]


def _implied(size, first, frame_nbytes):
    return list(range(first, size - frame_nbytes + 1, frame_nbytes))


def test_sample_files(manifest):
    """On the sample files the searches return exactly the frame offsets the manifest implies."""
    m = manifest['sample_vdif']
    raw = load_file(m['file'])
    assert ix.vdif_locate(raw, 5032, 32, m['header0_words'], m['stream_mask']).tolist() == _implied(len(raw), 0, 5032)
    raw = load_file(manifest['vdif_triple']['file'])
    h0 = raw[:32].view('<u4').tolist()
    assert ix.vdif_locate(raw, 5032, 32, h0, m['stream_mask']).tolist() == [k * 5032 for k in range(48)]
    raw = load_file('samples/sample.m5b')
    assert ix.mark5b_locate(raw).tolist() == [0, 10016, 20032, 30048]
    for name in ('sample_m4', 'sample_16track_m4', 'sample_32track_m4', 'sample_32track_fanout2_m4',
                 'sample_64track_fanout2_ft_m4', 'm4_t16_f4', 'm4_t32_f2', 'm4_t32_f4', 'm4_t64_f4'):
        m = manifest[name]
        raw = load_file(m['file'])
        want = _implied(len(raw), m.get('offset0', 0), m['ntrack'] * 2500)
        assert len(want) >= 1
        assert ix.mark4_locate(raw, m['ntrack']).tolist() == want, name


def test_damaged_buffers_of_the_raw_kernel_tests():
    """The three damaged buffers of tests/test_corrupt_gpu.py: exactly the lists asserted there."""
    with open(golden_path('vdif_corrupt_cases.json')) as f:
        case = json.load(f)[9]
    base = load_file('synth/vdif_triple.bin').copy()
    keep = np.ones(len(base), bool)
    for lo, hi in case['remove']:
        keep[lo:hi] = False
    for pos in case.get('flip', []):
        base[pos] ^= 0x55
    blob = base[keep]
    from baseband_amd.vdif import VDIFHeader
    pattern, mask = VDIFHeader(blob[:32].view('<u4')).invariant_pattern()
    want = [k * 5032 for k in range(30)] + [k * 5032 - 10 for k in range(32, 48)]
    assert ix.vdif_locate(blob, 5032, 32, pattern, mask).tolist() == want

    base = load_file('samples/sample.m5b')
    blob = np.concatenate([base[:20100], base[20101:]])
    blob[30047 + 9] ^= 0xff
    assert ix.mark5b_locate(blob).tolist() == [0, 10016]
    recs = ix.mark5b_records(blob, [0, 10016, 20032, 30047])
    assert recs['payload_offset'].tolist() == [16, 10032, 20048, 30063]
    blob = base.copy()
    user = int(blob[4:8].view('<u4')[0]) & 0xffff0000
    blob[2 * 10016 + 6] ^= 0x5a
    assert ix.mark5b_locate(blob).tolist() == [0, 10016, 20032, 30048]
    assert ix.mark5b_locate(blob, user, 0xffff0000).tolist() == [0, 30048]

    base = np.load(golden_path('fixed_corrupt_files.npz'))['m4_fake']
    blob = np.concatenate([base[:80010], base[80100:]])
    assert ix.mark4_locate(blob, 16).tolist() == [0] + [k * 40000 - 90 for k in range(2, 8)]


def test_record_fields_of_the_samples(manifest):
    """Record fields equal the *_header_fields of the same headers, and the time indices are the
    ones the files are known to hold."""
    m = manifest['sample_vdif']
    raw = load_file(m['file'])
    h0 = orc.vdif_header_fields(m['header0_words'])
    n = len(raw) // 5032
    args = (5032, 32, m['header0_words'], m['stream_mask'], h0['seconds'], h0['frame_nr'], 1600)
    recs = ix.vdif_records(raw, (0, n), *args)
    at = ix.vdif_records(raw, [k * 5032 for k in range(n)], *args)
    for k in range(n):
        f = orc.vdif_header_fields(raw[k * 5032:k * 5032 + 32].view('<u4'))
        assert recs['thread_id'][k] == f['thread_id'] and recs['payload_offset'][k] == k * 5032 + 32
        assert recs['time_index'][k] == (f['seconds'] - h0['seconds']) * 1600 + f['frame_nr'] - h0['frame_nr']
        assert recs['flags'][k] == ix.FRAME_OK | (ix.FRAME_INVALID if f['invalid_data'] else 0)
    assert recs['time_index'].tolist() == [0] * 8 + [1] * 8
    assert sorted(recs['thread_id'][:8].tolist()) == m['thread_ids']
    for key in recs:
        assert recs[key].tolist() == at[key].tolist()

    raw = load_file('samples/sample.m5b')
    f0 = orc.mark5b_header_fields(raw[:16].view('<u4'))
    assert ix.crc16_mark5b_ok(*[int(x) for x in raw[8:16].view('<u4')])
    assert ix.mark5b_header_words(f0['frame_nr'], f0['jday'], f0['seconds'], f0['user'], int(f0['internal_tvg']),
                                  f0['bcd_fraction']) == raw[:16].view('<u4').tolist()
    recs = ix.mark5b_records(raw, (0, 4), f0['jday'] * 86400 + f0['seconds'], f0['frame_nr'], 6400)
    assert recs['time_index'].tolist() == [0, 1, 2, 3]
    assert recs['flags'].tolist() == [ix.FRAME_OK] * 4
    assert recs['payload_offset'].tolist() == [16 + k * 10016 for k in range(4)]

    for name, year in (('sample_m4', 2014), ('sample_16track_m4', 2013), ('sample_32track_m4', 2015),
                       ('m4_t64_f4', 2015)):
        m = manifest[name]
        raw = load_file(m['file'])
        nt, off0 = m['ntrack'], m.get('offset0', 0)
        F = nt * 2500
        nfr = (len(raw) - off0) // F
        stream = raw[off0:off0 + 20 * nt].view(orc.MARK4_DTYPES[nt])
        f = orc.mark4_header_fields(orc.mark4_stream2words(stream))
        ref_qms = orc.mark4_time_quarter_ms(f)
        frame_qms = 4000 // m['frame_rate'] if 'frame_rate' in m else \
            round(m['samples_per_frame'] / m['sample_rate_hz'] * 4000)
        recs = ix.mark4_records(raw, (off0, nfr), nt, year, ref_qms, frame_qms)
        assert recs['time_index'].tolist() == list(range(nfr)), name
        assert recs['payload_offset'].tolist() == [off0 + k * F for k in range(nfr)]
        want_flags = [ix.FRAME_OK | (ix.FRAME_INVALID if k in m.get('invalid', []) else 0) for k in range(nfr)]
        assert recs['flags'].tolist() == want_flags, name
        assert np.array_equal(ix.mark4_words2stream(orc.mark4_stream2words(stream), nt), stream)


def test_index_and_verify_restatements():
    recs = dict(payload_offset=np.array([32, 5064, 10096, 15128, 20160], np.int64),
                time_index=np.array([0, 0, 1, 5, -1], np.int32),
                thread_id=np.array([0, 1, 0, 1, 0], np.int16),
                flags=np.array([1, 1, 3, 1, 1], np.uint16))
    slot = np.full(1024, -1, np.int16)
    slot[0], slot[1] = 1, 0
    assert ix.build_index(recs, 2, 2, slot).tolist() == [5064, 32, -1, -1]
    assert ix.build_index(recs, 6, 1, None).tolist() == [5064, -1, -1, -1, -1, 15128]
    assert ix.verify_count(recs, 0, 2, 4) == 1          # record 3 is out of place
    assert ix.verify_count(recs, 0, 2, 3) == 0
    recs['flags'][1] = 2
    assert ix.verify_count(recs, 0, 2, 0) == 1
    assert ix.pack_recs(recs).shape == (5, 4)
