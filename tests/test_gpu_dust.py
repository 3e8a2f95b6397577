"""nh_dust_mask on the GPU (nohuman_amd/csrc/nh_dust.hip) against the model (tests/dust_model.py mask), byte for byte, and the
count of masked bases.  Every input's model mask is computed once, on the CPU, and checked to hold a real share of masked and of
clear bases before the GPU is used: two all-clear masks that agree show nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import dust_model as dm

pytestmark = pytest.mark.gpu
NH_EINVAL = -1


def gpu_mask(seqs):
    import nohuman_amd
    return nohuman_amd.dust_mask(seqs)


def raw_mask(buf: bytearray, starts, lens, n_seg=None, n_bytes=None, null=()):
    """nh_dust_mask through ctypes on `buf` in place -> (return code, masked_bases)"""
    from nohuman_amd import _lib
    cbuf = (C.c_char * max(len(buf), 1)).from_buffer(buf)
    st = (C.c_uint64 * max(len(starts), 1))(*starts)
    ln = (C.c_uint64 * max(len(lens), 1))(*lens)
    masked = C.c_uint64(0)
    rc = _lib.lib().nh_dust_mask(0, None if "text" in null else C.cast(cbuf, C.c_void_p), len(buf) if n_bytes is None else n_bytes,
                                 None if "starts" in null else st, None if "lens" in null else ln,
                                 len(starts) if n_seg is None else n_seg, None if "masked" in null else C.byref(masked))
    del cbuf
    return rc, masked.value


def share_of_acgt(seqs, masks) -> float:
    acgt = sum(sum(b - a for a, b in dm.runs(s)) for s in seqs)
    return sum(int(m.sum()) for m in masks) / acgt


def assert_same(got, seqs, masks):
    assert len(got) == len(seqs)
    for i, (g, s, m) in enumerate(zip(got, seqs, masks)):
        if g != dm.apply(s, m):
            gm = np.frombuffer(g, np.uint8) != np.frombuffer(s, np.uint8)
            bad = np.flatnonzero(gm != m)
            raise AssertionError("sequence %d of %d bases: %d bases differ from the model, the first at %d" % (i, len(s), bad.size, bad[0]))


@pytest.fixture(scope="module")
def every_length():
    """one segment of every length 1 .. 1300, low-complexity content from mixed generators"""
    rng = np.random.default_rng(64)
    seqs = []
    for n in range(1, 1301):
        k = n % 4
        seqs.append(dm.mixed(rng, n, flank=(10, 40, 120, 25)[k], longest=(90, 30, 200, 64)[k], n_share=0.002 if k == 1 else 0.0,
                             lower_share=0.3 if k == 2 else 0.0))
    masks = [dm.mask_bool(s) for s in seqs]
    return seqs, masks


def test_every_length(every_length):
    seqs, masks = every_length
    assert 0.05 < share_of_acgt(seqs, masks) < 0.95
    got, n = gpu_mask(seqs)
    assert_same(got, seqs, masks)
    assert n == sum(int(m.sum()) for m in masks)


def test_long_segments():
    rng = np.random.default_rng(65)
    planted, where = dm.plant(rng, dm.iid(rng, 200_000), range(5, 301))
    assert len(where) == 296 and where[-1][0] + 300 <= 200_000
    m = dm.mask_bool(planted)
    assert 0.05 < share_of_acgt([planted], [m]) < 0.95
    all_a = b"A" * 65536  # every tile border lies inside a masked stretch
    got, n = gpu_mask([planted, all_a])
    assert_same(got, [planted, all_a], [m, np.ones(65536, bool)])
    assert n == int(m.sum()) + 65536


def test_segment_borders():
    rng = np.random.default_rng(66)
    seqs = [b"CGTCAGTAAAA", b"AAAATGCAGTC", b"", b"ACACAC", b"ACACAC", b"A", b"AA", b"", b"AAAAAAA", b"AAA", b"AAAA"]
    # (the joined ends would be maskable: the model says so)
    assert dm.masked_count(seqs[0] + seqs[1]) == 8 and dm.masked_count(seqs[3] + seqs[4]) == 12
    # an N at every offset -64 .. +64 around the middle of a planted stretch of 40 bases
    for off in range(-64, 65):
        s = bytearray(dm.iid(rng, 100) + dm.stretch(rng, 40) + dm.iid(rng, 100))
        s[120 + off] = ord("N")
        seqs.append(bytes(s))
    masks = [dm.mask_bool(s) for s in seqs]
    assert not any(m.any() for m in masks[:8]) and masks[8].all() and not masks[9].any() and not masks[10].any()
    assert 0.05 < share_of_acgt(seqs, masks) < 0.95
    got, n = gpu_mask(seqs)
    assert_same(got, seqs, masks)
    assert n == sum(int(m.sum()) for m in masks)


def test_bytes_between_segments_stay():
    """segments with gaps between them: the gaps' bytes (maskable, had they been in a segment) are neither changed nor counted"""
    rng = np.random.default_rng(67)
    segs = [dm.mixed(rng, n) for n in (500, 37, 800, 7, 1200)]
    gap = b"A" * 70
    buf = bytearray(gap)
    starts = []
    for s in segs:
        starts.append(len(buf))
        buf += s + gap
    masks = [dm.mask_bool(s) for s in segs]
    assert 0.05 < share_of_acgt(segs, masks) < 0.95
    want = bytearray(buf)
    for a, s, m in zip(starts, segs, masks):
        want[a:a + len(s)] = dm.apply(s, m)
    rc, n = raw_mask(buf, starts, [len(s) for s in segs])
    assert rc == 0 and n == sum(int(m.sum()) for m in masks)
    assert buf == want


def test_edge_requests():
    from nohuman_amd import _lib
    text = b"ACGT" * 20  # masked whole, were it masked
    buf = bytearray(text)
    assert raw_mask(buf, [], [], n_seg=0) == (0, 0) and buf == text
    assert raw_mask(buf, [0, 80, 3], [0, 0, 0]) == (0, 0) and buf == text          # empty segments, one at the very end
    for starts, lens in (([0, 70], [10, 11]), ([81], [0]), ([0], [81]), ([1 << 63], [1 << 63]), ([2], [(1 << 64) - 1])):
        rc, n = raw_mask(buf, starts, lens)
        assert rc == NH_EINVAL and n == 0 and buf == text, (starts, lens)
        assert _lib.lib().nh_last_error().decode().startswith("nh_dust_mask:")
    for null in ("text", "starts", "lens"):
        assert raw_mask(buf, [0], [80], null=(null,))[0] == NH_EINVAL and buf == text
    rc, _ = raw_mask(buf, [0], [80], null=("masked",))                            # the count is optional
    assert rc == 0 and buf == b"N" * 80
    got, n = gpu_mask(b"acgt" * 20)                                               # one sequence alone; lowercase
    assert got == [b"N" * 80] and n == 80
    assert gpu_mask([]) == ([], 0)
