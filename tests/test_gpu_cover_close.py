"""k_cover_close on the GPU (nh_cover_close_device; nohuman_amd/csrc/nh_cover.hip) against tests/hitmask_model.close_words on forged
bitmaps: no database is asked, the bitmap is whatever the test says.  Bits outside every sequence are prefilled and must stay."""
import numpy as np
import pytest

from tests import hitmask_model as hm
from tests.test_gpu_cover import dev_tables, error_bit_is_clear

pytestmark = pytest.mark.gpu


def words_of(bits):
    n = len(bits)
    pad = np.zeros((-n) % 32, dtype=bool)
    return np.packbits(np.concatenate((bits, pad)).astype(np.uint8), bitorder="little").view("<u4").copy()


def gpu_close(eng, words, text_len, recs, gap, count=True, start=5):
    """-> (the bitmap's words, the counter: it is added to, it started at `start`)"""
    import torch
    d_c = torch.from_numpy(np.concatenate((words, np.full(1, 0xA5A5A5A5, np.uint32))).view(np.int32).copy()).cuda()
    d_s, d_l = dev_tables(recs)
    d_n = torch.full((1,), start, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.cover_close_device(d_c.data_ptr(), text_len, d_s.data_ptr(), d_l.data_ptr(), len(recs), gap, d_n.data_ptr() if count else 0)
    torch.cuda.synchronize()
    out = d_c.cpu().numpy().view(np.uint32)
    assert out[-1] == 0xA5A5A5A5  # (the word behind the bitmap)
    return out[:-1], int(d_n.cpu()[0]) - start


def check(eng, bits, recs, gap, skip=()):
    n = len(bits)
    words = words_of(bits)
    want, added = hm.close_words(words, n, recs, gap, skip)
    got, counted = gpu_close(eng, words, n, recs, gap)
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, "gap %d: %d words differ, first %d: got %08x, want %08x, was %08x" % (
        gap, diff.size, diff[0], got[diff[0]], want[diff[0]], words[diff[0]])
    assert counted == added, (gap, counted, added)
    got2, _ = gpu_close(eng, words, n, recs, gap, count=False)  # (no counter: the same bitmap)
    assert np.array_equal(got2, want)
    return want, added


def test_sequences_back_to_back_in_one_word(toy_engine):
    """three sequences in one word, every gap between them touches an end; the bits outside them stay"""
    bits = np.array([c == "1" for c in "1" + "1100" + "0011" + "101" + "0" + "1001" + "111"], dtype=bool)
    recs = [(1, 4), (5, 4), (9, 3), (13, 4)]
    for gap in (1, 2, 100):
        want, added = check(toy_engine, bits, recs, gap)
        assert added == (1 if gap == 1 else 3)
    error_bit_is_clear(toy_engine)


@pytest.mark.parametrize("gap", [1, 31, 32, 33, 34, 100, 4096])
def test_a_run_of_exactly_gap_and_of_gap_plus_one(toy_engine, gap):
    """at every alignment of the run's start in its word"""
    for sh in (0, 1, 30, 31):
        bits = np.zeros(3 * gap + 200, dtype=bool)
        a = 40 + sh
        bits[a - 2:a] = True              # .. 11 [gap zeros] 1 [gap + 1 zeros] 11
        bits[a + gap] = True
        bits[a + 2 * gap + 2:a + 2 * gap + 4] = True
        want, added = check(toy_engine, bits, [(7, len(bits) - 9)], gap)
        assert added == gap
        assert hm.bits_of(want, len(bits))[a:a + gap].all() and not hm.bits_of(want, len(bits))[a + gap + 1:a + 2 * gap + 2].any()


def test_runs_across_word_boundaries_and_several_words(toy_engine):
    rng = np.random.default_rng(3)
    n = 5000
    bits = np.zeros(n, dtype=bool)
    p = 0
    while p < n:  # covered runs of 1..40, uncovered runs of 1..140
        c = int(rng.integers(1, 41))
        bits[p:p + c] = True
        p += c + int(rng.integers(1, 141))
    recs = [(0, 1500), (1500, 1), (1501, 2), (1503, 31), (1534, 66), (1600, 3400)]
    seen = set()
    for gap in (1, 31, 64, 100, 139, 4096):
        want, added = check(toy_engine, bits, recs, gap)
        seen.add(added)
    assert len(seen) >= 5  # (the gaps tell the runs apart)
    error_bit_is_clear(toy_engine)


def test_a_sequence_shorter_than_a_word_and_runs_at_its_ends(toy_engine):
    bits = np.array([c == "1" for c in "000" + "0010010" + "0" * 30 + "1000001" + "0001" + "1000"], dtype=bool)
    recs = [(3, 7), (40, 7), (47, 4), (51, 4)]
    want, added = check(toy_engine, bits, recs, 5)
    assert added == 2 + 5  # the two inner runs; the runs at a sequence's start or end stay
    want, added = check(toy_engine, bits, recs, 4)
    assert added == 2
    # the same bits as one sequence: the runs at the borders are inner runs now
    want, added = check(toy_engine, bits, [(0, len(bits))], 34)
    assert added > 7


def test_gap_zero_and_no_sequence_launch_nothing(toy_engine):
    bits = np.array([c == "1" for c in "1010010001" * 7], dtype=bool)
    words = words_of(bits)
    got, counted = gpu_close(toy_engine, words, len(bits), [(0, len(bits))], 0)
    assert np.array_equal(got, words) and counted == 0
    got, counted = gpu_close(toy_engine, words, len(bits), [], 34)
    assert np.array_equal(got, words) and counted == 0
    error_bit_is_clear(toy_engine)


def test_many_sequences_and_a_long_one(toy_engine):
    """more sequences than one launch has waves for at once in a block, and a sequence of many rounds of 64 words"""
    rng = np.random.default_rng(4)
    lens = [int(x) for x in rng.integers(0, 90, size=700)] + [70000]
    recs, p = [], 3
    for ln in lens:
        recs.append((p, ln))
        p += ln + int(rng.integers(0, 3))
    bits = rng.random(p + 9) < 0.04
    want, added = check(toy_engine, bits, recs, 34)
    assert added > 1000
    check(toy_engine, bits, recs, 2000)


def test_a_sequence_outside_the_text_is_skipped(toy_engine):
    from nohuman_amd import EngineError
    bits = np.array([c == "1" for c in "1001" * 50], dtype=bool)
    n = len(bits)
    recs = [(0, 40), (40, 40), (n - 20, 40), (n + 500, 8), (80, 40), (2 ** 40, 2 ** 32 - 1)]
    want, added = check(toy_engine, bits, recs, 2, skip={2, 3, 5})
    assert added == 3 * 10 * 2  # (ten runs of two bases in each of the three sequences that are closed)
    with pytest.raises(EngineError) as ei:
        error_bit_is_clear(toy_engine)
    assert ei.value.code == -4 and "host intervals" in ei.value.message
    error_bit_is_clear(toy_engine)  # read once, the word is clean again


def test_a_gap_above_the_cap_is_refused(toy_engine):
    from nohuman_amd import EngineError
    words = words_of(np.ones(64, dtype=bool))
    with pytest.raises(EngineError) as ei:
        gpu_close(toy_engine, words, 64, [(0, 64)], 4097)
    assert ei.value.code == -1 and "NH_HOST_GAP_MAX" in ei.value.message
