"""tests/hitmask_model.py by hand: the gap closing at gap and gap + 1, runs that touch an end of the sequence, mates closed
separately, an empty sequence, gap 0 as the identity, the record and the counts.  No GPU, no library."""
import numpy as np

from tests import builder_model as bmod
from tests import hitmask_model as hm


def cov(s):
    return np.array([c == "1" for c in s], dtype=bool)


def text(c):
    return "".join("1" if x else "0" for x in c)


def test_closing_at_gap_and_gap_plus_one():
    c = cov("0111000110000111")  # inner runs of 3 and 4
    assert text(hm.close(c, 2)[0]) == "0111000110000111" and hm.close(c, 2)[1] == 0
    assert text(hm.close(c, 3)[0]) == "0111111110000111" and hm.close(c, 3)[1] == 3
    assert text(hm.close(c, 4)[0]) == "0111111111111111" and hm.close(c, 4)[1] == 7
    assert text(hm.close(c, 4096)[0]) == "0111111111111111"


def test_runs_that_touch_an_end_are_never_closed():
    assert text(hm.close(cov("0001110"), 100)[0]) == "0001110"
    assert text(hm.close(cov("1000000"), 100)[0]) == "1000000"
    assert text(hm.close(cov("0000001"), 100)[0]) == "0000001"
    assert text(hm.close(cov("0000000"), 100)[0]) == "0000000"
    assert text(hm.close(cov("101"), 1)[0]) == "111"
    assert text(hm.close(cov("1"), 1)[0]) == "1" and text(hm.close(cov("10"), 1)[0]) == "10"


def test_gap_zero_is_the_identity_and_the_input_is_not_changed():
    c = cov("1010010001")
    keep = c.copy()
    out, added = hm.close(c, 0)
    assert np.array_equal(out, keep) and added == 0
    out, added = hm.close(c, 2)
    assert text(out) == "1111110001" and added == 3 and np.array_equal(c, keep)


def test_an_empty_sequence():
    out, added = hm.close(cov(""), 34)
    assert out.shape == (0,) and added == 0


def test_mates_are_closed_separately_on_a_bitmap():
    """two sequences back to back: the uncovered bases between the last covered base of one and the first of the next are two runs
    that touch an end each, whatever the gap"""
    bits = cov("1100" + "0011" + "101")  # sequences [0, 4), [4, 8), [8, 11)
    n = len(bits)
    words = np.packbits(np.concatenate((bits, np.zeros(32 - n, dtype=bool))).astype(np.uint8), bitorder="little").view("<u4")
    got, added = hm.close_words(words, n, [(0, 4), (4, 4), (8, 3)], 100)
    assert text(hm.bits_of(got, n)) == "1100" + "0011" + "111" and added == 1
    # as ONE sequence everything between the first and the last covered base closes
    got, added = hm.close_words(words, n, [(0, n)], 100)
    assert text(hm.bits_of(got, n)) == "1" * n and added == 5
    # a skipped sequence keeps its bits
    got, added = hm.close_words(words, n, [(0, 4), (4, 4), (8, 3)], 100, skip={2})
    assert text(hm.bits_of(got, n)) == text(bits) and added == 0


def test_close_words_across_word_boundaries():
    n = 200
    bits = np.zeros(n, dtype=bool)
    bits[[3, 31, 33, 64, 165]] = True  # runs of 27, 1, 30, 100 inside [3, 166)
    words = np.packbits(np.concatenate((bits, np.zeros(224 - n, dtype=bool))).astype(np.uint8), bitorder="little").view("<u4")
    got, added = hm.close_words(words, n, [(0, n)], 99)
    want = bits.copy()
    want[3:65] = True
    assert np.array_equal(hm.bits_of(got, n), want) and added == 27 + 1 + 30
    got, added = hm.close_words(words, n, [(0, n)], 100)
    want[64:166] = True
    assert np.array_equal(hm.bits_of(got, n), want) and added == 27 + 1 + 30 + 100


def test_the_record_keeps_the_inputs_own_bases():
    r = bmod.parse_record(b"@id x\r\nacgTNacg\r\n+id\r\nIIII#III\r\n", True)
    assert hm.put(r) == b"@id x\nacgTNacg\n+\nIIII#III\n"
    assert hm.put(r, cov("01100001")) == b"@id x\naNNTNacN\n+\nIIII#III\n"
    f = bmod.parse_record(b">f\nAC\nGT\n", False)
    assert hm.put(f, cov("1001")) == b">f\nNCGN\n"


class _NoDB:
    """a database without a minimizer: no base is covered"""
    k, l = 35, 31
    toggle_mask = spaced_seed_mask = 0
    revcom_version, ambiguity_rule, min_hash = 1, 1, 0

    def get(self, mz):
        return 0


def test_the_counts_without_a_covered_base():
    recs = [[bmod.parse_record(b"@a\n" + b"ACGT" * 10 + b"\n+\n" + b"I" * 40 + b"\n", True),
             bmod.parse_record(b"@b\n\n+\n\n", True)]]
    read_as = [(recs[0][0].seq,), (b"",)]
    texts, counts, masks = hm.outputs(_NoDB(), recs, read_as, [5, 0], 34)
    assert texts == [recs[0][0].raw + recs[0][1].raw] and counts == (40, 0, 0)
    assert masks[1] == [None] and not masks[0][0][1].any()
