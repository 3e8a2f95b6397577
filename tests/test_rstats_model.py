"""The Python model of the read statistics (tests/rstats_model.py) on cases worked out by hand, and what the corpora of
tests/test_gpu_rstats_run.py contain: reads of both classes, so that a run that equals the model cannot pass with the class
index swapped or one class never counted.  No GPU needed."""
import numpy as np

from tests import qmask_model as qm
from tests import rstats_model as rm


def test_median_and_n50_of_three_reads():
    assert rm.median([2, 10, 3]) == 3 and rm.n50([2, 10, 3]) == 10          # 10 alone holds 10 of 15 bases
    assert rm.median([4, 4, 4]) == 4 and rm.n50([4, 4, 4]) == 4
    assert rm.median([1, 2, 3, 4]) == 2                                       # the LOWER of the two middle ones
    assert rm.median([7]) == 7 and rm.n50([7]) == 7
    assert rm.median([]) == 0 and rm.n50([]) == 0
    assert rm.median([0, 0]) == 0 and rm.n50([0, 0]) == 0                     # reads without bases
    assert rm.n50([1] * 10 + [5]) == 1                                        # 5 holds 5 of 15: not half


def test_n50_tie_at_the_half_way_point():
    assert rm.n50([5, 3, 2]) == 5      # 5 holds exactly half of 10: 2 * 5 >= 10
    assert rm.n50([4, 3, 3]) == 3      # 4 holds 4 of 10; 4 + 3 = 7 do: 14 >= 10
    assert rm.n50([6, 6]) == 6


READS = [(0, False, b"ACGTN", b"IIII!"), (0, True, b"GGCC", b"5555"), (0, False, b"acgtacgtac", b"?" * 10)]


def test_accumulators_by_hand():
    a = rm.accumulate(READS)
    nh, h = a[0, 0], a[1, 0]
    assert [int(x) for x in nh[:8]] == [2, 15, 5, 10, 7, 1, 2, 15]
    assert [int(x) for x in h[:8]] == [1, 4, 4, 4, 4, 0, 1, 4]
    assert int(nh[8 + 40]) == 4 and int(nh[8 + 0]) == 1 and int(nh[8 + 30]) == 10 and int(nh[8:].sum()) == 15
    assert int(h[8 + 20]) == 4 and int(h[8:].sum()) == 4
    assert int(a[0, 1, rm.MIN_LEN]) == rm.NONE and int(a[0, 1, rm.READS]) == 0    # an empty accumulator: min_len all-ones
    twice = rm.accumulate(READS, a)
    assert int(twice[0, 0, rm.READS]) == 4 and int(twice[0, 0, rm.MIN_LEN]) == 5 and int(twice[0, 0, 8 + 30]) == 20


def test_table_by_hand():
    got = rm.table(rm.summary(READS, 1)).decode()
    want = (rm.HEADER +
            "input\t1\t3\t19\t4\t6.33\t5\t10\t10\t57.89\t1\t94.74\t73.68\t12.57\n"
            "nonhuman\t1\t2\t15\t5\t7.50\t5\t10\t10\t46.67\t1\t93.33\t93.33\t11.72\n"
            "human\t1\t1\t4\t4\t4.00\t4\t4\t4\t100.00\t0\t100.00\t0.00\t20.00\n")
    assert got == want


def test_empty_class():
    sm = rm.summary([(0, False, b"ACGT", b"IIII"), (0, False, b"", b"")], 1)
    assert int(sm["cls"][1, 0, rm.MIN_LEN]) == 0 and int(sm["cls"][0, 0, rm.MIN_LEN]) == 0 and int(sm["cls"][0, 0, rm.READS]) == 2
    lines = rm.table(sm).decode().splitlines()
    assert lines[3] == "human\t1\t0\t0\t0\tNA\t0\t0\t0\tNA\t0\tNA\tNA\tNA"
    assert lines[2] == "nonhuman\t1\t2\t4\t0\t2.00\t0\t4\t4\t50.00\t0\t100.00\t100.00\t40.00"
    assert lines[1].split("\t")[1:] == lines[2].split("\t")[1:]
    # no read at all, and only reads without bases
    assert rm.table(rm.summary([], 1)).decode().splitlines()[1] == "input\t1\t0\t0\t0\tNA\t0\t0\t0\tNA\t0\tNA\tNA\tNA"
    assert rm.table(rm.summary([(0, True, b"", b"")], 1)).decode().splitlines()[3] == "human\t1\t1\t0\t0\t0.00\t0\t0\t0\tNA\t0\tNA\tNA\tNA"


def test_fasta_mate():
    """mate 2 without qualities: its bases count, its quality columns are NA"""
    reads = [(0, True, b"ACGT", b"IIII"), (1, True, b"GGGGGG", None), (0, False, b"TT", b"++"), (1, False, b"NNNC", None)]
    sm = rm.summary(reads, 2)
    assert [int(x) for x in sm["cls"][1, 1, :8]] == [1, 6, 6, 6, 6, 0, 0, 0] and int(sm["cls"][1, 1, 8:].sum()) == 0
    assert [int(x) for x in sm["cls"][0, 1, :8]] == [1, 4, 4, 4, 1, 3, 0, 0]
    lines = rm.table(sm).decode().splitlines()
    assert len(lines) == 7 and [ln.split("\t")[:2] for ln in lines[1:]] == [[s, m] for s in rm.SETS for m in ("1", "2")]
    assert lines[2] == "input\t2\t2\t10\t4\t5.00\t4\t6\t6\t70.00\t3\tNA\tNA\tNA"
    assert lines[6] == "human\t2\t1\t6\t6\t6.00\t6\t6\t6\t100.00\t0\tNA\tNA\tNA"
    assert lines[3].endswith("\t0.00\t0.00\t10.00")  # ('+' is Phred 10)


def test_quality_bytes_outside_the_printable_range():
    """read as unsigned, less 33, clamped: 10 and 32 to bin 0, 127 and 255 to bin 93"""
    a = rm.accumulate([(0, False, b"ACGTACGT", bytes([32, 127, 10, 255, 33, 126, 34, 125]))])[0, 0]
    assert int(a[8 + 0]) == 3 and int(a[8 + 93]) == 3 and int(a[8 + 1]) == 1 and int(a[8 + 92]) == 1 and int(a[8:].sum()) == 8
    assert int(a[rm.QUAL_BASES]) == 8 and int(a[rm.GC]) == 4 and int(a[rm.OTHER]) == 0
    a = rm.accumulate([(0, False, b"acgtnRYx-*", None)])[0, 0]
    assert int(a[rm.GC]) == 2 and int(a[rm.OTHER]) == 6


def test_reads_of_text():
    text = b"@r\nACGT\n+\nII5!\n>f\nGGN\n"
    recs = [(3, 4, 10), (18, 3, rm.NONE)]
    reads = rm.reads_of_text(text, recs, [0, 7])
    assert reads == [(0, False, b"ACGT", b"II5!"), (0, True, b"GGN", None)]
    assert rm.reads_of_text(text, recs, [9], mates=2) == [(0, True, b"ACGT", b"II5!"), (1, True, b"GGN", None)]
    assert rm.reads_of_text(text, recs, [0, 7], bad={0}) == [(0, True, b"GGN", None)]


def _both_classes(toy, toy_oracle, records, q):
    calls = qm.classify(toy_oracle, records, q)[0]["call"]
    sm = rm.summary(rm.reads_of_records(records, calls), len(records))
    for m in range(len(records)):
        for c in range(2):
            assert int(sm["cls"][c, m, rm.READS]) >= 1, (q, c, m)
        # ... and the two classes differ in what they hold: a swapped index cannot pass
        assert not np.array_equal(sm["cls"][0, m], sm["cls"][1, m])
        assert int(sm["cls"][0, m, rm.READS]) != int(sm["cls"][1, m, rm.READS]) or int(sm["cls"][0, m, rm.BASES]) != int(sm["cls"][1, m, rm.BASES])
    return sm


def test_corpora_put_reads_in_both_classes(toy, toy_oracle):
    for paired in (False, True):
        _texts, records = qm.e2e_corpus(toy[3], paired)
        plain = _both_classes(toy, toy_oracle, records, 0)
        low = _both_classes(toy, toy_oracle, records, qm.Q_E2E)
        # the threshold moves reads between the classes; the input's bases stay
        assert int(plain["cls"][1, 0, rm.READS]) > int(low["cls"][1, 0, rm.READS])
        for w in (rm.READS, rm.BASES, rm.GC, rm.OTHER):
            assert int(plain["cls"][:, :, w].sum()) == int(low["cls"][:, :, w].sum())
    _texts, records = qm.ont_corpus(toy[3])
    sm = _both_classes(toy, toy_oracle, records, 0)
    assert int(sm["cls"][:, 0, rm.MAX_LEN].max()) == 20_000 and int(sm["cls"][:, 0, rm.MIN_LEN].min()) == 40
