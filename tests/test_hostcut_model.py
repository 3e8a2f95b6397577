"""tests/hostcut_model.py on its own cases: the pieces at the three places a run can lie, the identity of the counts, the record's
form, and the two capacities the builder reserves before it knows the calls -- P(L) pieces a sequence, the output's bytes -- on
coverages as the mark pass and the closing can leave them."""
import numpy as np
import pytest

from tests import builder_model as bmod
from tests import hitmask_model as hm
from tests import hostcut_model as hc
from tests import intervals_model as im

K = hc.K


def cov_of(n, covered):
    c = np.zeros(n, dtype=bool)
    for a, b in covered:
        c[a:b] = True
    return c


@pytest.mark.parametrize("m", [1, 2, 35, 40, 200])
@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_runs_of_m_minus_1_m_and_m_plus_1(m, where):
    for ln in (m - 1, m, m + 1):
        if where == "start":
            n, cov, want = ln + 40, [(ln, ln + 40)], (0, ln)
        elif where == "end":
            n, cov, want = 40 + ln, [(0, 40)], (40, 40 + ln)
        else:
            n, cov, want = 40 + ln + 50, [(0, 40), (40 + ln, 90 + ln)], (40, 40 + ln)
        c = cov_of(n, cov)
        got = hc.pieces(c, m)
        assert got == ([want] if ln >= m and ln > 0 else []), (ln, got)
        t = hc.tally(c, m)
        assert t == (n, int(ln >= m and ln > 0), ln if ln >= m else 0, n - ln, 0 if ln >= m else ln, int(not (ln >= m and ln > 0)))


def test_no_covered_base_is_one_piece_and_all_covered_is_dropped():
    assert hc.pieces(np.zeros(77, dtype=bool), 35) == [(0, 77)]
    assert hc.tally(np.zeros(77, dtype=bool), 35) == (77, 1, 77, 0, 0, 0)
    assert hc.pieces(np.ones(77, dtype=bool), 1) == [] and hc.tally(np.ones(77, dtype=bool), 1) == (77, 0, 0, 77, 0, 1)
    assert hc.pieces(np.zeros(0, dtype=bool), 1) == [] and hc.tally(np.zeros(0, dtype=bool), 1) == (0, 0, 0, 0, 0, 1)
    assert hc.pieces(np.zeros(34, dtype=bool), 35) == [] and hc.tally(np.zeros(34, dtype=bool), 35) == (34, 0, 0, 0, 34, 1)


def test_the_count_identity_on_random_coverages():
    rng = np.random.default_rng(1)
    for _ in range(300):
        n = int(rng.integers(0, 400))
        closed, _added = hm.close(hc.kmer_union(rng, n, rng.random() * 0.1), int(rng.integers(0, 60)))
        for m in (1, 20, 35, 36, 100):
            hb, np_, pb, cb, sb, dr = hc.tally(closed, m)
            assert hb == n == pb + cb + sb and dr == (np_ == 0)
            assert np_ == len(hc.pieces(closed, m)) and pb == sum(b - a for a, b in hc.pieces(closed, m))


@pytest.mark.parametrize("fastq", [True, False])
def test_the_record_of_a_piece(fastq):
    s, q = b"ACGTacgtNNACGTACGTAC", b"IIIIJJJJ##KKKKLLLLMM"
    for h, head, rest in ((b"r1", b"r1", b""), (b"r1 a comment", b"r1", b" a comment"), (b"r1\ttab\tcomment", b"r1", b"\ttab\tcomment"),
                          (b"r/1 x", b"r/1", b" x")):
        raw = b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" if fastq else b">" + h + b"\n" + s + b"\n"
        r = bmod.parse_record(raw, fastq)
        mark = raw[:1]
        want = mark + head + b":4-10" + rest + b"\n" + s[4:10] + (b"\n+\n" + q[4:10] if fastq else b"") + b"\n"
        assert hc.piece_record(r, 4, 10) == want
    # CRLF and "+id": the fields, not the lines
    r = bmod.parse_record(b"@id c\r\n" + s + b"\r\n+id c\r\n" + q + b"\r\n", True)
    assert hc.piece_record(r, 0, 20) == b"@id:0-20 c\n" + s + b"\n+\n" + q + b"\n"


def test_text_of_writes_the_other_fragments_whole_and_in_order():
    recs = [bmod.parse_record(b"@a%d x\n" % i + b"ACGT" * 25 + b"\n+\n" + b"I" * 100 + b"\n", True) for i in range(4)]
    closed = [None, cov_of(100, [(10, 50)]), None, np.ones(100, dtype=bool)]
    text, six, cuts = hc.text_of(recs, [False, True, False, True], closed, 35)
    assert text == recs[0].raw + hc.piece_record(recs[1], 50, 100) + recs[2].raw
    assert six == (200, 1, 50, 140, 10, 1) and cuts == [None, [(50, 100)], None, []]


def closed_coverages(rng, count):
    for _ in range(count):
        n = int(rng.integers(0, 700))
        yield hm.close(hc.kmer_union(rng, n, rng.random() ** 3 * 0.3), int(rng.choice([0, 0, 10, 34, 100])))[0]


def test_the_bound_on_the_pieces_holds_and_is_attained():
    rng = np.random.default_rng(2)
    attained = set()
    for closed in closed_coverages(rng, 2000):
        for m in (1, 35, 40, 200):
            p = len(hc.pieces(closed, m))
            assert p <= hc.max_pieces(len(closed), m), (len(closed), m, p)
    # attained: pieces of exactly m with covered runs of exactly k between them
    for m in (1, 35, 40):
        for pcs in (1, 2, 5):
            n = pcs * m + (pcs - 1) * K
            c = np.zeros(n, dtype=bool)
            for j in range(pcs - 1):
                c[(j + 1) * m + j * K:(j + 1) * (m + K)] = True
            assert len(hc.pieces(c, m)) == pcs == hc.max_pieces(n, m)
            attained.add((m, pcs))
    assert len(attained) == 9
    assert hc.max_pieces(34, 35) == 0 and hc.max_pieces(35, 35) == 1 and hc.max_pieces(104, 35) == 1 and hc.max_pieces(105, 35) == 2


def test_the_output_capacity_holds():
    rng = np.random.default_rng(3)
    for fastq in (True, False):
        recs, closed = [], []
        for i, c in enumerate(closed_coverages(rng, 300)):
            n = len(c)
            s = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())
            h = b"read%d" % (10 ** int(rng.integers(0, 9))) + (b" c" if i % 2 else b"")
            raw = b"@" + h + b"\n" + s + b"\n+\n" + b"I" * n + b"\n" if fastq else b">" + h + b"\n" + s + b"\n"
            recs.append(bmod.parse_record(raw, fastq))
            closed.append(c)
        mask_cap = sum(len(r.raw) for r in recs) + len(recs) + 64  # (the mask builder's: the text, a newline a record, 64)
        for m in (1, 35, 200):
            for host in ([True] * len(recs), [i % 3 != 0 for i in range(len(recs))]):
                text, _six, cuts = hc.text_of(recs, host, closed, m)
                assert len(text) <= hc.output_cap(recs, m, mask_cap)
                items = sum(1 if c is None else len(c) for c in cuts)
                assert items <= len(recs) + sum(hc.max_pieces(r.slen, m) for r in recs)


def test_runs_are_the_interval_models():
    c = cov_of(50, [(0, 3), (10, 20), (49, 50)])
    assert im.runs(~c) == [(3, 10), (20, 49)] and hc.pieces(c, 8) == [(20, 49)] and hc.pieces(c, 7) == [(3, 10), (20, 49)]
