"""The model of the read lists (tests/calls_model.py) against hand-written -k lines, the bound the host puts on a batch's
buffers, and the corpora of tests/test_gpu_calls.py: that they hold every case those tests rely on is asserted here, with the
CPU oracle's results.  No GPU needed."""
import numpy as np
import pytest

from tests import calls_model as cm
from tests.builder_model import parse_record

EXT = [0, 1, 10, 9606, 1234567]  # internal -> external taxon ids of the hand-written cases


def _rec(raw, fastq=True):
    return parse_record(raw, fastq)


# (mate 1's record, mate 2's or None, result, the -k line as nh_run writes it for the fragment, the ids line or None)
HAND = [
    (b"@r1\nACGTACGTAC\n+\nIIIIIIIIII\n", None, (0, 0, 0, 0), b"U\tr1\t0\t10\t0:0\n", None),
    (b"@r2 comment here\nACGT\n+\nIIII\n", None, (3, 7, 5, 2), b"C\tr2\t9606\t4\t9606:5 0:2\n", b"r2\n"),
    (b"@r3/1\nACGT\n+\nIIII\n", None, (2, 1, 1, 1), b"C\tr3/1\t10\t4\t10:1\n", b"r3/1\n"),  # single-end: nothing trimmed
    (b"@r3/1\nACGT\n+\nIIII\n", b"@r3/2\nACGTA\n+\nIIIII\n", (2, 1, 1, 1), b"C\tr3\t10\t4|5\t10:1 |:| 0:1\n", b"r3\n"),
    (b"@r4/3\nAC\n+\nII\n", b"@r4/3\n\n+\n\n", (0, 0, 0, 0), b"U\tr4/3\t0\t2|0\t|:|\n", None),
    (b"@/1\nAC\n+\nII\n", b"@/2\nAC\n+\nII\n", (4, 3, 2, 2), b"C\t/1\t1234567\t2|2\t|:|\n", b"/1\n"),  # two bytes: kept
    (b"@x/2\nAC\n+\nII\n", b"@x/2\nAC\n+\nII\n", (1, 3, 2, 2), b"C\tx\t1\t2|2\t|:|\n", b"x\n"),
    (b"@t\tdesc\r\nACG\r\n+\r\nIII\r\n", None, (0, 4294967295, 0, 0), b"U\tt\t0\t3\t0:0\n", None),
    (b"@c/1 desc/2\nACG\n+\nIII\n", b"@c/2\nACG\n+\nIII\n", (1, 2, 2, 2), b"C\tc\t1\t3|3\t1:2\n", b"c\n"),
    (b">fa1 desc\nACGTT\n", None, (1, 2, 2, 2), b"C\tfa1\t1\t5\t1:2\n", b"fa1\n"),
]


def test_columns_1_to_4_are_the_k_lines():
    for raw1, raw2, res, kline, idline in HAND:
        fastq = raw1[:1] == b"@"
        records = [[_rec(raw1, fastq)]] + ([[_rec(raw2)]] if raw2 else [])
        table, ids = cm.expected(records, [res], EXT)
        cols = table.split(b"\t")
        assert b"\t".join(cols[:4]) == b"\t".join(kline.split(b"\t")[:4]), (raw1, table)
        assert table.endswith(b"\n") and table.count(b"\n") == 1 and len(cols) == 7
        assert [int(x) for x in cols[4:]] == list(res[1:]), table
        assert ids == (idline or b""), (raw1, ids)


def test_tables_are_concatenated_in_input_order():
    records = [[_rec(h[0], h[0][:1] == b"@") for h in HAND if h[1] is None and h[0][:1] == b"@"]]
    results = [h[2] for h in HAND if h[1] is None and h[0][:1] == b"@"]
    table, ids = cm.expected(records, results, EXT)
    assert table == b"".join(cm.expected([[r]], [x], EXT)[0] for r, x in zip(records[0], results))
    assert ids == b"r2\nr3/1\n"
    assert cm.expected([[]], [], EXT) == (b"", b"")


def test_the_buffer_bound_holds_for_the_widest_line():
    """the host reserves sum(id lengths) + 79 a fragment (+ 64) for the table and sum + 1 a fragment for the ids: the widest
    numbers a line can carry fill the 79 exactly, and trimming only shortens a line"""
    big = 2 ** 64 - 1
    recs = [[_rec(b"@" + b"i" * 7 + b"\n" + b"A" * 3 + b"\n+\nIII\n")], [_rec(b"@m2\nA\n+\nI\n")]]
    recs[0][0].slen = recs[1][0].slen = 2 ** 32 - 1  # (the widest lengths: only the model's numbers matter here)
    table, ids = cm.expected(recs, [(1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)], [0, big])
    assert len(table) == 7 + cm.TAIL_MAX == 7 + 79
    assert len(ids) == 7 + 1
    cap = cm.buffer_caps(recs)
    assert cap[0] >= len(table) and cap[1] >= len(ids)
    for raw1, raw2, res, _k, _i in HAND:  # and every hand-written case lies within its bound
        fastq = raw1[:1] == b"@"
        records = [[_rec(raw1, fastq)]] + ([[_rec(raw2)]] if raw2 else [])
        table, ids = cm.expected(records, [res], EXT)
        cap = cm.buffer_caps(records)
        assert len(table) <= cap[0] - 64 and len(ids) <= cap[1] - 64


def _oracle_results(db, records):
    from oracle import oracle as orc
    paired = len(records) == 2
    bases, offs = orc.pack_reads(cm.fragments(records), paired)
    out, _ = db.classify(bases, offs, paired, 0.0)
    return out


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("fasta", [False, True])
def test_edge_corpus_holds_every_case(toy, toy_oracle, paired, fasta):
    _texts, records = cm.edge_corpus(toy[3], paired, fasta)
    res = _oracle_results(toy_oracle, records)
    cls = res["call"] != 0
    assert cls.sum() >= 10 and (~cls).sum() >= 10
    heads = [r.header for r in records[0]]
    raw = [cm.raw_id(h) for h in heads]
    ids = [cm.record_id(h, paired) for h in heads]
    for n in (1, 2, 3, 4, 5, 300):  # ... each among the classified fragments (the ids file) and among the others
        assert any(len(i) == n and c for i, c in zip(raw, cls)), n
        assert any(len(i) == n and not c for i, c in zip(raw, cls)), n
    for end in (b"/1", b"/2", b"/3"):
        assert any(i.endswith(end) and len(i) > 2 and c for i, c in zip(raw, cls)), end
    assert b"/1" in raw and b"/1" in ids  # the two-byte id is never trimmed
    assert (b"x" in ids and b"x/1" not in ids) == paired and (b"z/3" in ids)
    assert any(b"\t" in h for h in heads) and any(b" " in h for h in heads)
    assert any(b"/1" in h.split(b" ", 1)[-1] for h in heads if b" " in h)  # "/1" behind the id is no pair suffix
    lens = [r.slen for r in records[0]]
    for n in cm.EDGE_LENGTHS:
        assert n in lens
    if not fasta:
        assert 0 in lens
        assert any(r.raw.endswith(b"\r\n") for r in records[0])
    assert len({int(toy_oracle.external_ids[c]) for c in res["call"] if c}) >= 1
    table, idl = cm.expected(records, res, toy_oracle.external_ids)
    for text in (table, idl):  # lines start at every byte residue of a dword
        assert {p & 3 for p in cm.line_starts(text)} == {0, 1, 2, 3}
    # the digits: lengths of 1 to 4 digits, k-mer counts of 1 to 3
    assert {len(b"%d" % n) for n in lens} >= {1, 2, 3, 4}
    assert {len(b"%d" % int(t)) for t in res["total_kmers"]} >= {1, 2, 3}


def test_the_toy_taxonomy_has_no_id_above_four_digits(toy_oracle):
    """... so the GPU test of wider taxon ids patches the taxonomy image (tests/builder_model.py DIGIT_IDS)"""
    assert max(int(x) for x in toy_oracle.external_ids) == 9606


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025, 2049])
def test_read_corpora_hold_both_kinds(toy, toy_oracle, n, paired):
    _texts, records = cm.reads_corpus(toy[3], n, paired)
    assert len(records[0]) == n
    cls = _oracle_results(toy_oracle, records)["call"] != 0
    assert cls.sum() >= 10 and (~cls).sum() >= 10


def test_carry_corpus_passes_256_blocks(toy, toy_oracle):
    _text, records, unit, reps = cm.carry_corpus(toy[3])
    n = len(records[0])
    assert n == len(unit) * reps and n <= cm.CARRY_BATCH_FRAGS  # one batch
    assert (n + cm.BLOCK - 1) // cm.BLOCK > 256  # ... whose block sums need a second round of the scan
    cls = _oracle_results(toy_oracle, [unit])["call"] != 0
    assert cls.sum() >= 10 and (~cls).sum() >= 10
    assert max(r.slen for r in unit) <= 68
