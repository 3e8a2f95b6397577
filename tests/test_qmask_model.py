"""The Python model of runs with a minimum base quality (tests/qmask_model.py): the masking rule by hand, and what the
corpora of tests/test_gpu_minq_run.py contain -- a GPU run that equals the model then cannot pass without the masking having
changed a call, a count and a hit list.  No GPU needed."""
import numpy as np

from tests import builder_model as bm
from tests import qmask_model as qm


def test_rule_by_hand():
    q = 20
    seq = b"ACGTACGTAC"
    #        score: 20 (kept), 19 (masked), 0, 93, 40, 21, 19, 20, 2, 30
    qual = bytes(33 + s for s in (20, 19, 0, 93, 40, 21, 19, 20, 2, 30))
    assert qm.mask_seq(seq, qual, q) == b"ANNTACNTNC"
    assert qm.mask_seq(seq, qual, 0) == seq
    assert qm.mask_seq(seq, qual, 1) == b"ACNTACGTAC"          # only the score 0 is below 1
    assert qm.mask_seq(seq, qual, 93) == b"NNNTNNNNNN"         # only '~' survives 93
    assert qm.mask_seq(b"", b"", 20) == b""
    assert qm.mask_seq(seq, bytes([32, 10, 200, 255, 33, 52, 53, 126, 127, 128]), q) == b"NNGTNNGTAC"  # bytes read as unsigned


def test_fasta_records_are_never_masked():
    fa = bm.parse_record(b">r1\nACGTACGT\n", False)
    fq = bm.parse_record(b"@r1\nACGTACGT\n+\n!!!!IIII\n", True)
    assert qm.masked_fragments([[fa]], 40) == [b"ACGTACGT"]
    assert qm.masked_fragments([[fq]], 40) == [b"NNNNACGT"]
    assert qm.masked_fragments([[fq], [fa]], 40) == [(b"NNNNACGT", b"ACGTACGT")]
    assert qm.masked_bases([[fq], [fa]], 40) == 4 and qm.masked_bases([[fq]], 0) == 0


def test_hitlist_and_k_lines():
    ext = [0, 1, 9606]
    assert qm.hitlist(np.array([], dtype=np.uint32), ext) == b"0:0"
    t = np.array([2, 2, qm.AMBIG, qm.AMBIG, qm.AMBIG, 0, qm.BORDER, 1], dtype=np.uint32)
    assert qm.hitlist(t, ext) == b"9606:2 A:3 0:1 |:| 1:1"


def _a_runs(line):
    return [x for x in line.split(b"\t")[4].split(b" ") if x.startswith(b"A:")]


def _properties(toy, toy_oracle, paired):
    texts, records = qm.e2e_corpus(toy[3], paired)
    plain = qm.expected(toy_oracle, records, 0)
    low = qm.expected(toy_oracle, records, qm.Q_E2E)
    r0, r1 = plain["res"], low["res"]
    flips = [f for f in range(len(r0)) if r0["call"][f] != 0 and r1["call"][f] == 0]
    fewer = [f for f in range(len(r0)) if r0["call"][f] != 0 and r1["call"][f] != 0 and r1["clade_hits"][f] < r0["clade_hits"][f]]
    k0, k1 = plain["k"].splitlines(), low["k"].splitlines()
    new_a = [f for f in range(len(r0)) if len(_a_runs(k1[f])) > len(_a_runs(k0[f]))]
    assert len(flips) >= 10 and len(fewer) >= 10 and len(new_a) >= 10, (len(flips), len(fewer), len(new_a))
    # only classification changes: the k-mer totals, the lengths and the bases stay
    assert np.array_equal(r0["total_kmers"], r1["total_kmers"])
    assert [ln.split(b"\t")[3] for ln in k0] == [ln.split(b"\t")[3] for ln in k1]
    assert plain["stats"][3] == low["stats"][3] and plain["stats"][1] > low["stats"][1] > 10
    assert low["masked_bases"] > 1000
    # the records written keep their bases: a kept record is byte for byte its input
    kept = b"".join(r.raw for r, c in zip(records[0], r1["call"]) if c == 0)
    assert low["normal"][0] == kept and b"N" * 20 not in kept
    # the corpus has qualities exactly at the threshold and one below it
    assert any(r.qual[0] == 33 + qm.Q_E2E and r.qual[1] == 32 + qm.Q_E2E for r in records[0])
    assert sum(len(t) for t in texts) < 200_000


def test_e2e_corpus_single_end(toy, toy_oracle):
    _properties(toy, toy_oracle, False)


def test_e2e_corpus_paired(toy, toy_oracle):
    _properties(toy, toy_oracle, True)


def test_ont_corpus(toy, toy_oracle):
    """reads long enough to be cut (more than 48 * 124 k-mers) with a low-quality stretch across the cuts at 3968 and 7936
    k-mers; masking changes their hit lists"""
    texts, records = qm.ont_corpus(toy[3])
    long_reads = [r for r in records[0] if r.slen - 34 > 48 * 124]
    assert len(long_reads) == 3
    for r in long_reads:
        for cut in (qm.SEG_KMERS, 2 * qm.SEG_KMERS):
            assert all(b - 33 < qm.Q_E2E for b in r.qual[cut - 100:cut + 100])
    plain, low = qm.expected(toy_oracle, records, 0), qm.expected(toy_oracle, records, qm.Q_E2E)
    assert plain["k"] != low["k"] and (low["res"]["call"] != 0).sum() >= 3
    assert any(int(a[2:]) >= 300 for ln in low["k"].splitlines() for a in _a_runs(ln))
