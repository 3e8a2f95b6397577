"""The Python model of runs with --dust-reads (tests/rdust_model.py): the masking rule on records by hand, the database that
holds low-complexity minimizers, and what the corpora of tests/test_gpu_read_dust_run.py contain -- a GPU run that equals the
model then cannot pass without the mask having changed a call, a count and a hit list.  No GPU needed."""
import numpy as np
import pytest

from tests import builder_model as bm
from tests import dust_model as dm
from tests import rdust_model as rd


@pytest.fixture(scope="module")
def lc_oracle():
    from oracle import oracle as orc
    ob, tb, hb = rd.lc_db()[:3]
    return orc.OracleDB(ob, tb, hb)


def test_rule_on_records_by_hand():
    fq = bm.parse_record(b"@r1\n" + b"ACGTTGCA" + b"A" * 9 + b"GATC\n+\n" + b"I" * 8 + b"!" * 2 + b"I" * 11 + b"\n", True)
    fa = bm.parse_record(b">r1\nACGTTGCAAAAA\nAAAAAGATC\n", False)
    want = b"ACGTTGC" + b"N" * 10 + b"GATC"  # (the A in front of the nine belongs to the homopolymer)
    assert rd.masked_seq(fq) == want and rd.masked_seq(fa) == want  # FASTA as FASTQ, the lines of a FASTA sequence joined
    assert rd.masked_seq(fq, dust=False) == fq.seq
    # with a minimum base quality: the union; DUST saw the original bases (two N in the stretch would have ended it otherwise)
    assert rd.masked_seq(fq, q=20) == want
    low = bm.parse_record(b"@r2\n" + b"ACGTTGCA" + b"A" * 9 + b"GATC\n+\n" + b"!!" + b"I" * 9 + b"!" + b"I" * 9 + b"\n", True)
    assert rd.masked_seq(low, q=20) == b"NNGTTGC" + b"N" * 10 + b"GATC"
    assert rd.masked_seq(low, q=20, dust=False) == b"NNGTTGCAAAANAAAAAGATC"
    assert rd.masked_fragments([[fq], [fa]]) == [(want, want)]
    assert rd.dust_masked_bases([[fq], [fa]]) == 20
    # each sequence on its own: two records that end and begin with A x 6
    a, b = bm.parse_record(b">a\nCGTCG" + b"A" * 6 + b"\n", False), bm.parse_record(b">b\n" + b"A" * 6 + b"GCTGA\n", False)
    assert rd.masked_seq(a) == a.seq and rd.masked_seq(b) == b.seq and b"N" in dm.mask(a.seq + b.seq)


def test_database_holds_low_complexity_minimizers(lc_oracle):
    """the satellite alone, with no flank of the genome, is called host by the unmasked table; masked, it has no k-mer left"""
    genomes, own = rd.lc_db()[3], rd.lc_db()[5]
    assert rd.SATELLITE in genomes[rd.HUMAN] and b"A" * 40 in own
    assert dm.mask(own)[100:280] == b"N" * 180 and dm.mask(own)[400:440] == b"N" * 40
    rng = np.random.default_rng(1)
    read = bm.parse_record(b"@sat\n" + rd.satellite_read(rng) + b"\n+\n" + b"I" * 210 + b"\n", True)
    plain, _, _ = rd.classify(lc_oracle, [[read]], dust=False)
    masked, _, _ = rd.classify(lc_oracle, [[read]])
    assert plain["call"][0] != 0 and plain["hit_groups"][0] >= 2
    assert masked["call"][0] == 0 and masked["clade_hits"][0] == 0 and masked["total_kmers"][0] == plain["total_kmers"][0]


def _a_runs(line):
    return [x for x in line.split(b"\t")[4].split(b" ") if x.startswith(b"A:")]


def _properties(lc_oracle, paired, fasta=False):
    texts, records = rd.e2e_corpus(paired, fasta=fasta)
    plain = rd.expected(lc_oracle, records, dust=False)
    dust = rd.expected(lc_oracle, records)
    r0, r1 = plain["res"], dust["res"]
    n = len(r0)
    flips = [f for f in range(n) if r0["call"][f] != 0 and r1["call"][f] == 0]
    fewer = [f for f in range(n) if r0["call"][f] != 0 and r1["call"][f] != 0 and r1["clade_hits"][f] < r0["clade_hits"][f]]
    k0, k1 = plain["k"].splitlines(), dust["k"].splitlines()
    new_a = [f for f in range(n) if len(_a_runs(k1[f])) > len(_a_runs(k0[f]))]
    assert len(flips) >= 30 and len(fewer) >= 10 and len(new_a) >= 60, (len(flips), len(fewer), len(new_a))
    # the microbial-like reads that carry the satellite: host without the flag, kept with it -- every one of them
    sat = [f for f in range(n) if f % 5 == 1]
    assert all(r0["call"][f] != 0 and r1["call"][f] == 0 for f in sat)
    assert all(r0["call"][f] != 0 and r1["call"][f] == r0["call"][f] for f in range(n) if f % 5 == 0 and b"N" not in rd.masked_seq(records[0][f]))
    assert not any(r1["call"][f] != 0 and r0["call"][f] == 0 for f in range(n))  # masking never adds a call
    # only classification changes: the k-mer totals, the lengths and the bases stay
    assert np.array_equal(r0["total_kmers"], r1["total_kmers"])
    assert [ln.split(b"\t")[3] for ln in k0] == [ln.split(b"\t")[3] for ln in k1]
    assert plain["stats"][3] == dust["stats"][3] and plain["stats"][1] > dust["stats"][1] > 30
    assert dust["masked_bases"] > 5000 and plain["masked_bases"] == 0
    assert plain["report"] != dust["report"] and plain["calls"] != dust["calls"] and plain["ids"] != dust["ids"]
    # the records written keep their bases: a kept record is byte for byte its input text
    kept = b"".join(r.text[:r.hlen] + b"\n" + r.seq + b"\n" for r, c in zip(records[0], r1["call"]) if c == 0) if fasta else \
        b"".join(r.raw for r, c in zip(records[0], r1["call"]) if c == 0)
    assert dust["normal"][0] == kept and rd.SATELLITE[20:120] in kept
    if not fasta:
        # with a minimum base quality as well: the union changes more than either mask alone
        both = rd.expected(lc_oracle, records, q=rd.Q_E2E)
        lowq = rd.expected(lc_oracle, records, q=rd.Q_E2E, dust=False)
        assert both["k"] != dust["k"] and both["k"] != lowq["k"]
        assert all(both["res"]["call"][f] == 0 for f in sat) and any(lowq["res"]["call"][f] != 0 for f in sat)
    if paired:
        assert any(r.slen == 0 for r in records[1]) and any(b"N" in rd.masked_seq(r) for r in records[1])
    assert sum(len(t) for t in texts) < 250_000


def test_e2e_corpus_single_end(lc_oracle):
    _properties(lc_oracle, False)


def test_e2e_corpus_paired(lc_oracle):
    _properties(lc_oracle, True)


def test_e2e_corpus_fasta(lc_oracle):
    _properties(lc_oracle, False, fasta=True)
    _texts, records = rd.e2e_corpus(False, fasta=True)
    assert any(r.raw.count(b"\n") > 2 for r in records[0]) and not any(r.fastq for r in records[0])


def test_ont_corpus(lc_oracle):
    """reads long enough to be cut by the classifier and to span many of the kernel's tiles, with stretches across tile
    borders; masking changes their hit lists"""
    texts, records = rd.ont_corpus()
    long_reads = [r for r in records[0] if r.slen - 34 > 48 * 124]
    assert len(long_reads) == 3
    # a masked stretch lies across a multiple of 900 virtual positions (the reads in order, one separator behind each)
    voff, across = 0, 0
    for r in records[0]:
        m = dm.mask_bool(bytes(r.seq))
        for b in range(900 - voff % 900, r.slen - 1, 900):
            across += int(m[b - 1] and m[b])
        voff += r.slen + 1
    assert across >= 3
    plain, dust = rd.expected(lc_oracle, records, dust=False), rd.expected(lc_oracle, records)
    assert plain["k"] != dust["k"] and (dust["res"]["call"] != 0).sum() >= 3
    assert any(int(a[2:]) >= 100 for ln in dust["k"].splitlines() for a in _a_runs(ln))
    assert dust["masked_bases"] > 3000
