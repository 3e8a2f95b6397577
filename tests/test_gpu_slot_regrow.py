"""A slot's feature buffers regrow after they have been used (nh_run.hip: Slot, BuiltOut and their reserve): the same input run
twice on two slots a device (NOHUMAN_SLOTS=2), once in many batches whose needs jump -- so that every buffer a feature keeps in
a slot is given back and allocated again in the middle of the run, in both slots -- and once with the default limits, in one
batch (the text-cut input: in a few large ones).  Every file the two runs write must be the same bytes, the stats and the
features' counts the same numbers.  No model is needed: the one-batch run is the reference, and it is checked by the other
tests.  This pins behaviour that the owning buffer types of the slots had to keep: the test passes at the commit before them too.

The rule (grow() and Buf::reserve): a buffer that held `a` elements was allocated with a + a / 4 + 4096; it is freed and
allocated again when a later batch needs more than that.

Count-cut, paired, NOHUMAN_BATCH_FRAGS=64: 256 pairs of 50-base reads (4 batches, 2 a slot), then 256 pairs of 4 000-base reads
(4 batches).  A record is 2 L + 12 bytes at most, so a mate's text is <= 64 * 112 = 7 168 bytes in a short batch and >= 64 * 8 008
= 512 512 in a long one.  The text-sized buffers of both mates together: the text and the quality / DUST text held <= 14 400 + 320
bytes and were allocated with <= 22 576, the long batches need > 1 025 024; the cover bitmap (a bit a byte: words = bytes / 32)
held <= 461 words, allocated <= 4 673, needs > 32 032; a builder's output of a mate (the text + 36 bytes a fragment + 64) held
<= 9 536 bytes, allocated <= 16 016, needs > 512 512; the k-mer taxa (a word a k-mer and one a pair) held 64 * 33 + 1 words,
allocated 6 737, need 64 * 7 933 + 1.  The arrays that hold an entry a fragment do not regrow here (64 <= 4 096 + ...).

Text-cut, single-end, NOHUMAN_BATCH_TEXT=524288: 32 reads of 30 kb (a record is 60 kb: 8 records a batch, 4 batches), then
20 000 reads of 40 .. 60 bases (a record is <= 6 + 2 * 60 + 5 = 131 bytes and 110 on average: more than 4 400 a batch, the test
asserts that of its input; 4 to 5 batches).  What holds an entry a fragment or a sequence held 8, was allocated for 8 + 2 + 4 096
= 4 106 of them (the scratch arrays, a few words more than a word a sequence, for a few more) and needs > 4 400: the starts, lengths, results and k-mer taxa offsets, the
record table, the id lengths, the host-filtered results, the cover passes' scratch (a word a sequence and more) and the
DUST scan's scratch.  The text-sized buffers do not regrow in this order; the count-cut shape is for them.

Requests: A, a split run through every extra (calls, human ids, --minimum-base-quality, --dust-reads, read statistics, a host
selection, host intervals, kraken output, two per-taxon selectors); B, a masked run with --host-bases-only and host intervals;
C, a paired BAM in and BAM out, a split run, count-cut only (a BAM file's BGZF members end where the batches' spans do, so the
two BAM outputs are compared as the streams they inflate to; every other file of C as the bytes it is)."""
import gzip
import os

import numpy as np
import pytest

from tests import bam_model as bm
from tests import bam_pair_model as bp
from tests import synth
from tests.test_gpu_mask import _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BATCH_FRAGS, BATCH_TEXT = 64, 524288
COUNT_CUT = {"NOHUMAN_BATCH_FRAGS": str(BATCH_FRAGS)}
TEXT_CUT = {"NOHUMAN_BATCH_TEXT": str(BATCH_TEXT)}
Q = 12
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    from nohuman_amd import Engine
    with Engine.open(DB) as e:
        yield e


def read_of(rng, genomes, n, i):
    """n bases: stretches of the toy genomes and random stretches in turn, so that long reads are classified as short ones are;
    every fourth read (by i) is random bases alone"""
    if i % 4 == 3:
        return synth.random_seq(rng, n)
    keys = sorted(genomes)
    parts, have = [], 0
    while have < n:
        g = genomes[keys[int(rng.integers(0, len(keys)))]]
        ln = int(rng.integers(40, 300))
        at = int(rng.integers(0, len(g) - ln))
        parts += [g[at:at + ln], synth.random_seq(rng, int(rng.integers(0, 60)))]
        have += len(parts[-2]) + len(parts[-1])
    return b"".join(parts)[:n]


def quals(rng, n):
    """mostly good, a tenth below the threshold: the quality mask has something to do"""
    q = rng.integers(Q, 41, n, dtype=np.uint8)
    q[rng.random(n) < 0.1] = 3
    return q


def fastq(name, seq, q):
    return b"@" + name + b"\n" + seq + b"\n+\n" + (q + 33).tobytes() + b"\n"


def count_cut_reads():
    """[(name, seq1, qual1, seq2, qual2)]: 256 pairs of 50 bases, then 256 pairs of 4 000; every fifth mate with a poly-A stretch"""
    if "pairs" not in _CACHE:
        rng = np.random.default_rng(41)
        genomes = synth.toy_db()[3]
        out = []
        for i in range(8 * BATCH_FRAGS):
            ln = 50 if i < 4 * BATCH_FRAGS else 4000
            s1, s2 = read_of(rng, genomes, ln, i), read_of(rng, genomes, ln, i)
            if i % 5 == 0:
                s1 = s1[:10] + b"A" * 30 + s1[40:]
            out.append((b"p%d" % i, s1, quals(rng, ln), s2, quals(rng, ln)))
        _CACHE["pairs"] = out
    return _CACHE["pairs"]


def count_cut_fastq(tmp):
    reads = count_cut_reads()
    p1, p2 = tmp / "cc_1.fq", tmp / "cc_2.fq"
    p1.write_bytes(b"".join(fastq(n + b"/1", s1, q1) for n, s1, q1, _s2, _q2 in reads))
    p2.write_bytes(b"".join(fastq(n + b"/2", s2, q2) for n, _s1, _q1, s2, q2 in reads))
    return str(p1), str(p2)


def text_cut_fastq(tmp):
    if "single" not in _CACHE:
        rng = np.random.default_rng(42)
        genomes = synth.toy_db()[3]
        recs = []
        for i in range(32 + 20000):
            ln = 30000 if i < 32 else int(rng.integers(40, 61))
            s = read_of(rng, genomes, ln, i)
            if i % 5 == 0:
                s = s[:5] + b"A" * 30 + s[35:]
            recs.append(fastq(b"%x" % i, s, quals(rng, ln)))
        # the batches of the short reads: more than 4 400 records in any BATCH_TEXT bytes of them
        sizes = np.cumsum([len(r) for r in recs[32:]])
        fewest = min(int(np.searchsorted(sizes, sizes[k] + BATCH_TEXT) - k) for k in range(0, len(sizes) - 5000, 500))
        assert fewest > 4400 and all(len(r) > 60000 for r in recs[:32]), fewest
        _CACHE["single"] = b"".join(recs)
    p = tmp / "tc.fq"
    p.write_bytes(_CACHE["single"])
    return str(p), None


def paired_bam(tmp):
    reads = count_cut_reads()
    recs = []
    for i, (n, s1, q1, s2, q2) in enumerate(reads):
        recs += bp.forge_pair(n, s1, s2, q1.tobytes(), q2.tobytes(), rev=(i & 1, (i >> 1) & 1), mate2_first=i % 3 == 2,
                              tags=(b"RGZgroup1\0", b"NMC\x03"))
    p = tmp / "cc.bam"
    p.write_bytes(bm.bgzf(bm.forge_header(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@RG\tID:group1\n") + b"".join(recs), 60000))
    return str(p), None


def one_run(tmp, tag, eng, ins, env, request, inflate=()):
    """-> ({file: bytes}, the numbers of the run)"""
    from nohuman_amd.engine import ReadStats
    d = tmp / tag
    d.mkdir()
    p = lambda x: str(d / x)
    in1, in2 = ins
    paired = in2 is not None
    kw = dict(kraken_output=p("k"), report=p("r"), threads=4)
    if request == "A":
        rs = ReadStats(p("rs"))
        kw.update(human_out1=p("h1"), calls=p("calls"), human_ids=p("ids"), min_base_quality=Q, dust_reads=True, read_stats=rs,
                  host_taxids=[10, 9606], keep_taxids=[111], host_intervals=p("bed"),
                  taxon_outs=[(10, p("t10_1"), p("t10_2") if paired else None), ("other", p("to_1"), p("to_2") if paired else None)])
    elif request == "B":
        kw.update(mask=True, host_bases_only=True, host_gap=34, host_intervals=p("bed"))
    else:
        kw.update(human_out1=p("h1"), out_codec=6, calls=p("calls"))
    if paired:
        kw.update(in2=in2, out2=p("o2"))
        if request == "A":
            kw.update(human_out2=p("h2"))
    new = dict(env, NOHUMAN_SLOTS="2")
    old = {k: os.environ.get(k) for k in new}
    os.environ.update(new)
    try:
        st = _run(lambda: eng.run(in1, p("o1"), **kw), tmp / (tag + ".stderr"))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    files = {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}
    for f in inflate:
        assert files[f][-28:] == bm.BGZF_EOF
        files[f] = gzip.decompress(files[f])
    numbers = {f: getattr(st, f) for f, _t in st._fields_ if f != "seconds"}
    numbers.update({k: v for k, v in vars(st).items()})
    if request == "A":
        numbers["read_stats"] = bytes(rs.raw)
    return files, numbers


def check(tmp, eng, ins, env, request, want_files, inflate=()):
    batched, nb = one_run(tmp, "batched", eng, ins, env, request, inflate)
    whole, nw = one_run(tmp, "whole", eng, ins, {}, request, inflate)
    print("%s %s: %s" % (request, env, {f: len(b) for f, b in batched.items()}), {k: v for k, v in nb.items() if k != "read_stats"})
    assert set(want_files) <= set(batched) and sorted(batched) == sorted(whole), (sorted(batched), sorted(whole))
    for f in want_files:
        assert len(batched[f]) > 0, f
    for f in batched:
        assert batched[f] == whole[f], "%s differs between the run in batches and the run in one" % f
    assert nb == nw and nb["classified"] > 0 and nb["unclassified"] > 0, (nb, nw)
    return nb


A_FILES = ("o1", "h1", "calls", "ids", "rs", "bed", "k", "r", "t10_1")


def test_split_run_with_every_extra_count_cut(tmp_path, eng):
    n = check(tmp_path, eng, count_cut_fastq(tmp_path), COUNT_CUT, "A", A_FILES + ("o2", "h2", "t10_2"))
    assert n["total_sequences"] == 8 * BATCH_FRAGS and n["spared_fragments"] > 0 and n["dust_masked_bases"] > 0 and n["intervals"] > 0


def test_split_run_with_every_extra_text_cut(tmp_path, eng):
    n = check(tmp_path, eng, text_cut_fastq(tmp_path), TEXT_CUT, "A", A_FILES)
    assert n["total_sequences"] == 32 + 20000 and n["spared_fragments"] > 0 and n["dust_masked_bases"] > 0 and n["intervals"] > 0


def test_host_bases_only_count_cut(tmp_path, eng):
    n = check(tmp_path, eng, count_cut_fastq(tmp_path), COUNT_CUT, "B", ("o1", "o2", "bed", "k", "r"))
    assert n["masked_bases"] > 0 and n["closed_bases"] > 0


def test_host_bases_only_text_cut(tmp_path, eng):
    n = check(tmp_path, eng, text_cut_fastq(tmp_path), TEXT_CUT, "B", ("o1", "bed", "k", "r"))
    assert n["masked_bases"] > 0 and n["closed_bases"] > 0


def test_bam_in_bam_out_count_cut(tmp_path, eng):
    n = check(tmp_path, eng, paired_bam(tmp_path), COUNT_CUT, "C", ("o1", "h1", "calls", "k", "r"), inflate=("o1", "h1"))
    assert n["total_sequences"] == 8 * BATCH_FRAGS
