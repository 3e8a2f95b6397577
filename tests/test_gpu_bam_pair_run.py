"""Whole runs on a paired BAM (nh_run* with the paired BAM reader in front, nohuman_amd/csrc/nh_bam.*): a forged BAM of 700
toy-database pairs -- forward and reverse mates, absent qualities on one mate, mate 2 stored first, secondary, supplementary and
empty records before, between and after mates, tags -- against the same run on the two FASTQ files tests/bam_pair_model.py
transcodes it to: every output byte for byte (gzip outputs: their inflated bytes) and the three totals, in batches of 100 pairs so
that several are in flight and the reader's buffer sets come round again; BAM output of pairs (out_codec 6), with and without
human_out1, against bam_pair_model.select_pairs on the calls the run's own calls table states; the same on two logical devices;
the CLI with its default names; and an orphan after 250 good pairs, which ends the run as a malformed second FASTQ file does."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_model as bm
from tests import bam_pair_model as pm
from tests import bamout_model as bo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
N_PAIRS = 700

CHILD = r"""
import gzip, hashlib, json, os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
ids = %(ids)r
res = {}
raw = lambda p: open(p, "rb").read()
for what, kw in (("plain", {}), ("gzip", dict(out_codec=2, codec_threads=2))):
    rd = (lambda p: gzip.decompress(open(p, "rb").read())) if what == "gzip" else raw
    for kind in ("split", "human", "mask", "hostbases", "taxa", "quality"):
        for src, ins in (("bam", dict(in1=%(bam)r)), ("fq", dict(in1=%(fq1)r, in2=%(fq2)r))):
            d = os.path.join(%(tmp)r, "%%s_%%s_%%s" %% (what, kind, src))
            os.mkdir(d)
            p = {x: os.path.join(d, x) for x in ("o1", "o2", "h1", "h2", "c", "i", "s", "k", "r", "b", "t1", "t2", "u1", "u2", "m")}
            common = dict(out2=p["o2"], device_ids=ids, threads=4, **ins, **kw)
            if kind == "split":
                st = engine.run(%(db)r, out1=p["o1"], human_out1=p["h1"], human_out2=p["h2"], calls=p["c"], human_ids=p["i"], read_stats=p["s"],
                                kraken_output=p["k"], report=p["r"], host_intervals=p["b"], **common)
                files = [rd(p[x]) for x in ("o1", "o2", "h1", "h2")] + [raw(p[x]) for x in ("c", "i", "s", "k", "r", "b")]
            elif kind == "human":
                st = engine.run(%(db)r, out1=p["o1"], keep_human=True, kraken_output=p["k"], **common)
                files = [rd(p["o1"]), rd(p["o2"]), raw(p["k"])]
            elif kind == "mask":
                st = engine.run(%(db)r, out1=p["o1"], mask=True, report=p["r"], **common)
                files = [rd(p["o1"]), rd(p["o2"]), raw(p["r"])]
            elif kind == "hostbases":
                st = engine.run(%(db)r, out1=p["o1"], mask=True, host_bases_only=True, host_gap=34, host_intervals=p["b"], **common)
                files = [rd(p["o1"]), rd(p["o2"]), raw(p["b"])]
            elif kind == "taxa":
                st = engine.run(%(db)r, out1=p["o1"], taxon_outs=[(10, p["t1"], p["t2"]), ("other", p["u1"], p["u2"])], **common)
                files = [rd(p[x]) for x in ("o1", "o2", "t1", "t2", "u1", "u2")]
            else:
                st = engine.run(%(db)r, out1=p["o1"], min_base_quality=3, dust_reads=True, host_taxids=[10], calls=p["c"], read_stats=p["s"],
                                report=p["r"], report_minimizer_data=True, minimizer_table=p["m"], **common)
                files = [rd(p["o1"]), rd(p["o2"]), raw(p["c"]), raw(p["s"]), raw(p["r"]), raw(p["m"])]
            res["%%s %%s %%s" %% (what, kind, src)] = [[len(f), hashlib.sha256(f).hexdigest()] for f in files] + \
                [[st.total_sequences, st.classified, st.unclassified]]
# BAM output of pairs: out1 alone, out1 and human_out1, the host records alone
bamout = {}
for name, kw in (("kept", {}), ("split", dict(human_out1="h.bam")), ("human", dict(keep_human=True)), ("host10", dict(host_taxids=[10]))):
    d = os.path.join(%(tmp)r, "bamout_" + name)
    os.mkdir(d)
    if "human_out1" in kw:
        kw["human_out1"] = os.path.join(d, "h.bam")
    st = engine.run(%(db)r, %(bam)r, os.path.join(d, "o.bam"), out_codec=6, calls=os.path.join(d, "c.tsv"), kraken_output=os.path.join(d, "k.txt"),
                    device_ids=ids, threads=4, **kw)
    bamout[name] = [sorted(os.listdir(d)), [st.total_sequences, st.classified, st.unclassified]]
print("RESULT " + json.dumps([res, bamout]))
"""


def forged_pairs(genomes, n=N_PAIRS, seed=3):
    """-> the BAM stream of n toy-database pairs with what a collated BAM may hold in between"""
    from tests import synth
    rng = np.random.default_rng(seed)
    reads = synth.sample_reads(rng, genomes, n, paired=True, lower_rate=0.0, len_jitter=60)
    recs = [bm.forge_record(b"sec_first", b"ACGTAC", None, flag=bm.SECONDARY | pm.P1, cigar=[(6 << 4)])]
    for i, (s1, s2) in enumerate(reads):
        s1, s2 = s1 or b"A", s2 or b"C"
        q1 = None if i % 11 == 5 else rng.integers(2, 42, len(s1), dtype=np.uint8).tobytes()
        q2 = None if i % 13 == 7 else rng.integers(2, 42, len(s2), dtype=np.uint8).tobytes()
        between = []
        if i % 9 == 0:
            between.append(bm.forge_record(b"sec%d" % i, s1[:50], None, flag=bm.SECONDARY | pm.P1, cigar=[(len(s1[:50]) << 4)]))
        if i % 17 == 0:
            between.append(bm.forge_record(b"empty%d" % i, b"", b"", flag=0x4))
        recs += pm.forge_pair(b"pair%d/%d ch=%d" % (i, i % 7, i % 512) if i % 2 else b"p%d" % i, s1, s2, q1, q2, rev=(i % 3 == 1, i % 4 == 2),
                              mate2_first=i % 5 == 3, between=between, tags=(b"RGZgrp\0" if i % 4 == 0 else b"", b"qsi\x0c\0\0\0" if i % 3 == 0 else b""),
                              extra_flag=0x4 | 0x8)
        if i % 13 == 0:
            recs.append(bm.forge_record(b"sup%d" % i, s2[:30], bytes(len(s2[:30])), flag=bm.SUPPLEMENTARY | bm.REVERSE | pm.P2))
    return bm.forge_header(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@RG\tID:grp\n") + b"".join(recs)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, toy):
    tmp = tmp_path_factory.mktemp("bam_pair_run")
    stream = forged_pairs(toy[3])
    t1, t2, pc = pm.to_fastq_pair(stream)
    _, counts = pm.file_order_fastq(stream)
    ps = pm.pairs(stream)
    assert pc.pairs == N_PAIRS and counts.reads == 2 * N_PAIRS and counts.skipped_secondary > 100 and counts.skipped_empty > 20
    assert sum(a is m2 for _, m2, a, _ in ps) > 100 and sum(b.ordinal - a.ordinal > 1 for _, _, a, b in ps) > 50
    assert counts.reverse_complemented > 300 and counts.missing_qualities > 80
    bam, fq1, fq2 = tmp / "reads.bam", tmp / "reads_1.fq", tmp / "reads_2.fq"
    bam.write_bytes(bm.bgzf(stream, 4000))
    fq1.write_bytes(t1)
    fq2.write_bytes(t2)
    return str(bam), str(fq1), str(fq2), counts, stream


def _flags(calls_path, n):
    """the host flag of every pair as the run's calls table states it"""
    lines = open(calls_path, "rb").read().split(b"\n")[:-1]
    assert len(lines) == n and all(ln[:2] in (b"C\t", b"U\t") for ln in lines)
    return [ln[:1] == b"C" for ln in lines]


def _check_bam_out(tmp_path, stream, name, listing, host_is_taxon_10=False):
    d = tmp_path / ("bamout_" + name)
    flags = _flags(str(d / "c.tsv"), N_PAIRS)
    if host_is_taxon_10:  # (the calls table states the true call: the host pairs are those whose call lies in taxon 10's clade)
        lines = open(str(d / "c.tsv"), "rb").read().split(b"\n")[:-1]
        flags = [ln.split(b"\t")[2] in (b"10", b"11", b"12", b"111", b"112") for ln in lines]
    assert 0 < sum(flags) < N_PAIRS
    outs = {"o.bam": name == "human"}
    if name == "split":
        outs["h.bam"] = True
    assert listing == sorted(list(outs) + ["c.tsv", "k.txt"])
    for fn, want in outs.items():
        data = gzip.decompress((d / fn).read_bytes())
        assert data == pm.select_pairs(stream, flags, want), (name, fn)
        assert (d / fn).read_bytes().endswith(bm.BGZF_EOF)
        head, recs = pm.parse(data)
        assert head == pm.header_bytes(stream) and len(recs) == 2 * sum(f == want for f in flags)
        old = bm.PAIRED
        bm.PAIRED = 0  # (tests/bam_model.py's walk refuses flag 0x1: lifted, tests/bamout_model.parse reads the output as it stands)
        try:
            assert bo.parse(data) == (head, recs)
        finally:
            bm.PAIRED = old


def _child(tmp_path, inputs, ids, extra_env):
    bam, fq1, fq2, counts, stream = inputs
    env = dict(os.environ, NOHUMAN_BATCH_FRAGS="100", NOHUMAN_RCCL="0", NOHUMAN_TRACE="1", **extra_env)
    env.pop("NOHUMAN_GZ_READER", None)
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), db=DB, bam=bam, fq1=fq1, fq2=fq2, ids=ids)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res, bamout = json.loads(out.stdout.split("RESULT ")[1])
    totals = None
    for what in ("plain", "gzip"):
        for kind in ("split", "human", "mask", "hostbases", "taxa", "quality"):
            b, f = res["%s %s bam" % (what, kind)], res["%s %s fq" % (what, kind)]
            assert b == f, (what, kind, b, f)
            assert b[-1][0] == N_PAIRS and 0 < b[-1][1] < N_PAIRS, (what, kind, b[-1])
            assert all(n > 0 for n, _ in b[:-1]), (what, kind, b)
            if kind == "split":
                totals = b[-1]
    assert "BAM reader: %d records, %d kept" % (counts.records, counts.reads) in out.stderr
    for name, (listing, st) in bamout.items():
        assert st == totals, (name, st, totals)
        _check_bam_out(tmp_path, stream, name, listing, host_is_taxon_10=name == "host10")
    return out.stderr


def test_every_output_of_a_paired_bam_run_is_the_two_fastq_run_s(tmp_path, inputs):
    err = _child(tmp_path, inputs, [0], {})
    assert "bam-out:" in err


def test_the_same_on_two_logical_devices(tmp_path, inputs):
    err = _child(tmp_path, inputs, [0, 1], {"NOHUMAN_FAKE_DEVICES": "2", "NOHUMAN_DEBUG_DEVICE": "1"})
    assert "DEVICE DISCIPLINE" not in err, [ln for ln in err.splitlines() if "DISCIPLINE" in ln][:3]


def test_cli_with_default_names(tmp_path, inputs):
    assert os.path.exists(BIN), "the CLI host is not built"
    bam, fq1, fq2, counts, stream = inputs
    e = dict(os.environ, NOHUMAN_DEVICES="0")
    o1, o2 = str(tmp_path / "fq.1.fq"), str(tmp_path / "fq.2.fq")
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "-o", o1, "-O", o2, fq1, fq2], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want1, want2 = open(o1, "rb").read(), open(o2, "rb").read()
    assert want1 and want2 and want1.count(b"\n") == want2.count(b"\n")
    work = tmp_path / "w"
    work.mkdir()
    (work / "reads.bam").write_bytes(open(bam, "rb").read())
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "-v", str(work / "reads.bam")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(work)) == ["reads.bam", "reads.nohuman_1.fq.gz", "reads.nohuman_2.fq.gz"]
    assert gzip.decompress((work / "reads.nohuman_1.fq.gz").read_bytes()) == want1
    assert gzip.decompress((work / "reads.nohuman_2.fq.gz").read_bytes()) == want2
    assert "BAM input: paired, %d pairs" % N_PAIRS in r.stderr and "BAM input: %d records, %d kept" % (counts.records, counts.reads) in r.stderr
    # --bam-out: one BAM, both mates of every kept pair, in file order
    calls = str(tmp_path / "calls.tsv")
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "--bam-out", "--calls", calls, str(work / "reads.bam")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(work)) == ["reads.bam", "reads.nohuman.bam", "reads.nohuman_1.fq.gz", "reads.nohuman_2.fq.gz"]
    assert gzip.decompress((work / "reads.nohuman.bam").read_bytes()) == pm.select_pairs(stream, _flags(calls, N_PAIRS), False)


def test_an_orphan_ends_the_run_like_a_malformed_second_fastq(tmp_path, inputs, toy_engine):
    from nohuman_amd import EngineError
    rng = np.random.default_rng(9)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seq = lambda n: acgt[rng.integers(0, 4, n)].tobytes()  # noqa: E731
    good = bm.forge_header() + b"".join(r for i in range(250) for r in pm.forge_pair(b"p%d" % i, seq(120), seq(110), bytes([30]) * 120, bytes([31]) * 110,
                                                                                     mate2_first=i % 2 == 1))
    t1, t2, _ = pm.to_fastq_pair(good)
    bad_bam = tmp_path / "bad.bam"
    bad_bam.write_bytes(bm.bgzf(good + bm.forge_record(b"orphan", b"ACGT", bytes(4), flag=pm.P1)))
    bad1, bad2 = tmp_path / "bad_1.fq", tmp_path / "bad_2.fq"
    bad1.write_bytes(t1 + b"@orphan\nACGT\n+\nIIII\n")
    bad2.write_bytes(t2 + b"Xnot a header\nACGT\n+\nIIII\n")
    left = {}
    os.environ["NOHUMAN_BATCH_FRAGS"] = "100"
    try:
        for name, ins in (("bam", dict(in1=str(bad_bam))), ("fq", dict(in1=str(bad1), in2=str(bad2)))):
            d = tmp_path / name
            d.mkdir()
            with pytest.raises(EngineError) as ei:
                toy_engine.run(out1=str(d / "o1.fq"), out2=str(d / "o2.fq"), human_out1=str(d / "h1.fq"), human_out2=str(d / "h2.fq"),
                               kraken_output=str(d / "k.txt"), threads=4, **ins)
            assert ei.value.code == -2, ei.value.message
            left[name] = (sorted(os.listdir(d)), ei.value.message)
    finally:
        os.environ.pop("NOHUMAN_BATCH_FRAGS", None)
    assert "record 501 (orphan) is the last kept record and has no mate" in left["bam"][1] and "samtools collate" in left["bam"][1]
    assert left["bam"][0] == left["fq"][0]  # whatever a malformed second FASTQ file leaves behind, an orphan leaves
    # the engine is as usable as before
    toy_engine.classify(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), np.array([0, 80], dtype=np.uint64))
