"""Whole runs on a BAM file (nh_run* with the BAM reader in front, nohuman_amd/csrc/nh_bam.*): a forged BAM of toy-database reads
-- forward and reverse-strand records, absent qualities, secondary, supplementary and empty records in between -- against the
same run on the FASTQ tests/bam_model.py transcodes it to: every output byte for byte (gzip outputs: their inflated bytes)
and the three totals, in small batches so that several are in flight and the reader's buffer sets come round again; the same on
two logical devices; the CLI; and a paired record, which ends the run as a malformed FASTQ does."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_model as bm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
N_READS = 700

CHILD = r"""
import gzip, hashlib, json, os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
ids = %(ids)r
res = {}
for what, kw in (("plain", {}), ("gzip", dict(out_codec=2, codec_threads=2))):
    rd = (lambda p: gzip.decompress(open(p, "rb").read())) if what == "gzip" else (lambda p: open(p, "rb").read())
    raw = lambda p: open(p, "rb").read()
    for kind in ("split", "human", "mask"):
        for src, in1 in (("bam", %(bam)r), ("fq", %(fq)r)):
            d = os.path.join(%(tmp)r, "%%s_%%s_%%s" %% (what, kind, src))
            os.mkdir(d)
            p = {x: os.path.join(d, x) for x in ("o", "h", "c", "i", "s", "k", "r")}
            if kind == "split":
                st = engine.run(%(db)r, in1, p["o"], human_out1=p["h"], calls=p["c"], human_ids=p["i"], read_stats=p["s"],
                                kraken_output=p["k"], report=p["r"], device_ids=ids, threads=4, **kw)
                files = [rd(p["o"]), rd(p["h"]), raw(p["c"]), raw(p["i"]), raw(p["s"]), raw(p["k"]), raw(p["r"])]
            elif kind == "human":
                st = engine.run(%(db)r, in1, p["o"], keep_human=True, kraken_output=p["k"], device_ids=ids, threads=4, **kw)
                files = [rd(p["o"]), raw(p["k"])]
            else:
                st = engine.run(%(db)r, in1, p["o"], mask=True, report=p["r"], device_ids=ids, threads=4, **kw)
                files = [rd(p["o"]), raw(p["r"])]
            res["%%s %%s %%s" %% (what, kind, src)] = [[len(f), hashlib.sha256(f).hexdigest()] for f in files] + \
                [[st.total_sequences, st.classified, st.unclassified]]
print("RESULT " + json.dumps(res))
"""


def forged_reads(genomes, n=N_READS, seed=3):
    """-> the BAM stream of n toy-database reads with what a BAM may hold in between"""
    from tests import synth
    rng = np.random.default_rng(seed)
    reads = synth.sample_reads(rng, genomes, n, lower_rate=0.0, len_jitter=60)
    recs = []
    for i, s in enumerate(reads):
        s = s or b"A"
        flag = bm.REVERSE if i % 3 == 1 else 0
        qual = None if i % 11 == 5 else rng.integers(2, 42, len(s), dtype=np.uint8).tobytes()
        recs.append(bm.forge_record(b"read%d/%d ch=%d" % (i, i % 7, i % 512) if i % 2 else b"r%d" % i, s, qual, flag=flag | 0x4,
                                    tags=b"qsi\x0c\0\0\0" if i % 4 == 0 else b""))
        if i % 9 == 0:
            recs.append(bm.forge_record(b"sec%d" % i, s[:50], None, flag=bm.SECONDARY, cigar=[(len(s[:50]) << 4)]))
        if i % 13 == 0:
            recs.append(bm.forge_record(b"sup%d" % i, s[:30], bytes(len(s[:30])), flag=bm.SUPPLEMENTARY | bm.REVERSE))
        if i % 17 == 0:
            recs.append(bm.forge_record(b"empty%d" % i, b"", b""))
    return bm.forge_header(b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:basecaller\n") + b"".join(recs)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, toy):
    tmp = tmp_path_factory.mktemp("bam_run")
    stream = forged_reads(toy[3])
    text, counts, _, _ = bm.to_fastq(stream)
    assert counts.reads == N_READS and counts.skipped_secondary > 50 and counts.skipped_empty > 20
    assert counts.reverse_complemented > 200 and counts.missing_qualities > 40
    bam, fq = tmp / "reads.bam", tmp / "reads.fq"
    bam.write_bytes(bm.bgzf(stream, 4000))
    fq.write_bytes(text)
    return str(bam), str(fq), counts, text


def _child(tmp_path, inputs, ids, extra_env):
    bam, fq, counts, _ = inputs
    env = dict(os.environ, NOHUMAN_BATCH_FRAGS="100", NOHUMAN_RCCL="0", NOHUMAN_TRACE="1", **extra_env)
    env.pop("NOHUMAN_GZ_READER", None)
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), db=DB, bam=bam, fq=fq, ids=ids)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.split("RESULT ")[1])
    for what in ("plain", "gzip"):
        for kind in ("split", "human", "mask"):
            b, f = res["%s %s bam" % (what, kind)], res["%s %s fq" % (what, kind)]
            assert b == f, (what, kind, b, f)
            assert b[-1][0] == counts.reads and 0 < b[-1][1] < counts.reads
            assert all(n > 0 for n, _ in b[:-1]), (what, kind, b)
    assert "BAM reader: %d records, %d kept" % (counts.records, counts.reads) in out.stderr
    return out.stderr


def test_every_output_of_a_bam_run_is_the_fastq_run_s(tmp_path, inputs):
    _child(tmp_path, inputs, [0], {})


def test_the_same_on_two_logical_devices(tmp_path, inputs):
    err = _child(tmp_path, inputs, [0, 1], {"NOHUMAN_FAKE_DEVICES": "2", "NOHUMAN_DEBUG_DEVICE": "1"})
    assert "DEVICE DISCIPLINE" not in err, [ln for ln in err.splitlines() if "DISCIPLINE" in ln][:3]


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli(tmp_path, inputs):
    bam, fq, counts, _ = inputs
    e = dict(os.environ, NOHUMAN_DEVICES="0")
    outs = {}
    for name, src in (("bam", bam), ("fq", fq)):
        o = str(tmp_path / (name + ".out.fq"))
        r = subprocess.run([BIN, "--db", DB, "-t", "4", "-v", "-o", o, src], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = (open(o, "rb").read(), r.stderr)
    assert outs["bam"][0] == outs["fq"][0] and outs["bam"][0].count(b"\n") % 4 == 0 and outs["bam"][0]
    line = "BAM input: %d records, %d kept, %d secondary or supplementary and %d without bases skipped, %d reverse-complemented" % (
        counts.records, counts.reads, counts.skipped_secondary, counts.skipped_empty, counts.reverse_complemented)
    assert line in outs["bam"][1] and "BAM input" not in outs["fq"][1]
    # the default output name: the input's stem, and gzip, the codec the input's magic shows
    work = tmp_path / "w"
    work.mkdir()
    (work / "reads.bam").write_bytes(open(bam, "rb").read())
    r = subprocess.run([BIN, "--db", DB, "-t", "4", str(work / "reads.bam")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(work)) == ["reads.bam", "reads.nohuman.fq.gz"]
    assert gzip.decompress((work / "reads.nohuman.fq.gz").read_bytes()) == outs["bam"][0]
    h = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert "BAM" in h.stdout + h.stderr


def test_a_paired_record_ends_the_run_like_a_malformed_fastq(tmp_path, inputs, toy_engine):
    from nohuman_amd import EngineError
    _, _, _, text = inputs
    recs = text.split(b"\n")
    good = b"\n".join(recs[:4 * 250]) + b"\n"
    bad_fq = tmp_path / "bad.fq"
    bad_fq.write_bytes(good + b"Xnot a header\nACGT\n+\nIIII\n")
    stream = forged_reads_prefix(250)
    bad_bam = tmp_path / "bad.bam"
    bad_bam.write_bytes(bm.bgzf(stream + bm.forge_record(b"mate1", b"ACGT", bytes(4), flag=bm.PAIRED | 0x40)))
    left = {}
    os.environ["NOHUMAN_BATCH_FRAGS"] = "100"
    try:
        for name, src in (("bam", bad_bam), ("fq", bad_fq)):
            d = tmp_path / name
            d.mkdir()
            with pytest.raises(EngineError) as ei:
                toy_engine.run(str(src), str(d / "o.fq"), human_out1=str(d / "h.fq"), kraken_output=str(d / "k.txt"), threads=4)
            assert ei.value.code == -2, ei.value.message
            left[name] = (sorted(os.listdir(d)), ei.value.message)
    finally:
        os.environ.pop("NOHUMAN_BATCH_FRAGS", None)
    assert "record 251 (mate1) is paired" in left["bam"][1] and "samtools fastq -1" in left["bam"][1]
    assert left["bam"][0] == left["fq"][0]  # whatever a malformed FASTQ leaves behind, a malformed BAM leaves
    # the engine is as usable as before
    toy_engine.classify(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), np.array([0, 80], dtype=np.uint64))


def forged_reads_prefix(n):
    """a stream of n plain kept records"""
    rng = np.random.default_rng(9)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return bm.forge_header() + b"".join(
        bm.forge_record(b"p%d" % i, acgt[rng.integers(0, 4, 120)].tobytes(), bytes([30]) * 120, flag=0x4) for i in range(n))
