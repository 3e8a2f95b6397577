"""Runs with --host-intervals on the GPU (nh_run_intervals, `--host-intervals FILE`; nh_cover.hip behind the classifier): the BED
file and the three counts against tests/intervals_model.py applied to the parsed input -- the sequences as the classifier reads
them, the calls from the CPU oracle --, and EVERY OTHER output of the run, byte for byte, against the same run without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import builder_model as bmod
from tests import intervals_model as im
from tests import qmask_model as qm
from tests import rdust_model as rd
from tests.test_gpu_mask import _run
from tests.test_gpu_minq_run import FILES, _inputs, _paths, _read, stats_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
Q = qm.Q_E2E
_CACHE = {}


def toy_lit(toy):
    if "toy" not in _CACHE:
        _CACHE["toy"] = lit.DB.from_images(toy[0], toy[1], toy[2])
    return _CACHE["toy"]


def corpus(toy, name):
    """(texts, records): 150 fragments of the minimum-base-quality corpus, computed once"""
    if name == "ep":  # the mate files swapped: the host reads are mate 2, the ids mate 2's
        texts, records = corpus(toy, "pe")
        return texts[::-1], records[::-1]
    if name not in _CACHE:
        _CACHE[name] = qm.e2e_corpus(toy[3], name == "pe", n=150)
    return _CACHE[name]


def model(ldb, odb, records, q=0, dust=False, host_of=None):
    """the BED file and the counts of a run on `records`: the classifier's view of the sequences, the oracle's calls"""
    frags = rd.masked_fragments(records, q, dust)
    if len(records) == 1:
        frags = [(s,) for s in frags]
    res = rd.classify(odb, records, q, dust)[0]
    return im.bed(ldb, [r.header for r in records[0]], frags, [int(c) for c in res["call"]], odb.external_ids, host_of)


def run(tmp, name, eng, ins, bed=True, env=None, **kw):
    """one run of `eng` -> (the files it wrote, the BED file, stderr, stats)"""
    p = _paths(tmp, name)
    in1, in2 = ins
    args = dict(in2=in2, out2=p["o2"] if in2 else None, kraken_output=p["k"], report=p["r"], threads=4, calls=p["c"], human_ids=p["i"])
    for k, v in kw.items():
        args[k] = p[v] if isinstance(v, str) and v in p else v
    if args.get("human_out1") and not in2:
        args.pop("human_out2", None)
    bedf = os.path.join(os.path.dirname(p["o1"]), "host.bed")
    if bed:
        args["host_intervals"] = bedf
    errf = tmp / (name + ".stderr")
    new = dict(env or {}, NOHUMAN_TRACE="1")
    old = {k: os.environ.get(k) for k in new}
    os.environ.update(new)
    try:
        st = _run(lambda: eng.run(in1, p["o1"], **args), errf)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    codec = kw.get("out_codec", 0)
    files = {x: _read(p[x], codec if x in ("o1", "o2", "h1", "h2") else 0) for x in FILES}
    return files, (open(bedf, "rb").read() if os.path.exists(bedf) else None), errf.read_bytes().decode(errors="replace"), st


def both(tmp, eng, ins, want, env=None, **kw):
    """the run with and without the flag: the BED file and the counts are the model's, everything else is the same bytes"""
    with_, bed, err, st = run(tmp, "with", eng, ins, True, env, **kw)
    without, none, err0, st0 = run(tmp, "without", eng, ins, False, env, **kw)
    text, counts = want
    assert none is None and "host-intervals:" not in err0 and not hasattr(st0, "intervals")
    assert bed == text, (len(bed), len(text), bed[:300], text[:300])
    assert (st.interval_fragments, st.intervals, st.covered_bases) == counts
    assert "host-intervals: %d intervals in %d fragments, %d bases covered" % (counts[1], counts[0], counts[2]) in err, err[-2000:]
    for x in FILES:
        assert with_[x] == without[x], (x, "differs between the run with the flag and the run without")
    assert with_["o1"] is not None and with_["k"] and stats_of(st) == stats_of(st0)
    return with_, st


@pytest.mark.parametrize("name", ["se", "pe", "ep"])
def test_fastq_in_batches(tmp_path, toy, toy_oracle, toy_engine, name):
    """single and paired FASTQ (ids with /1 and /2; "ep": the host reads in the second file), four batches on the slots in turn"""
    texts, records = corpus(toy, name)
    want = model(toy_lit(toy), toy_oracle, records)
    mates = {ln.split(b"\t")[3] for ln in want[0].split(b"\n")[:-1]}
    assert want[1][1] > 50 and mates == ({b"2"} if name == "ep" else {b"1"}) and b"/1\t" not in want[0] and b"/2\t" not in want[0]
    both(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, env={"NOHUMAN_BATCH_FRAGS": "40"})


def test_gzip_input_through_the_gpu_reader(tmp_path, toy, toy_oracle, toy_engine):
    texts, records = corpus(toy, "pe")
    want = model(toy_lit(toy), toy_oracle, records)
    both(tmp_path, toy_engine, _inputs(tmp_path, "in", texts, gz=True), want, env={"NOHUMAN_GZ_READER": "device", "NOHUMAN_BATCH_FRAGS": "64"},
         out_codec=2)


def test_fasta(tmp_path, toy, toy_oracle, toy_engine):
    _t, records = corpus(toy, "se")
    raws = [b">" + r.header[1:] + b"\n" + r.seq + b"\n" for r in records[0]]
    recs = [[bmod.parse_record(x, False) for x in raws]]
    p = tmp_path / "in.fa"
    p.write_bytes(b"".join(raws))
    both(tmp_path, toy_engine, [str(p), None], model(toy_lit(toy), toy_oracle, recs))


@pytest.mark.parametrize("kind", ["mask", "keep_human", "split"])
def test_kinds_of_run(tmp_path, toy, toy_oracle, toy_engine, kind):
    texts, records = corpus(toy, "pe")
    kw = dict(mask=True) if kind == "mask" else dict(keep_human=True) if kind == "keep_human" else dict(human_out1="h1", human_out2="h2")
    both(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), model(toy_lit(toy), toy_oracle, records), **kw)


def test_minimum_base_quality(tmp_path, toy, toy_oracle, toy_engine):
    """the intervals are those of the quality-masked copy: they agree with the calls"""
    texts, records = corpus(toy, "se")
    want = model(toy_lit(toy), toy_oracle, records, q=Q)
    assert want[0] != model(toy_lit(toy), toy_oracle, records)[0]
    both(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, min_base_quality=Q)


def host_table(ldb, host, keep):
    """one byte a node: its deepest listed ancestor-or-self is a host taxid"""
    out = [0] * len(ldb.external)
    for i in range(1, len(out)):
        a = i
        while a and ldb.external[a] not in host and ldb.external[a] not in keep:
            a = ldb.parent[a]
        out[i] = int(bool(a) and ldb.external[a] in host)
    return out


def test_host_taxid(tmp_path, toy, toy_oracle, toy_engine):
    """--host-taxid 10 --keep-taxid 111: a k-mer whose value lies outside clade 10, or in clade 111, is no host k-mer; a read
    called 111 is spared, and its line -- the k-mers it shares with its ancestors -- carries the true call"""
    ldb = toy_lit(toy)
    texts, records = corpus(toy, "se")
    want = model(ldb, toy_oracle, records, host_of=host_table(ldb, {10}, {111}))
    plain = model(ldb, toy_oracle, records)
    assert 0 < want[1][2] < plain[1][2]
    assert {b"10", b"111"} <= {ln.split(b"\t")[4] for ln in want[0].split(b"\n")[:-1]}
    _files, st = both(tmp_path, toy_engine, _inputs(tmp_path, "in", texts), want, host_taxids=[10], keep_taxids=[111])
    assert st.spared_fragments > 0


def test_dust_reads(tmp_path):
    """a database that holds a microsatellite's minimizers: the stretch is host without --dust-reads and has no interval with it"""
    from nohuman_amd import Engine
    from oracle import oracle as orc
    ob, tb, hb = rd.lc_db()[:3]
    ldb, odb = lit.DB.from_images(ob, tb, hb), orc.OracleDB(ob, tb, hb)
    texts, records = rd.e2e_corpus(False, n=100)
    want, plain = model(ldb, odb, records, dust=True), model(ldb, odb, records)
    assert want[1][2] < plain[1][2] and want[1][1] > 10
    with Engine.from_images(ob, tb, hb) as eng:
        both(tmp_path, eng, _inputs(tmp_path, "in", texts), want, dust_reads=True)


def forged_bam(toy, n=60):
    from tests import bam_model as bm
    from tests import synth
    rng = np.random.default_rng(13)
    reads = synth.sample_reads(rng, toy[3], n, lower_rate=0.0, len_jitter=60)
    recs = [bm.forge_record(b"r%d" % i, s or b"A", None, flag=(bm.REVERSE if i % 3 == 1 else 0) | 0x4) for i, s in enumerate(reads)]
    stream = bm.forge_header(b"@HD\tVN:1.6\tSO:unknown\n") + b"".join(recs)
    text, counts, _t, _k = bm.to_fastq(stream)
    assert counts.reverse_complemented >= n // 3 - 1
    return bm.bgzf(stream, 4000), text, reads


@pytest.mark.parametrize("bam_out", [False, True])
def test_bam_input(tmp_path, toy, toy_oracle, toy_engine, bam_out):
    """the coordinates of a BAM record are those of the FASTQ text it is transcoded to: a reverse-strand record is counted on its
    reverse complement"""
    from tests import synth
    bam, text, reads = forged_bam(toy)
    records = [bmod.parse_file(text, True)]
    assert records[0][1].seq == synth.revcomp(reads[1]) != reads[1]
    p = tmp_path / "in.bam"
    p.write_bytes(bam)
    kw = dict(out_codec=6, codec_threads=2) if bam_out else {}
    both(tmp_path, toy_engine, [str(p), None], model(toy_lit(toy), toy_oracle, records), **kw)


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
d = %(tmp)r
st = engine.run(%(db)r, %(in1)r, os.path.join(d, "o1"), in2=%(in2)r, out2=os.path.join(d, "o2"), device_ids=[0, 1], threads=4,
                kraken_output=os.path.join(d, "k"), host_intervals=os.path.join(d, "bed"))
print("CHILD OK %%d %%d %%d" %% (st.interval_fragments, st.intervals, st.covered_bases))
"""


def test_two_logical_devices(tmp_path, toy, toy_oracle):
    """NOHUMAN_FAKE_DEVICES=2: batches in turn on two logical devices, the discipline checked at every launch and copy; the
    devices' counts are summed"""
    texts, records = corpus(toy, "pe")
    text, counts = model(toy_lit(toy), toy_oracle, records)
    in1, in2 = _inputs(tmp_path, "d", texts)
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="20")
    src = CHILD % dict(root=ROOT, tmp=str(tmp_path), db=DB, in1=in1, in2=in2)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK %d %d %d" % counts in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    assert "DEVICE DISCIPLINE" not in out.stderr
    assert (tmp_path / "bed").read_bytes() == text


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli(tmp_path, toy, toy_oracle):
    texts, records = corpus(toy, "pe")
    text, counts = model(toy_lit(toy), toy_oracle, records)
    in1, in2 = _inputs(tmp_path, "cli", texts)
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    outs = {}
    for name, extra in (("with", ["--host-intervals", str(tmp_path / "host.bed")]), ("without", [])):
        o = {x: str(tmp_path / (name + "_" + x)) for x in ("o1", "o2", "k", "c")}
        r = subprocess.run([BIN, "--db", DB, "-t", "4", "-v", "-o", o["o1"], "-O", o["o2"], "-k", o["k"], "--calls", o["c"], in1, in2] + extra,
                           env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = ([open(v, "rb").read() for v in o.values()], r.stderr)
    assert outs["with"][0] == outs["without"][0]
    assert (tmp_path / "host.bed").read_bytes() == text and not (tmp_path / "host.bed.partial").exists()
    assert "Host intervals: %d intervals in %d reads, %d bases covered" % (counts[1], counts[0], counts[2]) in outs["with"][1], outs["with"][1][-2000:]
    assert "Host intervals:" not in outs["without"][1]
