"""Runs with --dust-reads on the GPU (nh_run_dust, `--dust-reads`; k_rdust in front of the classifier): every file of the run --
the records, the -k lines, the report, the calls table, the human ids -- and the stats, byte for byte against the Python model
of tests/rdust_model.py (the CPU oracle on sequences masked by tests/dust_model.py, each on its own; the records from the
original bases), on a database whose table holds low-complexity minimizers.  tests/test_rdust_model.py asserts that the
corpora hold reads whose call, counts and hit list the mask changes."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import rdust_model as rd
from tests.test_gpu_mask import _run
from tests.test_gpu_minq_run import FILES, _inputs, _paths, _read, same, stats_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
TRACE = re.compile(r"dust-reads: (\d+) of (\d+) bases masked, kernel ([0-9.]+) ms")
Q = rd.Q_E2E
_MODEL = {}


@pytest.fixture(scope="module")
def lc_oracle():
    from oracle import oracle as orc
    ob, tb, hb = rd.lc_db()[:3]
    return orc.OracleDB(ob, tb, hb)


@pytest.fixture(scope="module")
def lc_engine():
    from nohuman_amd import Engine
    ob, tb, hb = rd.lc_db()[:3]
    eng = Engine.from_images(ob, tb, hb)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def lc_dir(tmp_path_factory):
    return rd.write_db(tmp_path_factory.mktemp("lc_db"))


def model(lc_oracle, name, q=0, dust=True):
    """(texts, records, expected): computed once per corpus and kind of run, and shared"""
    if name not in _MODEL:
        _MODEL[name] = rd.ont_corpus() if name == "ont" else rd.e2e_corpus(name == "pe", fasta=name == "fa")
    texts, records = _MODEL[name]
    key = (name, q, dust)
    if key not in _MODEL:
        _MODEL[key] = rd.expected(lc_oracle, records, q=q, dust=dust)
    return texts, records, _MODEL[key]


def inputs(tmp, name, texts, gz=False, fasta=False):
    ins = _inputs(tmp, name, texts, gz)
    if fasta:
        for p in ins:
            if p:
                os.rename(p, p.replace(".fq", ".fa"))
        ins = [p.replace(".fq", ".fa") if p else None for p in ins]
    return ins


def run(tmp, name, eng, ins, q=0, dust=True, env=None, lists=True, **kw):
    """one run of `eng` -> (the files it wrote, stderr, stats)"""
    p = _paths(tmp, name)
    in1, in2 = ins
    args = dict(in2=in2, out2=p["o2"] if in2 else None, kraken_output=p["k"], report=p["r"], threads=4, min_base_quality=q, dust_reads=dust)
    if lists:
        args.update(calls=p["c"], human_ids=p["i"])
    for k, v in kw.items():
        args[k] = p[v] if isinstance(v, str) and v in p else v
    if args.get("human_out1") and not in2:
        args.pop("human_out2", None)
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
    return files, errf.read_bytes().decode(errors="replace"), st


def trace_of(err):
    t = TRACE.findall(err)
    assert len(t) == 1, err[-3000:]
    return int(t[0][0]), int(t[0][1])


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("corpus", ["se", "pe"])
def test_plain_and_gzip_runs(tmp_path, lc_oracle, lc_engine, corpus, gz):
    """plain -> plain and gzip -> gzip, several batches; masked_bases and the trace line's count are the model's sum"""
    texts, records, want = model(lc_oracle, corpus)
    files, err, st = run(tmp_path, "r", lc_engine, inputs(tmp_path, "r", texts, gz), out_codec=2 if gz else 0,
                         env={"NOHUMAN_BATCH_FRAGS": "70"})
    same(files, want, records, name=corpus)
    assert stats_of(st) == want["stats"]
    assert st.dust_masked_bases == want["masked_bases"] > 0
    assert trace_of(err) == (want["masked_bases"], want["stats"][3])
    assert "qmask" not in err


def test_satellite_read_is_host_without_the_flag_and_kept_with_it(tmp_path, lc_oracle, lc_engine):
    texts, records, want = model(lc_oracle, "se")
    _t, _r, plain = model(lc_oracle, "se", dust=False)
    ins = inputs(tmp_path, "s", texts)
    with_flag, _err, _st = run(tmp_path, "with", lc_engine, ins)
    without, err, st = run(tmp_path, "without", lc_engine, ins, dust=False)
    same(without, plain, records, name="without")
    assert "dust-reads:" not in err and not hasattr(st, "dust_masked_bases")
    sat = [r for f, r in enumerate(records[0]) if f % 5 == 1]
    assert len(sat) == 60
    for r in sat:
        assert r.raw in with_flag["o1"] and r.raw not in without["o1"]  # (kept with its own bases)


def test_fasta(tmp_path, lc_oracle, lc_engine):
    texts, records, want = model(lc_oracle, "fa")
    files, err, st = run(tmp_path, "fa", lc_engine, inputs(tmp_path, "fa", texts, fasta=True), env={"NOHUMAN_BATCH_FRAGS": "110"})
    same(files, want, records, name="fasta")
    assert stats_of(st) == want["stats"] and trace_of(err)[0] == want["masked_bases"] > 0


@pytest.mark.parametrize("corpus", ["se", "pe"])
def test_with_a_minimum_base_quality_the_union_of_the_masks(tmp_path, lc_oracle, lc_engine, corpus):
    texts, records, want = model(lc_oracle, corpus, q=Q)
    _t, _r, dust_only = model(lc_oracle, corpus)
    _t, _r, q_only = model(lc_oracle, corpus, q=Q, dust=False)
    assert want["k"] != dust_only["k"] and want["k"] != q_only["k"]
    files, err, st = run(tmp_path, "u", lc_engine, inputs(tmp_path, "u", texts), q=Q, env={"NOHUMAN_BATCH_FRAGS": "90"})
    same(files, want, records, name="union " + corpus)
    assert stats_of(st) == want["stats"]
    assert trace_of(err)[0] == want["masked_bases"]  # (DUST on the original bases: the count does not depend on Q)
    assert "qmask: Q %d" % Q in err


@pytest.mark.parametrize("corpus", ["se", "pe"])
def test_split_masked_and_keep_human_runs(tmp_path, lc_oracle, lc_engine, corpus):
    texts, records, want = model(lc_oracle, corpus)
    ins = inputs(tmp_path, "m", texts)
    files, _err, st = run(tmp_path, "split", lc_engine, ins, human_out1="h1", human_out2="h2")
    same(files, want, records, human=True, name="split")
    assert stats_of(st) == want["stats"]
    files, _err, st = run(tmp_path, "mask", lc_engine, ins, mask=True, lists=False)
    same(files, want, records, mode="masked", lists=False, name="mask")
    assert stats_of(st) == want["stats"] and st.dust_masked_bases == want["masked_bases"]
    files, _err, st = run(tmp_path, "keep", lc_engine, ins, keep_human=True, lists=False)
    same(files, want, records, mode="keep", lists=False, name="-H")


def test_long_reads(tmp_path, lc_oracle, lc_engine):
    """ONT-like reads of many tiles each, with stretches across the tiles' borders and the classifier's cuts"""
    texts, records, want = model(lc_oracle, "ont")
    files, err, st = run(tmp_path, "ont", lc_engine, inputs(tmp_path, "ont", texts))
    same(files, want, records, name="ont")
    assert stats_of(st) == want["stats"] and trace_of(err)[0] == want["masked_bases"]


def test_without_the_flag_is_nh_run_host(tmp_path, lc_oracle, lc_engine):
    """nh_run_engine_dust with a NULL struct and with enable 0 against nh_run_engine_host: the same bytes, no dust-reads line"""
    from nohuman_amd import _lib
    from nohuman_amd.engine import _extras
    texts, _records, want = model(lc_oracle, "pe")
    in1, in2 = inputs(tmp_path, "z", texts)
    L = _lib.lib()
    out = {}
    os.environ["NOHUMAN_TRACE"] = "1"
    try:
        for name in ("null", "off", "host", "on"):
            p = _paths(tmp_path, name)
            a = _lib.nh_run_args(in1=in1.encode(), in2=in2.encode(), out1=p["o1"].encode(), out2=p["o2"].encode(),
                                 kraken_output=p["k"].encode(), report=p["r"].encode(), threads=4, n_devices=1)
            x = _extras(False, None, None, p["c"], p["i"])
            s = _lib.nh_stats()
            rdd = _lib.nh_read_dust(C.sizeof(_lib.nh_read_dust), 1 if name == "on" else 0, 99)
            h = lc_engine.handle
            fn = {"null": lambda: L.nh_run_engine_dust(h, C.byref(a), C.byref(x), 0, None, None, None, 0, None, None, None, C.byref(s)),
                  "off": lambda: L.nh_run_engine_dust(h, C.byref(a), C.byref(x), 0, None, None, None, 0, None, None, C.byref(rdd), C.byref(s)),
                  "on": lambda: L.nh_run_engine_dust(h, C.byref(a), C.byref(x), 0, None, None, None, 0, None, None, C.byref(rdd), C.byref(s)),
                  "host": lambda: L.nh_run_engine_host(h, C.byref(a), C.byref(x), 0, None, None, None, 0, None, None, C.byref(s))}[name]
            errf = tmp_path / (name + ".stderr")
            assert _run(fn, errf) == 0, L.nh_last_error()
            assert ("dust-reads:" in errf.read_text(errors="replace")) == (name == "on")
            out[name] = ({f: _read(p[f]) for f in FILES}, stats_of(s), int(rdd.masked_bases))
    finally:
        os.environ.pop("NOHUMAN_TRACE", None)
    assert out["null"][:2] == out["host"][:2] and out["off"][:2] == out["host"][:2]
    assert out["off"][2] == 0 and out["on"][2] == want["masked_bases"]
    assert out["on"][0]["k"] == want["k"] != out["host"][0]["k"]


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
d = %(tmp)r
st = engine.run(%(db)r, %(in1)r, os.path.join(d, "o1"), in2=%(in2)r, out2=os.path.join(d, "o2"), device_ids=[0, 1], threads=4,
                kraken_output=os.path.join(d, "k"), report=os.path.join(d, "r"), calls=os.path.join(d, "c"),
                human_ids=os.path.join(d, "i"), dust_reads=True)
print("CHILD OK masked %%d" %% st.dust_masked_bases)
"""


def test_two_logical_devices(tmp_path, lc_oracle, lc_dir):
    """NOHUMAN_FAKE_DEVICES=2: batches in turn on two logical devices, the discipline checked at every launch and copy; the
    devices' counts are summed"""
    texts, records, want = model(lc_oracle, "pe")
    in1, in2 = inputs(tmp_path, "d", texts)
    p = _paths(tmp_path, "two")
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="40")
    src = CHILD % dict(root=ROOT, tmp=os.path.dirname(p["o1"]), db=lc_dir, in1=in1, in2=in2)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK masked %d" % want["masked_bases"] in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    assert "DEVICE DISCIPLINE" not in out.stderr
    same({f: _read(p[f]) for f in FILES}, want, records, name="two devices")


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flag_writes_what_the_python_entry_writes(tmp_path, lc_oracle, lc_dir):
    texts, records, want = model(lc_oracle, "pe")
    in1, in2 = inputs(tmp_path, "cli", texts)
    p = _paths(tmp_path, "cli")
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    args = ["--db", lc_dir, "-t", "4", "--dust-reads", "-v", "-o", p["o1"], "-O", p["o2"], "-k", p["k"], "-r", p["r"],
            "--calls", p["c"], "--human-ids", p["i"], in1, in2]
    r = subprocess.run([BIN] + args, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    same({f: _read(p[f]) for f in FILES}, want, records, name="cli")
    assert "%d low-complexity bases of the reads masked" % want["masked_bases"] in r.stderr, r.stderr[-2000:]
    # ... and with a minimum base quality, without the lists
    _t, _r, both = model(lc_oracle, "pe", q=Q)
    q = _paths(tmp_path, "cli2")
    r = subprocess.run([BIN, "--db", lc_dir, "--dust-reads", "--minimum-base-quality=%d" % Q, "-o", q["o1"], "-O", q["o2"], "-k", q["k"], in1, in2],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _read(q["o1"]) == both["normal"][0] and _read(q["o2"]) == both["normal"][1] and _read(q["k"]) == both["k"]
    assert "low-complexity bases" not in r.stderr  # (logged with -v only)


def test_database_built_without_masking(tmp_path):
    """an unmasked build_db of a genome that carries the satellite (tests/test_gpu_build_db_dust.py's): the microbial read with
    the satellite is removed without the flag and kept, with its bases, with it"""
    import nohuman_amd
    from nohuman_amd import engine
    from tests import build_db_util as u
    from tests.test_gpu_build_db_dust import low_complexity_genome, satellite_read
    fa = u.write_fasta(tmp_path / "genome.fa", low_complexity_genome())
    nohuman_amd.build_db([fa], str(tmp_path / "db"))
    read = satellite_read()
    other = rd.synth.random_seq(np.random.default_rng(5), 150)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@satellite\n" + read + b"\n+\n" + b"I" * len(read) + b"\n@other\n" + other + b"\n+\n" + b"I" * 150 + b"\n")
    kept = {}
    for name, flag in (("with", True), ("without", False)):
        out = tmp_path / (name + ".fq")
        st = engine.run(str(tmp_path / "db"), str(fq), str(out), threads=1, dust_reads=flag)
        kept[name] = out.read_bytes()
        assert st.total_sequences == 2 and st.classified == (0 if flag else 1)
    assert kept["with"] == fq.read_bytes()
    assert b"@satellite\n" not in kept["without"] and b"@other\n" in kept["without"]
