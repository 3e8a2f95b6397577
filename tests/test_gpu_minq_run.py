"""Runs with a minimum base quality on the GPU (nh_run_minq, `--minimum-base-quality`; k_qmask in front of the classifier):
every file of the run -- the records, the -k lines, the report, the calls table, the human ids -- and the stats, byte for
byte against the Python model of tests/qmask_model.py (the CPU oracle on sequences masked in Python; the records from the
original bases).  tests/test_qmask_model.py asserts that the corpora hold reads whose call, counts and hit list the
threshold changes."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import pytest

from tests import qmask_model as qm
from tests.test_gpu_mask import _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
TRACE = re.compile(r"qmask: Q (\d+), (\d+) of (\d+) bases masked, kernel ([0-9.]+) ms")
Q = qm.Q_E2E
FILES = ("o1", "o2", "h1", "h2", "k", "r", "c", "i")
_MODEL = {}


def model(toy, toy_oracle, name):
    """(texts, records, expected): computed once per corpus and shared"""
    if name not in _MODEL:
        texts, records = qm.ont_corpus(toy[3]) if name == "ont" else qm.e2e_corpus(toy[3], name == "pe")
        _MODEL[name] = (texts, records, qm.expected(toy_oracle, records, Q))
    return _MODEL[name]


def _first_diff(a, b):
    n = min(len(a), len(b))
    i = next((k for k in range(n) if a[k] != b[k]), n)
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(a), len(b), i, a[max(0, i - 40):i + 40], b[max(0, i - 40):i + 40])


def _inputs(tmp, name, texts, gz=False):
    ins = []
    for m, text in enumerate(texts):
        p = tmp / ("%s_in%d.fq%s" % (name, m + 1, ".gz" if gz else ""))
        p.write_bytes(gzip.compress(text, 6) if gz else text)
        ins.append(str(p))
    return ins + [None] * (2 - len(ins))


def _paths(tmp, name):
    d = tmp / name
    d.mkdir()
    return {x: str(d / x) for x in FILES}


def _read(path, codec=0):
    if not os.path.exists(path):
        return None
    data = open(path, "rb").read()
    return gzip.decompress(data) if codec == 2 else data


def run(tmp, name, eng, ins, q=Q, env=None, lists=True, **kw):
    """one run of `eng` -> (the files it wrote, stderr, stats)"""
    p = _paths(tmp, name)
    in1, in2 = ins
    args = dict(in2=in2, out2=p["o2"] if in2 else None, kraken_output=p["k"], report=p["r"], threads=4, min_base_quality=q)
    if lists:
        args.update(calls=p["c"], human_ids=p["i"])
    for k, v in kw.items():
        args[k] = p[v] if isinstance(v, str) and v in p else v
    if args.get("human_out1") and not in2:
        args.pop("human_out2", None)
    errf = tmp / (name + ".stderr")
    old = {k: os.environ.get(k) for k in dict(env or {}, NOHUMAN_TRACE="1")}
    os.environ.update(dict(env or {}, NOHUMAN_TRACE="1"))
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


def same(files, want, records, mode="normal", human=False, lists=True, name=""):
    """the run's files against the model's"""
    paired = len(records) == 2
    for m in range(2 if paired else 1):
        got = files["o%d" % (m + 1)]
        assert got == want[mode][m], (name, "out", m + 1, _first_diff(got, want[mode][m]))
        if human:
            got = files["h%d" % (m + 1)]
            assert got == want["keep"][m], (name, "human out", m + 1, _first_diff(got, want["keep"][m]))
    assert files["k"] == want["k"], (name, "-k", _first_diff(files["k"], want["k"]))
    assert files["r"] == want["report"], (name, "report", _first_diff(files["r"], want["report"]))
    if lists:
        assert files["c"] == want["calls"], (name, "calls", _first_diff(files["c"], want["calls"]))
        assert files["i"] == want["ids"], (name, "ids", _first_diff(files["i"], want["ids"]))


def stats_of(st):
    return (st.total_sequences, st.classified, st.unclassified, st.total_bases)


def trace_of(err):
    t = TRACE.findall(err)
    assert len(t) == 1, err[-3000:]
    return int(t[0][0]), int(t[0][1]), int(t[0][2])


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("corpus", ["se", "pe"])
def test_plain_and_gzip_runs(tmp_path, toy, toy_oracle, toy_engine, corpus, gz):
    """plain -> plain and gzip -> gzip; the trace line's masked count is the model's"""
    texts, records, want = model(toy, toy_oracle, corpus)
    files, err, st = run(tmp_path, "r", toy_engine, _inputs(tmp_path, "r", texts, gz), out_codec=2 if gz else 0,
                         env={"NOHUMAN_BATCH_FRAGS": "150"})
    same(files, want, records, name=corpus)
    assert stats_of(st) == want["stats"]
    assert trace_of(err) == (Q, want["masked_bases"], want["stats"][3])


def test_reader_on_the_gpu(tmp_path, toy, toy_oracle, toy_engine):
    """gzip in, gzip out, the batches born on the GPU: the record table is still the host's"""
    texts, records, want = model(toy, toy_oracle, "pe")
    files, err, st = run(tmp_path, "g", toy_engine, _inputs(tmp_path, "g", texts, True), out_codec=2,
                         env={"NOHUMAN_GZ_READER": "device", "NOHUMAN_BATCH_FRAGS": "130"})
    assert "gzip reader: GPU / GPU" in err, err[-2000:]
    same(files, want, records, name="gpu reader")
    assert stats_of(st) == want["stats"] and trace_of(err)[1] == want["masked_bases"]


@pytest.mark.parametrize("corpus", ["se", "pe"])
def test_split_masked_and_keep_human_runs(tmp_path, toy, toy_oracle, toy_engine, corpus):
    texts, records, want = model(toy, toy_oracle, corpus)
    ins = _inputs(tmp_path, "m", texts)
    files, _err, st = run(tmp_path, "split", toy_engine, ins, human_out1="h1", human_out2="h2")
    same(files, want, records, human=True, name="split")
    assert stats_of(st) == want["stats"]
    files, _err, st = run(tmp_path, "mask", toy_engine, ins, mask=True, lists=False)
    same(files, want, records, mode="masked", lists=False, name="mask")
    assert stats_of(st) == want["stats"]
    files, _err, st = run(tmp_path, "keep", toy_engine, ins, keep_human=True, lists=False)
    same(files, want, records, mode="keep", lists=False, name="-H")
    assert stats_of(st) == want["stats"]


def test_halves_used_in_parts(tmp_path, toy, toy_oracle, toy_engine):
    """paired batches cut by text: the halves differ in length and are used in parts"""
    texts, records, want = model(toy, toy_oracle, "pe")
    files, _err, st = run(tmp_path, "parts", toy_engine, _inputs(tmp_path, "parts", texts), env={"NOHUMAN_BATCH_TEXT": "20000"})
    same(files, want, records, name="parts")
    assert stats_of(st) == want["stats"]


def test_long_reads_cut_into_segments(tmp_path, toy, toy_oracle, toy_engine):
    """ONT-like reads with low-quality stretches across the cuts between their segments"""
    texts, records, want = model(toy, toy_oracle, "ont")
    files, err, st = run(tmp_path, "ont", toy_engine, _inputs(tmp_path, "ont", texts))
    same(files, want, records, name="ont")
    assert stats_of(st) == want["stats"] and trace_of(err)[1] == want["masked_bases"]


def test_threshold_zero_is_the_run_without_it(tmp_path, toy, toy_oracle, toy_engine):
    """nh_run_engine_minq with Q = 0 against nh_run_engine_ex and nh_run_engine: the same bytes, and no qmask trace line"""
    from nohuman_amd import _lib
    from nohuman_amd.engine import _extras
    texts, _records, want = model(toy, toy_oracle, "pe")
    in1, in2 = _inputs(tmp_path, "z", texts)
    L = _lib.lib()
    out = {}
    os.environ["NOHUMAN_TRACE"] = "1"
    try:
        for name, lists in (("minq0", True), ("ex", True), ("minq0_plain", False), ("plain", False)):
            p = _paths(tmp_path, name)
            a = _lib.nh_run_args(in1=in1.encode(), in2=in2.encode(), out1=p["o1"].encode(), out2=p["o2"].encode(),
                                 kraken_output=p["k"].encode(), report=p["r"].encode(), threads=4, n_devices=1)
            x = _extras(False, None, None, p["c"], p["i"]) if lists else None
            s = _lib.nh_stats()
            fn = {"minq0": lambda: L.nh_run_engine_minq(toy_engine.handle, C.byref(a), C.byref(x), 0, C.byref(s)),
                  "ex": lambda: L.nh_run_engine_ex(toy_engine.handle, C.byref(a), C.byref(x), C.byref(s)),
                  "minq0_plain": lambda: L.nh_run_engine_minq(toy_engine.handle, C.byref(a), None, 0, C.byref(s)),
                  "plain": lambda: L.nh_run_engine(toy_engine.handle, C.byref(a), C.byref(s))}[name]
            errf = tmp_path / (name + ".stderr")
            assert _run(fn, errf) == 0, L.nh_last_error()
            assert "qmask" not in errf.read_text(errors="replace")
            out[name] = ({f: _read(p[f]) for f in FILES}, stats_of(s))
    finally:
        os.environ.pop("NOHUMAN_TRACE", None)
    assert out["minq0"] == out["ex"] and out["minq0_plain"] == out["plain"]
    assert out["ex"][0]["k"] != want["k"]  # (and the threshold does change this corpus's run)


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine
d = %(tmp)r
engine.run(%(db)r, %(in1)r, os.path.join(d, "o1"), in2=%(in2)r, out2=os.path.join(d, "o2"), device_ids=[0, 1, 2], threads=4,
           kraken_output=os.path.join(d, "k"), report=os.path.join(d, "r"), calls=os.path.join(d, "c"),
           human_ids=os.path.join(d, "i"), min_base_quality=%(q)d)
print("CHILD OK")
"""


def test_three_logical_devices(tmp_path, toy, toy_oracle):
    """NOHUMAN_FAKE_DEVICES=3: batches in turn on three logical devices, the discipline checked at every launch and copy"""
    texts, records, want = model(toy, toy_oracle, "pe")
    in1, in2 = _inputs(tmp_path, "d", texts)
    p = _paths(tmp_path, "three")
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="3", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="60")
    src = CHILD % dict(root=ROOT, tmp=os.path.dirname(p["o1"]), db=DB, in1=in1, in2=in2, q=Q)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    assert "DEVICE DISCIPLINE" not in out.stderr
    same({f: _read(p[f]) for f in FILES}, want, records, name="three devices")


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flag_writes_what_the_python_entry_writes(tmp_path, toy, toy_oracle):
    texts, records, want = model(toy, toy_oracle, "pe")
    in1, in2 = _inputs(tmp_path, "cli", texts)
    p = _paths(tmp_path, "cli")
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    args = ["--db", DB, "-t", "4", "--minimum-base-quality", str(Q), "-o", p["o1"], "-O", p["o2"], "-k", p["k"], "-r", p["r"],
            "--calls", p["c"], "--human-ids", p["i"], in1, in2]
    r = subprocess.run([BIN] + args, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    same({f: _read(p[f]) for f in FILES}, want, records, name="cli")
    # ... and without the lists: nh_run_minq with no extras
    q = _paths(tmp_path, "cli2")
    r = subprocess.run([BIN, "--db", DB, "--minimum-base-quality=%d" % Q, "-o", q["o1"], "-O", q["o2"], "-k", q["k"], in1, in2],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _read(q["o1"]) == want["normal"][0] and _read(q["o2"]) == want["normal"][1] and _read(q["k"]) == want["k"]


def test_quality_line_of_another_length_fails_the_run(tmp_path, toy_engine):
    """kraken2 ends such a run; here the message names both lengths, and the same file runs without a threshold"""
    from nohuman_amd import EngineError
    p = tmp_path / "bad.fq"
    p.write_bytes(b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGTACGTAC\n+\nIIIIIII\n@c\nACGT\n+\nIIII\n")
    with pytest.raises(EngineError) as ei:
        toy_engine.run(str(p), str(tmp_path / "o.fq"), min_base_quality=Q)
    assert ei.value.code == -2 and "(10)" in ei.value.message and "(7)" in ei.value.message and "read 2" in ei.value.message
    st = toy_engine.run(str(p), str(tmp_path / "o.fq"))
    assert st.total_sequences == 3
