"""Runs with read statistics on the GPU (nh_run_rstats, `--read-stats`; k_rstats behind the classifier): the table and the
returned numbers against the Python model of tests/rstats_model.py on the corpora of tests/qmask_model.py (the CPU oracle's
calls; tests/test_rstats_model.py asserts that they put reads in both classes), every other file of the run byte for byte
against the same run without the option, and the same numbers whatever the batches, the devices and the kind of run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import qmask_model as qm
from tests import rstats_model as rm
from tests.test_gpu_minq_run import _inputs, _paths, _read, run, stats_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
TRACE = re.compile(r"rstats: (\d+) bases, kernel ([0-9.]+) ms")
Q = qm.Q_E2E
GPU_READER = {"NOHUMAN_GZ_READER": "device", "NOHUMAN_GZDEV_MIN_BYTES": "0"}
_MODEL = {}


def model(toy, toy_oracle, name, q=0):
    """(texts, records, the run's files and stats, the statistics' summary, their table): once per corpus and threshold"""
    if (name, q) not in _MODEL:
        texts, records = qm.ont_corpus(toy[3]) if name == "ont" else qm.e2e_corpus(toy[3], name == "pe")
        want = qm.expected(toy_oracle, records, q)
        sm = rm.summary(rm.reads_of_records(records, want["res"]["call"]), len(records))
        _MODEL[(name, q)] = (texts, records, want, sm, rm.table(sm))
    return _MODEL[(name, q)]


def same_numbers(raw, sm, name=""):
    got = rm.summary_of_struct(raw)
    assert got["mates"] == sm["mates"], name
    for key in ("cls", "median", "n50"):
        diff = np.argwhere(got[key] != sm[key])
        assert diff.size == 0, (name, key, [(tuple(int(x) for x in d), int(got[key][tuple(d)]), int(sm[key][tuple(d)])) for d in diff[:8]])


def same_table(path, table, name=""):
    got = open(path, "rb").read()
    assert rm.same_table(got, table) is None, (name, rm.same_table(got, table), got, table)


def with_stats(tmp, name, eng, ins, sm, table, **kw):
    """a run with the option: its numbers and its table are the model's; -> (files, stderr, stats)"""
    from nohuman_amd import ReadStats
    rs = ReadStats(str(tmp / (name + ".stats.tsv")))
    files, err, st = run(tmp, name, eng, ins, read_stats=rs, **kw)
    same_numbers(rs.raw, sm, name)
    same_table(rs.path, table, name)
    return files, err, st


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("corpus", ["se", "pe", "ont"])
def test_plain_and_gzip_runs(tmp_path, toy, toy_oracle, toy_engine, corpus, gz):
    """plain -> plain, and gzip -> gzip with the reader on the GPU (the text never reaches the host); the run without the
    option writes the same bytes and prints no rstats line"""
    texts, records, want, sm, table = model(toy, toy_oracle, corpus)
    ins = _inputs(tmp_path, "r", texts, gz)
    kw = dict(q=0, out_codec=2 if gz else 0, env=dict(GPU_READER if gz else {}, NOHUMAN_BATCH_FRAGS="150"))
    files, err, st = with_stats(tmp_path, "with", toy_engine, ins, sm, table, **kw)
    if gz:
        assert "gzip reader: GPU" in err, err[-2000:]
    t = TRACE.findall(err)
    assert len(t) == 1 and int(t[0][0]) == want["stats"][3], err[-3000:]
    assert stats_of(st) == want["stats"]
    plain, perr, pst = run(tmp_path, "without", toy_engine, ins, **kw)
    assert "rstats:" not in perr
    assert files == plain and stats_of(st) == stats_of(pst)
    assert files["k"] == want["k"] and files["c"] == want["calls"]
    # the numbers of the table hold what the run's own totals hold
    assert int(sm["cls"][:, :, rm.READS].sum()) == want["stats"][0] * len(records) and int(sm["cls"][1, 0, rm.READS]) == want["stats"][1]


@pytest.mark.parametrize("corpus", ["se", "pe"])
def test_whatever_the_batches(tmp_path, toy, toy_oracle, toy_engine, corpus):
    """one batch, many batches, paired batches cut by text (halves used in parts)"""
    texts, _records, _want, sm, table = model(toy, toy_oracle, corpus)
    ins = _inputs(tmp_path, "b", texts)
    for name, env in (("one", {}), ("many", {"NOHUMAN_BATCH_FRAGS": "37"}), ("parts", {"NOHUMAN_BATCH_TEXT": "20000"})):
        with_stats(tmp_path, name, toy_engine, ins, sm, table, q=0, env=env, lists=False)


@pytest.mark.parametrize("corpus", ["se", "pe"])
def test_whatever_the_kind_of_run(tmp_path, toy, toy_oracle, toy_engine, corpus):
    """masked, split, -H: the sets follow the calls, not what the run writes; only the table path, no struct, and the reverse"""
    from nohuman_amd import ReadStats
    texts, records, want, sm, table = model(toy, toy_oracle, corpus)
    ins = _inputs(tmp_path, "m", texts)
    files, _err, _st = with_stats(tmp_path, "mask", toy_engine, ins, sm, table, q=0, mask=True, lists=False)
    assert files["o1"] == want["masked"][0]
    files, _err, _st = with_stats(tmp_path, "split", toy_engine, ins, sm, table, q=0, human_out1="h1", human_out2="h2")
    assert files["h1"] == want["keep"][0] and files["o1"] == want["normal"][0]
    files, _err, _st = with_stats(tmp_path, "keep", toy_engine, ins, sm, table, q=0, keep_human=True, lists=False)
    assert files["o1"] == want["keep"][0]
    path = str(tmp_path / "only.tsv")
    run(tmp_path, "path", toy_engine, ins, q=0, lists=False, read_stats=path)
    same_table(path, table)
    rs = ReadStats()
    run(tmp_path, "struct", toy_engine, ins, q=0, lists=False, read_stats=rs)
    same_numbers(rs.raw, sm)


@pytest.mark.parametrize("corpus", ["se", "pe", "ont"])
def test_with_a_minimum_base_quality(tmp_path, toy, toy_oracle, toy_engine, corpus):
    """the class counts follow the masked calls; the bases counted are the input's: gc and other sum to the Q = 0 run's"""
    texts, records, want, sm, table = model(toy, toy_oracle, corpus, Q)
    _t, _r, want0, sm0, _table0 = model(toy, toy_oracle, corpus)
    if corpus != "ont":  # (the threshold moves reads between the classes of these corpora)
        assert want["stats"][1] != want0["stats"][1] and not np.array_equal(sm["cls"], sm0["cls"])
    ins = _inputs(tmp_path, "q", texts)
    files, err, st = with_stats(tmp_path, "minq", toy_engine, ins, sm, table, q=Q)
    assert stats_of(st) == want["stats"] and files["k"] == want["k"]
    assert "qmask: Q %d" % Q in err and len(TRACE.findall(err)) == 1
    for w in (rm.GC, rm.OTHER, rm.BASES, rm.READS):
        assert int(sm["cls"][:, :, w].sum()) == int(sm0["cls"][:, :, w].sum())


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from nohuman_amd import engine, ReadStats
d = %(tmp)r
engine.run(%(db)r, %(in1)r, os.path.join(d, "o1"), in2=%(in2)r, out2=os.path.join(d, "o2"), device_ids=[0, 1], threads=4,
           kraken_output=os.path.join(d, "k"), read_stats=os.path.join(d, "stats.tsv"))
print("CHILD OK")
"""


def test_two_logical_devices(tmp_path, toy, toy_oracle):
    """NOHUMAN_FAKE_DEVICES=2: an accumulator block per device, rows summed on the host"""
    texts, _records, want, _sm, table = model(toy, toy_oracle, "pe")
    in1, in2 = _inputs(tmp_path, "d", texts)
    p = _paths(tmp_path, "two")
    d = os.path.dirname(p["o1"])
    env = dict(os.environ, NOHUMAN_FAKE_DEVICES="2", NOHUMAN_DEBUG_DEVICE="1", NOHUMAN_RCCL="0", NOHUMAN_BATCH_FRAGS="60")
    src = CHILD % dict(root=ROOT, tmp=d, db=DB, in1=in1, in2=in2)
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    assert "DEVICE DISCIPLINE" not in out.stderr
    same_table(os.path.join(d, "stats.tsv"), table, "two devices")
    assert _read(os.path.join(d, "k")) == want["k"]


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flag(tmp_path, toy, toy_oracle):
    texts, _records, want, _sm, table = model(toy, toy_oracle, "pe")
    in1, in2 = _inputs(tmp_path, "cli", texts)
    p = _paths(tmp_path, "cli")
    stats = os.path.join(os.path.dirname(p["o1"]), "stats.tsv")
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    r = subprocess.run([BIN, "--db", DB, "-t", "4", "--read-stats", stats, "-o", p["o1"], "-O", p["o2"], "-k", p["k"], in1, in2],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Read statistics written to: " in r.stderr and "stats.tsv" in r.stderr
    same_table(stats, table, "cli")
    assert not os.path.exists(stats + ".partial")
    assert _read(p["o1"]) == want["normal"][0] and _read(p["o2"]) == want["normal"][1] and _read(p["k"]) == want["k"]


def test_quality_line_of_another_length_fails_the_run(tmp_path, toy_engine):
    """as with a minimum base quality: the message names both lengths, no table is written, and the same file runs without"""
    from nohuman_amd import EngineError
    p = tmp_path / "bad.fq"
    p.write_bytes(b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGTACGTAC\n+\nIIIIIII\n@c\nACGT\n+\nIIII\n")
    with pytest.raises(EngineError) as ei:
        toy_engine.run(str(p), str(tmp_path / "o.fq"), read_stats=str(tmp_path / "s.tsv"))
    assert ei.value.code == -2 and "(10)" in ei.value.message and "(7)" in ei.value.message and "read 2" in ei.value.message
    assert not (tmp_path / "s.tsv").exists()
    st = toy_engine.run(str(p), str(tmp_path / "o.fq"))
    assert st.total_sequences == 3
