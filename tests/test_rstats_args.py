"""Read statistics (nh_read_stats_device, nh_run_rstats / nh_run_engine_rstats, nh_read_stats_write, `--read-stats`): the
entries are declared, bound and exported; a table path that names an input or another output of the run is NH_EINVAL before
a device is touched or a file created; the table writer against the Python model; the CLI and the runner mirror parse the flag.
No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import rstats_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1
ENTRIES = ("nh_read_stats_device", "nh_run_rstats", "nh_run_engine_rstats", "nh_read_stats_write")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    assert "#define NH_RS_QBINS 94" in hdr and _lib.NH_RS_QBINS == 94
    assert len(_lib.SYMBOLS["nh_read_stats_device"][1]) == 12
    assert len(_lib.SYMBOLS["nh_run_rstats"][1]) == 6 and len(_lib.SYMBOLS["nh_run_engine_rstats"][1]) == 7
    assert C.sizeof(_lib.nh_read_class) == 8 * 102 and C.sizeof(_lib.nh_read_stats) == 4 * 816 + 2 * 48 + 8
    # the structs that existing callers pass keep their sizes
    assert C.sizeof(_lib.nh_stats) == 48 and C.sizeof(_lib.nh_run_extras) == 40


@pytest.fixture
def files(tmp_path):
    (tmp_path / "a.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    return tmp_path


def _args(d):
    from nohuman_amd import _lib
    a = _lib.nh_run_args()
    a.db_dir = DB.encode()
    a.in1 = str(d / "a.fq").encode()
    a.out1 = str(d / "o.fq").encode()
    a.kraken_output = str(d / "k.txt").encode()
    a.report = str(d / "r.txt").encode()
    return a


def test_table_path_that_names_another_file_of_the_run(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    out = _lib.nh_read_stats()
    before = sorted(p.name for p in files.iterdir())
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode(),
                           human_ids=str(files / "i.txt").encode())
    os.link(files / "a.fq", files / "same_inode.fq")  # the input under another name
    before = sorted(p.name for p in files.iterdir())
    for name, role in (("a.fq", "input"), ("same_inode.fq", "input"), ("o.fq", "output"), ("k.txt", "output"), ("r.txt", "output"),
                       ("c.txt", "output"), ("i.txt", "output")):
        path = str(files / name).encode()
        for res in (None, C.byref(out)):
            assert L.nh_run_rstats(C.byref(_args(files)), C.byref(x), 0, path, res, C.byref(s)) == NH_EINVAL, name
            msg = L.nh_last_error()
            assert path in msg and role.encode() in msg, msg
            assert L.nh_run_engine_rstats(None, C.byref(_args(files)), C.byref(x), 0, path, res, C.byref(s)) == NH_EINVAL
            assert path in L.nh_last_error()
    assert L.nh_run_rstats(C.byref(_args(files)), None, 0, b"", None, C.byref(s)) == NH_EINVAL and b"empty" in L.nh_last_error()
    # a path of its own passes the argument checks: the next refusal is the null engine
    assert L.nh_run_engine_rstats(None, C.byref(_args(files)), C.byref(x), 0, str(files / "s.tsv").encode(), None, C.byref(s)) == NH_EINVAL
    assert b"null engine" in L.nh_last_error()
    assert sorted(p.name for p in files.iterdir()) == before  # no file created


def test_without_path_and_struct_it_is_nh_run_minq(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode())
    for q in (94, 2 ** 32 - 1):
        for extras in (None, C.byref(x)):
            assert L.nh_run_minq(C.byref(_args(files)), extras, q, C.byref(s)) == NH_EINVAL
            want = L.nh_last_error()
            assert b"93" in want
            assert L.nh_run_rstats(C.byref(_args(files)), extras, q, None, None, C.byref(s)) == NH_EINVAL
            assert L.nh_last_error() == want
            assert L.nh_run_engine_rstats(None, C.byref(_args(files)), extras, q, None, None, C.byref(s)) == NH_EINVAL
            assert L.nh_last_error() == want
    x.struct_size -= 1
    assert L.nh_run_rstats(C.byref(_args(files)), C.byref(x), 0, None, None, C.byref(s)) == NH_EINVAL and b"struct_size" in L.nh_last_error()
    assert L.nh_run_engine_rstats(None, C.byref(_args(files)), None, 0, None, None, C.byref(s)) == NH_EINVAL and b"null engine" in L.nh_last_error()
    assert not (files / "o.fq").exists()


def _random_reads(rng, mates, n, fasta_mate2=False, lo=33, hi=126):
    reads = []
    for i in range(n):
        human = bool(rng.integers(0, 2))
        for m in range(mates):
            ln = int(rng.integers(0, 400))
            seq = rng.choice(np.frombuffer(b"ACGTacgtNn", dtype=np.uint8), size=ln).tobytes()
            qual = None if (fasta_mate2 and m == 1) else rng.integers(lo, hi + 1, size=ln).astype(np.uint8).tobytes()
            reads.append((m, human, seq, qual))
    return reads


def _written(tmp_path, sm):
    from nohuman_amd import _lib
    raw = rm.fill_struct(sm, _lib.nh_read_stats())
    p = tmp_path / "t.tsv"
    assert _lib.lib().nh_read_stats_write(C.byref(raw), str(p).encode()) == 0, _lib.lib().nh_last_error()
    return p.read_bytes()


def test_table_writer_against_the_model(tmp_path):
    rng = np.random.default_rng(5)
    cases = [rm.summary(_random_reads(rng, 1, 300), 1), rm.summary(_random_reads(rng, 2, 200, fasta_mate2=True), 2),
             rm.summary(_random_reads(rng, 2, 150, lo=35, hi=74), 2), rm.summary([], 1),
             rm.summary([(0, False, b"ACGT", b"IIII"), (0, False, b"", b"")], 1),   # an empty class, a read without bases
             rm.summary([(0, True, b"GGCC", bytes([32, 127, 10, 255]))], 1)]
    for sm in cases:
        got, want = _written(tmp_path, sm), rm.table(sm)
        assert rm.same_table(got, want) is None, (rm.same_table(got, want), got, want)
    # the hand-computed table of tests/test_rstats_model.py, byte for byte
    from tests.test_rstats_model import READS
    assert _written(tmp_path, rm.summary(READS, 1)) == rm.table(rm.summary(READS, 1))


def test_table_writer_refuses_bad_arguments(tmp_path):
    from nohuman_amd import _lib
    L = _lib.lib()
    raw = _lib.nh_read_stats()
    assert L.nh_read_stats_write(None, str(tmp_path / "t").encode()) == NH_EINVAL
    assert L.nh_read_stats_write(C.byref(raw), None) == NH_EINVAL
    assert L.nh_read_stats_write(C.byref(raw), str(tmp_path / "t").encode()) == NH_EINVAL and b"mates" in L.nh_last_error()
    raw.mates = 1
    assert L.nh_read_stats_write(C.byref(raw), str(tmp_path / "no" / "dir" / "t").encode()) == -2


def test_python_keywords(files):
    from nohuman_amd import Engine, EngineError, ReadStats, engine
    for fn in (engine.run, Engine.run):
        p = inspect.signature(fn).parameters
        assert "read_stats" in p and p["read_stats"].default is None
    assert callable(Engine.read_stats_device)
    rs = ReadStats()
    assert rs.path is None and rs.raw.mates == 0
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), read_stats=str(files / "o.fq"))
    assert ei.value.code == NH_EINVAL and "o.fq" in ei.value.message
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), read_stats=ReadStats(str(files / "a.fq")))
    assert ei.value.code == NH_EINVAL and "input" in ei.value.message
    assert not (files / "o.fq").exists()


def test_runner_mirrors_the_flag():
    from nohuman_amd import CommandRunner
    o = CommandRunner.parse_argv(["--db", "d", "--read-stats", "s.tsv", "--unclassified-out", "o.fq", "in.fq"])
    assert o["read_stats"] == "s.tsv" and o["inputs"] == ["in.fq"]
    assert CommandRunner.parse_argv(["--db", "d", "in.fq"])["read_stats"] is None
    o = CommandRunner.parse_argv(["--read-stats", "t", "--minimum-base-quality", "7", "--calls", "c", "in.fq"])
    assert (o["read_stats"], o["minimum_base_quality"], o["calls"]) == ("t", 7, "c")


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flag(files):
    r = _cli(["--help"])
    assert r.returncode == 0 and "--read-stats <FILE>" in r.stdout
    r = _cli(["--read-stats"])
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = _cli(["--db", DB, "--read-stats", "x.tsv", "--calls", "x.tsv", "-o", str(files / "o.fq"), str(files / "a.fq")])
    assert r.returncode == 2 and "--read-stats" in r.stderr and "same file" in r.stderr
    assert not (files / "o.fq").exists() and not (files / "x.tsv").exists()
