"""Minimizer data (nh_run_mdata / nh_run_engine_mdata, nh_minimizer_*_device, `--report-minimizer-data`, `--minimizer-table`):
the entries are declared, bound and exported; the structs have their sizes and no struct of an existing caller changed; every
argument error is NH_EINVAL before a device is touched or a file created; the CLI, the Python keywords and the runner mirror carry
the flags.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1
ENTRIES = ("nh_run_mdata", "nh_run_engine_mdata", "nh_minimizer_marks_bytes", "nh_minimizer_mark_device", "nh_minimizer_count_device")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    assert len(_lib.SYMBOLS["nh_run_mdata"][1]) == len(_lib.SYMBOLS["nh_run_taxa"][1]) + 1
    assert len(_lib.SYMBOLS["nh_run_engine_mdata"][1]) == len(_lib.SYMBOLS["nh_run_engine_taxa"][1]) + 1
    assert len(_lib.SYMBOLS["nh_minimizer_mark_device"][1]) == 10 and len(_lib.SYMBOLS["nh_minimizer_count_device"][1]) == 4


def test_struct_sizes():
    from nohuman_amd import _lib
    assert C.sizeof(_lib.nh_taxon_minimizers) == 72 and C.sizeof(_lib.nh_minimizer_data) == 32
    assert _lib.nh_minimizer_data.table.offset == 8 and _lib.nh_minimizer_data.taxa.offset == 16
    assert (_lib.nh_minimizer_data.taxa_cap.offset, _lib.nh_minimizer_data.n_taxa.offset) == (24, 28)
    # the structs that existing callers pass keep their sizes
    assert C.sizeof(_lib.nh_run_args) == 7 * 8 + 8 + 4 * 3 + 4 + 8 + 8 and C.sizeof(_lib.nh_run_extras) == 40
    assert C.sizeof(_lib.nh_stats) == 48 and C.sizeof(_lib.nh_taxon_out) == 32


@pytest.fixture
def files(tmp_path):
    (tmp_path / "a.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    return tmp_path


def _args(d, report=True):
    from nohuman_amd import _lib
    a = _lib.nh_run_args()
    a.db_dir = DB.encode()
    a.in1 = str(d / "a.fq").encode()
    a.out1 = str(d / "o.fq").encode()
    a.kraken_output = str(d / "k.txt").encode()
    a.report = str(d / "r.txt").encode() if report else None
    return a


def _md(**kw):
    from nohuman_amd import _lib
    md = _lib.nh_minimizer_data()
    md.struct_size = C.sizeof(_lib.nh_minimizer_data)
    for k, v in kw.items():
        setattr(md, k, v)
    return md


def _both(files, a, x, rs_path, outs, n_outs, md):
    """the two run entries (the engine one without an engine) -> their common (code, message)"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    got = []
    for engine in (False, True):
        pre = (None,) if engine else ()
        fn = L.nh_run_engine_mdata if engine else L.nh_run_mdata
        rc = fn(*pre, C.byref(a), C.byref(x) if x is not None else None, 0, rs_path, None, outs, n_outs,
                C.byref(md) if md is not None else None, C.byref(s))
        got.append((rc, L.nh_last_error()))
    assert got[0] == got[1], got
    return got[0]


def test_every_argument_error_comes_before_a_device_and_creates_nothing(files):
    from nohuman_amd import _lib
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode(),
                           human_ids=str(files / "i.txt").encode())
    touts = (_lib.nh_taxon_out * 1)()
    touts[0].taxid, touts[0].out1 = 9606, str(files / "t.fq").encode()
    os.link(files / "a.fq", files / "same_inode.fq")  # the input under another name
    before = sorted(p.name for p in files.iterdir())
    rs_path = str(files / "s.tsv").encode()
    rc, msg = _both(files, _args(files), x, rs_path, touts, 1, _md(struct_size=31, in_report=1))
    assert rc == NH_EINVAL and b"struct_size" in msg
    rc, msg = _both(files, _args(files, report=False), x, rs_path, touts, 1, _md(in_report=1))
    assert rc == NH_EINVAL and b"in_report" in msg and b"report" in msg
    rc, msg = _both(files, _args(files), x, rs_path, touts, 1, _md(table=b""))
    assert rc == NH_EINVAL and b"empty" in msg
    arr = (_lib.nh_taxon_minimizers * 4)()
    rc, msg = _both(files, _args(files), x, rs_path, touts, 1, _md(taxa=arr, taxa_cap=0))
    assert rc == NH_EINVAL and b"taxa_cap" in msg
    for name, role in (("a.fq", "input"), ("same_inode.fq", "input"), ("o.fq", "output"), ("k.txt", "output"), ("r.txt", "output"),
                       ("c.txt", "output"), ("i.txt", "output"), ("s.tsv", "output"), ("t.fq", "output")):
        path = str(files / name).encode()
        rc, msg = _both(files, _args(files), x, rs_path, touts, 1, _md(table=path))
        assert rc == NH_EINVAL and path in msg and role.encode() in msg, (name, msg)
    assert sorted(p.name for p in files.iterdir()) == before  # no file created


def test_without_md_it_is_nh_run_taxa(files):
    """md NULL, and md with nothing asked for, reach nh_run_taxa's own checks with nh_run_taxa's messages"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode())
    for md in (None, _md()):
        for q in (94, 2 ** 32 - 1):
            assert L.nh_run_taxa(C.byref(_args(files)), C.byref(x), q, None, None, None, 0, C.byref(s)) == NH_EINVAL
            want = L.nh_last_error()
            assert b"93" in want
            mdp = C.byref(md) if md is not None else None
            assert L.nh_run_mdata(C.byref(_args(files)), C.byref(x), q, None, None, None, 0, mdp, C.byref(s)) == NH_EINVAL
            assert L.nh_last_error() == want
        touts = (_lib.nh_taxon_out * 1)()
        touts[0].taxid, touts[0].out1 = 9606, str(files / "o.fq").encode()  # a per-taxon file that is out1
        rc, msg = _both(files, _args(files), x, None, touts, 1, md)
        assert rc == NH_EINVAL and b"nh_run_taxa" in msg and b"o.fq" in msg
        # nothing wrong: the next refusal is the null engine
        assert L.nh_run_engine_mdata(None, C.byref(_args(files)), C.byref(x), 0, None, None, None, 0,
                                     C.byref(md) if md is not None else None, C.byref(s)) == NH_EINVAL
        assert b"null engine" in L.nh_last_error()
    assert not (files / "o.fq").exists()


def test_device_entries_refuse_null_arguments():
    from nohuman_amd import _lib
    L = _lib.lib()
    n = C.c_uint64(0)
    assert L.nh_minimizer_marks_bytes(None, C.byref(n)) == NH_EINVAL
    assert L.nh_minimizer_mark_device(None, None, 0, None, None, 0, 0, None, None, None) == NH_EINVAL
    assert L.nh_minimizer_count_device(None, None, None, None) == NH_EINVAL


def test_python_keywords(files):
    from nohuman_amd import Engine, EngineError, engine
    for fn in (engine.run, Engine.run):
        p = inspect.signature(fn).parameters
        assert p["report_minimizer_data"].default is False and p["minimizer_table"].default is None
        assert p["minimizer_data"].default is None
    for name in ("minimizer_mark_device", "minimizer_count_device", "minimizer_marks_bytes"):
        assert callable(getattr(Engine, name))
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), report_minimizer_data=True)
    assert ei.value.code == NH_EINVAL and "report" in ei.value.message
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), minimizer_table=str(files / "a.fq"))
    assert ei.value.code == NH_EINVAL and "input" in ei.value.message
    assert not (files / "o.fq").exists()


def test_runner_mirrors_the_flags():
    from nohuman_amd import CommandRunner
    o = CommandRunner.parse_argv(["--db", "d", "--report", "r.txt", "--report-minimizer-data", "--minimizer-table", "m.tsv",
                                  "--unclassified-out", "o.fq", "in.fq"])
    assert o["report_minimizer_data"] is True and o["minimizer_table"] == "m.tsv" and o["inputs"] == ["in.fq"]
    o = CommandRunner.parse_argv(["--db", "d", "in.fq"])
    assert o["report_minimizer_data"] is False and o["minimizer_table"] is None


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flags(files):
    r = _cli(["--help"])
    assert r.returncode == 0 and "--report-minimizer-data" in r.stdout and "--minimizer-table <FILE>" in r.stdout
    r = _cli(["--db", DB, "--report-minimizer-data", "-o", str(files / "o.fq"), str(files / "a.fq")])
    assert r.returncode == 2 and r.stderr.startswith("error: ") and "try '--help'" in r.stderr and "--kraken-report" in r.stderr
    r = _cli(["--minimizer-table"])
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = _cli(["--db", DB, "--minimizer-table", "x.tsv", "--calls", "x.tsv", "-o", str(files / "o.fq"), str(files / "a.fq")])
    assert r.returncode == 2 and "--minimizer-table" in r.stderr and "same file" in r.stderr
    r = _cli(["--build-db", str(files / "db"), "--reference", str(files / "a.fq"), "--report-minimizer-data"])
    assert r.returncode == 2 and "--report-minimizer-data" in r.stderr
    assert not (files / "o.fq").exists() and not (files / "x.tsv").exists()
