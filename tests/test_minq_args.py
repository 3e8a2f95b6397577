"""kraken2's --minimum-base-quality (nh_quality_mask_device, nh_run_minq / nh_run_engine_minq, `--minimum-base-quality`): the
entries are declared, bound and exported, a threshold above 93 is NH_EINVAL before a device is touched or a file created,
the CLI and the runner mirror parse the flag.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1
ENTRIES = ("nh_quality_mask_device", "nh_run_minq", "nh_run_engine_minq")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    assert len(_lib.SYMBOLS["nh_quality_mask_device"][1]) == 11
    assert len(_lib.SYMBOLS["nh_run_minq"][1]) == 4 and len(_lib.SYMBOLS["nh_run_engine_minq"][1]) == 5


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


def test_threshold_above_93_is_refused_before_any_device(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    before = sorted(p.name for p in files.iterdir())
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode())
    for q in (94, 255, 2 ** 32 - 1):
        for extras in (None, C.byref(x)):
            assert L.nh_run_minq(C.byref(_args(files)), extras, q, C.byref(s)) == NH_EINVAL
            assert b"93" in L.nh_last_error()
            assert L.nh_run_engine_minq(None, C.byref(_args(files)), extras, q, C.byref(s)) == NH_EINVAL
            assert b"93" in L.nh_last_error()
        assert L.nh_quality_mask_device(None, None, 0, None, None, None, 0, q, None, None, None) == NH_EINVAL
        assert b"93" in L.nh_last_error()
    assert sorted(p.name for p in files.iterdir()) == before  # no file created
    # the extras are still checked: the other argument errors of nh_run_ex come through this entry as well
    x.struct_size -= 1
    assert L.nh_run_minq(C.byref(_args(files)), C.byref(x), 20, C.byref(s)) == NH_EINVAL and b"struct_size" in L.nh_last_error()
    assert L.nh_run_engine_minq(None, C.byref(_args(files)), None, 20, C.byref(s)) == NH_EINVAL and b"null engine" in L.nh_last_error()
    assert sorted(p.name for p in files.iterdir()) == before


def test_python_keywords(files):
    from nohuman_amd import Engine, EngineError, engine
    for fn in (engine.run, Engine.run):
        p = inspect.signature(fn).parameters
        assert "min_base_quality" in p and p["min_base_quality"].default == 0
    assert callable(Engine.quality_mask_device)
    for q in (94, -1):
        with pytest.raises(EngineError) as ei:
            engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), min_base_quality=q)
        assert ei.value.code == NH_EINVAL and "93" in ei.value.message
    assert not (files / "o.fq").exists()


def test_runner_mirrors_the_flag():
    from nohuman_amd import CommandRunner
    o = CommandRunner.parse_argv(["--db", "d", "--minimum-base-quality", "20", "--unclassified-out", "o.fq", "in.fq"])
    assert o["minimum_base_quality"] == 20 and o["inputs"] == ["in.fq"]
    assert CommandRunner.parse_argv(["--db", "d", "in.fq"])["minimum_base_quality"] == 0
    assert CommandRunner.parse_argv(["--minimum-base-quality", "93", "in.fq"])["minimum_base_quality"] == 93
    for bad in ("94", "-1", "abc", ""):
        with pytest.raises(OSError) as ei:
            CommandRunner.parse_argv(["--minimum-base-quality", bad, "in.fq"])
        assert "--minimum-base-quality" in str(ei.value)


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flag(files):
    r = _cli(["--help"])
    assert r.returncode == 0 and "--minimum-base-quality <INT>" in r.stdout
    for bad in ("-1", "94", "abc"):
        for form in (["--minimum-base-quality", bad], ["--minimum-base-quality=" + bad]):
            r = _cli(form + ["--db", DB, "-o", str(files / "o.fq"), str(files / "a.fq")])
            assert r.returncode == 2, (form, r.returncode, r.stderr)
            assert "--minimum-base-quality" in r.stderr and "dependencies" not in r.stderr, r.stderr
    r = _cli(["--minimum-base-quality"])
    assert r.returncode == 2 and "a value is required" in r.stderr
    assert not (files / "o.fq").exists() and not (files / "o.fq.partial").exists()
