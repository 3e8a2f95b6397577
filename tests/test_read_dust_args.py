"""--dust-reads (nh_run_dust / nh_run_engine_dust, nh_dust_reads_device, `--dust-reads`): the entries are declared, bound and
exported, a struct too small is NH_EINVAL before a device is touched or a file created, the CLI parses the flag and refuses it
beside --build-db, and --mask-low-complexity stays the builder's flag.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1
ENTRIES = ("nh_run_dust", "nh_run_engine_dust", "nh_dust_reads_device")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    # nh_run_host's argument list plus nh_read_dust *
    assert len(_lib.SYMBOLS["nh_run_dust"][1]) == len(_lib.SYMBOLS["nh_run_host"][1]) + 1 == 11
    assert len(_lib.SYMBOLS["nh_run_engine_dust"][1]) == len(_lib.SYMBOLS["nh_run_engine_host"][1]) + 1 == 12
    assert _lib.SYMBOLS["nh_run_dust"][1][:9] == _lib.SYMBOLS["nh_run_host"][1][:9]
    assert len(_lib.SYMBOLS["nh_dust_reads_device"][1]) == 9
    assert C.sizeof(_lib.nh_read_dust) == 16 and _lib.nh_read_dust.masked_bases.offset == 8
    assert "} nh_read_dust;" in hdr and "KEEPS THE INPUT'S BASES" in hdr
    # no existing struct changed size
    assert C.sizeof(_lib.nh_run_extras) == 40 and C.sizeof(_lib.nh_minimizer_data) == 32 and C.sizeof(_lib.nh_host_filter) == 48


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


def test_struct_too_small_is_refused_before_any_device(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    before = sorted(p.name for p in files.iterdir())
    for size in (0, 8, 15):
        for enable in (0, 1):
            rd = _lib.nh_read_dust(size, enable, 77)
            assert L.nh_run_dust(C.byref(_args(files)), None, 0, None, None, None, 0, None, None, C.byref(rd), C.byref(s)) == NH_EINVAL
            assert b"struct_size" in L.nh_last_error() and b"nh_read_dust" in L.nh_last_error()
            assert L.nh_run_engine_dust(None, C.byref(_args(files)), None, 0, None, None, None, 0, None, None, C.byref(rd), C.byref(s)) == NH_EINVAL
            assert b"struct_size" in L.nh_last_error()
            assert rd.masked_bases == 77  # (a struct that small is not written to)
    assert sorted(p.name for p in files.iterdir()) == before  # no file created
    # a good struct: the other argument errors come through this entry as nh_run_host's do
    rd = _lib.nh_read_dust(C.sizeof(_lib.nh_read_dust), 1, 0)
    assert L.nh_run_dust(C.byref(_args(files)), None, 94, None, None, None, 0, None, None, C.byref(rd), C.byref(s)) == NH_EINVAL
    assert b"93" in L.nh_last_error()
    assert L.nh_run_engine_dust(None, C.byref(_args(files)), None, 0, None, None, None, 0, None, None, C.byref(rd), C.byref(s)) == NH_EINVAL
    assert b"null engine" in L.nh_last_error()
    assert L.nh_run_engine_dust(None, C.byref(_args(files)), None, 0, None, None, None, 0, None, None, None, C.byref(s)) == NH_EINVAL
    assert b"null engine" in L.nh_last_error()
    assert L.nh_dust_reads_device(None, None, 0, None, None, 0, None, None, None) == NH_EINVAL
    assert sorted(p.name for p in files.iterdir()) == before


def test_python_keywords():
    from nohuman_amd import Engine, engine
    for fn in (engine.run, Engine.run):
        p = inspect.signature(fn).parameters
        assert "dust_reads" in p and p["dust_reads"].default is False
    assert callable(Engine.dust_reads_device)
    assert list(inspect.signature(Engine.dust_reads_device).parameters)[1:] == [
        "d_text", "text_len", "d_seq_starts", "d_seq_lens", "n_seq", "d_out", "d_masked", "stream"]


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flag(files):
    r = _cli(["--help"])
    assert r.returncode == 0
    line = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--dust-reads")]
    assert len(line) == 1 and "keep their bases" in line[0]
    (files / "g.fa").write_bytes(b">chr\n" + b"ACGT" * 30 + b"\n")
    # beside --build-db: an argument error, before the device probe
    for extra in ([], ["--mask-low-complexity"]):
        r = _cli(["--build-db", str(files / "db"), "--reference", str(files / "g.fa"), "--dust-reads"] + extra)
        assert r.returncode == 2, (r.returncode, r.stderr)
        assert "--dust-reads" in r.stderr and "--build-db" in r.stderr and "dependencies" not in r.stderr, r.stderr
    assert not (files / "db").exists()
    # --mask-low-complexity keeps its meaning for --build-db alone
    for extra in ([], ["--dust-reads"]):
        r = _cli(["--mask-low-complexity", "--db", DB, "-o", str(files / "o.fq"), str(files / "a.fq")] + extra)
        assert r.returncode == 2, (r.returncode, r.stderr)
        assert "--mask-low-complexity" in r.stderr and "--build-db" in r.stderr and "dependencies" not in r.stderr, r.stderr
    assert not (files / "o.fq").exists() and not (files / "o.fq.partial").exists()
