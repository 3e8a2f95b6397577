"""--host-intervals (nh_run_intervals / nh_run_engine_intervals, nh_host_cover_device, nh_cover_intervals_device,
`--host-intervals FILE`): the entries are declared, bound and exported, a struct too small or a path that names an input or
another output of the run is NH_EINVAL before a device is touched or a file created, hi == NULL goes where nh_run_dust goes,
and the CLI parses the flag.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1
ENTRIES = ("nh_run_intervals", "nh_run_engine_intervals", "nh_host_cover_device", "nh_cover_intervals_device")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    # nh_run_dust's argument list plus nh_host_intervals *
    assert len(_lib.SYMBOLS["nh_run_intervals"][1]) == len(_lib.SYMBOLS["nh_run_dust"][1]) + 1 == 12
    assert len(_lib.SYMBOLS["nh_run_engine_intervals"][1]) == len(_lib.SYMBOLS["nh_run_engine_dust"][1]) + 1 == 13
    assert _lib.SYMBOLS["nh_run_intervals"][1][:10] == _lib.SYMBOLS["nh_run_dust"][1][:10]
    assert len(_lib.SYMBOLS["nh_host_cover_device"][1]) == 10 and len(_lib.SYMBOLS["nh_cover_intervals_device"][1]) == 11
    assert C.sizeof(_lib.nh_host_intervals) == 40 and _lib.nh_host_intervals.path.offset == 8 and _lib.nh_host_intervals.fragments.offset == 16
    assert "} nh_host_intervals;" in hdr and "REVERSE COMPLEMENT" in hdr
    # no existing struct changed size
    assert C.sizeof(_lib.nh_run_extras) == 40 and C.sizeof(_lib.nh_minimizer_data) == 32 and C.sizeof(_lib.nh_host_filter) == 48
    assert C.sizeof(_lib.nh_read_dust) == 16


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


def _hi(path, size=None):
    from nohuman_amd import _lib
    return _lib.nh_host_intervals(C.sizeof(_lib.nh_host_intervals) if size is None else size, 0, path, 77, 78, 79)


def _both(files, x, rs, touts, n_touts, hi):
    """the two run entries with the same arguments -> their codes and messages"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    out = []
    out.append((L.nh_run_intervals(C.byref(_args(files)), x, 0, rs, None, touts, n_touts, None, None, None, hi, C.byref(s)), L.nh_last_error()))
    out.append((L.nh_run_engine_intervals(None, C.byref(_args(files)), x, 0, rs, None, touts, n_touts, None, None, None, hi, C.byref(s)), L.nh_last_error()))
    return out


def test_struct_too_small_is_refused_before_any_device(files):
    before = sorted(p.name for p in files.iterdir())
    for size in (0, 8, 39):
        for path in (None, str(files / "b.bed").encode()):
            hi = _hi(path, size)
            for rc, msg in _both(files, None, None, None, 0, C.byref(hi)):
                assert rc == NH_EINVAL and b"struct_size" in msg and b"nh_host_intervals" in msg, msg
            assert (hi.fragments, hi.intervals, hi.covered_bases) == (77, 78, 79)  # (a struct that small is not written to)
    assert sorted(p.name for p in files.iterdir()) == before  # no file created


def test_a_path_that_names_another_file_of_the_run_is_refused(files):
    from nohuman_amd import _lib
    before = sorted(p.name for p in files.iterdir())
    same = lambda name: str(files / name).encode()
    # in1, out1, -k, the report: through nh_run_args
    for name, word in (("a.fq", b"input"), ("o.fq", b"output"), ("k.txt", b"output"), ("r.txt", b"output")):
        hi = _hi(same(name))
        for rc, msg in _both(files, None, None, None, 0, C.byref(hi)):
            assert rc == NH_EINVAL and b"host intervals" in msg and word in msg and name.encode() in msg, msg
    # --calls and the human ids: through the extras
    x = _lib.nh_run_extras()
    x.struct_size = C.sizeof(_lib.nh_run_extras)
    x.calls, x.human_ids = same("c.tsv"), same("i.txt")
    for name in ("c.tsv", "i.txt"):
        for rc, msg in _both(files, C.byref(x), None, None, 0, C.byref(_hi(same(name)))):
            assert rc == NH_EINVAL and b"host intervals" in msg and name.encode() in msg, msg
    # the read statistics' table and a per-taxon file
    for rc, msg in _both(files, None, same("s.tsv"), None, 0, C.byref(_hi(same("s.tsv")))):
        assert rc == NH_EINVAL and b"host intervals" in msg and b"s.tsv" in msg, msg
    t = (_lib.nh_taxon_out * 1)()
    t[0].taxid, t[0].out1 = 9606, same("t.fq")
    for rc, msg in _both(files, None, None, t, 1, C.byref(_hi(same("t.fq")))):
        assert rc == NH_EINVAL and b"host intervals" in msg and b"t.fq" in msg, msg
    # an empty path
    for rc, msg in _both(files, None, None, None, 0, C.byref(_hi(b""))):
        assert rc == NH_EINVAL and b"empty path" in msg, msg
    assert sorted(p.name for p in files.iterdir()) == before  # nothing created


def test_null_goes_where_nh_run_dust_goes(files):
    """hi NULL, or its path NULL: nh_run_dust's checks in nh_run_dust's order, and its messages"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    for hi in (None, C.byref(_hi(None))):
        rd = _lib.nh_read_dust(8, 1, 0)
        assert L.nh_run_intervals(C.byref(_args(files)), None, 0, None, None, None, 0, None, None, C.byref(rd), hi, C.byref(s)) == NH_EINVAL
        a = L.nh_last_error()
        assert L.nh_run_dust(C.byref(_args(files)), None, 0, None, None, None, 0, None, None, C.byref(rd), C.byref(s)) == NH_EINVAL
        assert a == L.nh_last_error() and b"nh_read_dust" in a
        assert L.nh_run_intervals(C.byref(_args(files)), None, 94, None, None, None, 0, None, None, None, hi, C.byref(s)) == NH_EINVAL
        assert b"93" in L.nh_last_error()
        assert L.nh_run_engine_intervals(None, C.byref(_args(files)), None, 0, None, None, None, 0, None, None, None, hi, C.byref(s)) == NH_EINVAL
        a = L.nh_last_error()
        assert L.nh_run_engine_dust(None, C.byref(_args(files)), None, 0, None, None, None, 0, None, None, None, C.byref(s)) == NH_EINVAL
        assert a == L.nh_last_error() and b"null engine" in a
    # a good struct with a path: the engine entry's own refusal comes after the request's
    assert L.nh_run_engine_intervals(None, C.byref(_args(files)), None, 0, None, None, None, 0, None, None, None,
                                     C.byref(_hi(str(files / "b.bed").encode())), C.byref(s)) == NH_EINVAL
    assert b"null engine" in L.nh_last_error()
    assert L.nh_host_cover_device(None, None, 0, None, None, 0, None, 0, None, None) == NH_EINVAL
    assert L.nh_cover_intervals_device(None, None, 0, None, None, 0, None, 0, None, None, None) == NH_EINVAL
    assert not (files / "b.bed").exists() and not (files / "o.fq").exists()


def test_python_keywords():
    from nohuman_amd import Engine, engine
    from nohuman_amd.runner import CommandRunner
    for fn in (engine.run, Engine.run):
        p = inspect.signature(fn).parameters
        assert "host_intervals" in p and p["host_intervals"].default is None
    assert list(inspect.signature(Engine.host_cover_device).parameters)[1:] == [
        "d_text", "text_len", "d_seq_starts", "d_seq_lens", "n_seq", "d_cover", "d_host_of", "n_nodes", "stream"]
    assert list(inspect.signature(Engine.cover_intervals_device).parameters)[1:] == [
        "d_cover", "text_len", "d_seq_starts", "d_seq_lens", "n_seq", "d_intervals", "cap_records", "d_total", "d_error_bits", "stream"]
    o = CommandRunner.parse_argv(["--db", "d", "--host-intervals", "x.bed", "--unclassified-out", "o", "in.fq"])
    assert o["host_intervals"] == "x.bed" and o["inputs"] == ["in.fq"]
    assert CommandRunner.parse_argv(["--db", "d", "in.fq"])["host_intervals"] is None


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flag(files):
    r = _cli(["--help"])
    assert r.returncode == 0
    line = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--host-intervals")]
    assert len(line) == 1 and "BED" in line[0] and "reverse complement" in line[0]
    # without a value: an argument error
    r = _cli(["--db", DB, "-o", str(files / "o.fq"), str(files / "a.fq"), "--host-intervals"])
    assert r.returncode == 2 and "--host-intervals" in r.stderr and "dependencies" not in r.stderr, (r.returncode, r.stderr)
    # a file that is the input or another output: refused as an argument error, before the device probe
    for other in (str(files / "a.fq"), str(files / "o.fq")):
        r = _cli(["--db", DB, "-o", str(files / "o.fq"), "--host-intervals", other, str(files / "a.fq")])
        assert r.returncode == 2 and "--host-intervals" in r.stderr and "dependencies" not in r.stderr, (r.returncode, r.stderr)
    # beside --build-db
    (files / "g.fa").write_bytes(b">chr\n" + b"ACGT" * 30 + b"\n")
    r = _cli(["--build-db", str(files / "db"), "--reference", str(files / "g.fa"), "--host-intervals", str(files / "b.bed")])
    assert r.returncode == 2 and "--host-intervals" in r.stderr and "--build-db" in r.stderr, (r.returncode, r.stderr)
    assert not (files / "db").exists() and not (files / "o.fq").exists() and not (files / "b.bed").exists()
