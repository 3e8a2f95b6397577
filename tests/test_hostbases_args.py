"""--host-bases-only (nh_run_hostbases / nh_run_engine_hostbases, nh_cover_close_device, `--host-bases-only`, `--host-gap INT`): the
entries are declared, bound and exported; a struct too small, enable without a masked run and a gap above NH_HOST_GAP_MAX are
NH_EINVAL before a device is touched or a file created, through both entries and through run(); hb == NULL or enable == 0 goes where
nh_run_intervals goes; the CLI parses the flags.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1
GAP_MAX = 4096
ENTRIES = ("nh_run_hostbases", "nh_run_engine_hostbases", "nh_cover_close_device")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    assert "#define NH_HOST_GAP_MAX %d" % GAP_MAX in hdr and _lib.NH_HOST_GAP_MAX == GAP_MAX
    # nh_run_intervals' argument list plus nh_host_bases *
    assert len(_lib.SYMBOLS["nh_run_hostbases"][1]) == len(_lib.SYMBOLS["nh_run_intervals"][1]) + 1 == 13
    assert len(_lib.SYMBOLS["nh_run_engine_hostbases"][1]) == len(_lib.SYMBOLS["nh_run_engine_intervals"][1]) + 1 == 14
    assert _lib.SYMBOLS["nh_run_hostbases"][1][:11] == _lib.SYMBOLS["nh_run_intervals"][1][:11]
    assert len(_lib.SYMBOLS["nh_cover_close_device"][1]) == 9
    hb = _lib.nh_host_bases
    assert C.sizeof(hb) == 40 and (hb.enable.offset, hb.gap.offset, hb.reserved.offset, hb.host_bases.offset, hb.closed_bases.offset) == (4, 8, 12, 16, 32)
    assert "} nh_host_bases;" in hdr
    # no existing struct changed size
    assert C.sizeof(_lib.nh_run_extras) == 40 and C.sizeof(_lib.nh_host_intervals) == 40 and C.sizeof(_lib.nh_read_dust) == 16


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


def _extras(mask):
    from nohuman_amd import _lib
    x = _lib.nh_run_extras()
    x.struct_size = C.sizeof(_lib.nh_run_extras)
    x.mask = mask
    return x


def _hb(enable=1, gap=0, size=None):
    from nohuman_amd import _lib
    return _lib.nh_host_bases(C.sizeof(_lib.nh_host_bases) if size is None else size, enable, gap, 0, 77, 78, 79)


def _both(files, x, hi, hb, rd=None, minq=0, standalone=True):
    """the two run entries with the same arguments -> their codes and messages (standalone False: the engine entry's alone, twice --
    a request that passes its checks would open the database through the other)"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    out = []
    if standalone:
        out.append((L.nh_run_hostbases(C.byref(_args(files)), x, minq, None, None, None, 0, None, None, rd, hi, hb, C.byref(s)), L.nh_last_error()))
    out.append((L.nh_run_engine_hostbases(None, C.byref(_args(files)), x, minq, None, None, None, 0, None, None, rd, hi, hb, C.byref(s)), L.nh_last_error()))
    return out if standalone else out * 2


def test_struct_too_small_is_refused_before_any_device(files):
    before = sorted(p.name for p in files.iterdir())
    for size in (0, 8, 39):
        for enable in (0, 1):
            hb = _hb(enable, 0, size)
            for rc, msg in _both(files, C.byref(_extras(1)), None, C.byref(hb)):
                assert rc == NH_EINVAL and b"struct_size" in msg and b"nh_host_bases" in msg, msg
            assert (hb.host_bases, hb.masked_bases, hb.closed_bases) == (77, 78, 79)  # (a struct that small is not written to)
    assert sorted(p.name for p in files.iterdir()) == before


def test_enable_without_a_masked_run_is_refused(files):
    before = sorted(p.name for p in files.iterdir())
    for x in (None, C.byref(_extras(0))):
        for rc, msg in _both(files, x, None, C.byref(_hb(1, 34))):
            assert rc == NH_EINVAL and b"nh_run_hostbases" in msg and b"mask" in msg, msg
    assert sorted(p.name for p in files.iterdir()) == before


def test_a_gap_above_the_cap_is_refused(files):
    before = sorted(p.name for p in files.iterdir())
    for gap in (GAP_MAX + 1, 2 ** 32 - 1):
        for rc, msg in _both(files, C.byref(_extras(1)), None, C.byref(_hb(1, gap))):
            assert rc == NH_EINVAL and b"NH_HOST_GAP_MAX" in msg and str(gap).encode() in msg, msg
    # the cap itself passes the request's checks: the engine entry's own refusal comes after them
    rc, msg = _both(files, C.byref(_extras(1)), None, C.byref(_hb(1, GAP_MAX)), standalone=False)[1]
    assert rc == NH_EINVAL and b"null engine" in msg
    # not enabled: the gap is not looked at
    rc, msg = _both(files, C.byref(_extras(1)), None, C.byref(_hb(0, GAP_MAX + 1)), standalone=False)[1]
    assert rc == NH_EINVAL and b"null engine" in msg
    assert sorted(p.name for p in files.iterdir()) == before


def test_null_or_not_enabled_goes_where_nh_run_intervals_goes(files):
    """the refusals the two entries share, in nh_run_intervals' order and with its messages"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    small_hi = _lib.nh_host_intervals(8, 0, None, 0, 0, 0)
    same_hi = _lib.nh_host_intervals(C.sizeof(_lib.nh_host_intervals), 0, str(files / "o.fq").encode(), 0, 0, 0)
    small_rd = _lib.nh_read_dust(8, 1, 0)
    cases = [dict(hi=C.byref(small_hi)), dict(hi=C.byref(same_hi)), dict(rd=C.byref(small_rd)), dict(minq=94), dict()]
    for hb in (None, C.byref(_hb(0, 5))):
        for kw in cases:
            got = _both(files, None, kw.get("hi"), hb, kw.get("rd"), kw.get("minq", 0), standalone=bool(kw))
            a = _args(files)
            rc0 = m0 = None
            if kw:
                rc0 = L.nh_run_intervals(C.byref(a), None, kw.get("minq", 0), None, None, None, 0, None, None, kw.get("rd"), kw.get("hi"), C.byref(s))
                m0 = L.nh_last_error()
            rc1 = L.nh_run_engine_intervals(None, C.byref(a), None, kw.get("minq", 0), None, None, None, 0, None, None, kw.get("rd"), kw.get("hi"), C.byref(s))
            m1 = L.nh_last_error()
            if kw:  # (the case without a refusal of the request would open the database through the standalone entry)
                assert got[0] == (rc0, m0) and rc0 == NH_EINVAL, (kw, got[0], m0)
            assert got[1] == (rc1, m1) and rc1 == NH_EINVAL, (kw, got[1], m1)
    assert L.nh_cover_close_device(None, None, 0, None, None, 0, 0, None, None) == NH_EINVAL
    assert not (files / "o.fq").exists()


def test_run_refuses_through_the_python_entries(files):
    from nohuman_amd import EngineError, engine
    before = sorted(p.name for p in files.iterdir())
    kw = dict(kraken_output=str(files / "k.txt"))
    with pytest.raises(EngineError) as ei:  # host_bases_only implies mask: the library sees the gap
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), host_bases_only=True, host_gap=GAP_MAX + 1, **kw)
    assert ei.value.code == NH_EINVAL and "NH_HOST_GAP_MAX" in ei.value.message
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), host_gap=34, **kw)
    assert ei.value.code == NH_EINVAL and "host_bases_only" in ei.value.message
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), host_bases_only=True, host_gap=-1, **kw)
    assert ei.value.code == NH_EINVAL
    with pytest.raises(EngineError) as ei:  # a masked run's own refusal
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), host_bases_only=True, keep_human=True, **kw)
    assert ei.value.code == NH_EINVAL and "keep_human" in ei.value.message
    assert sorted(p.name for p in files.iterdir()) == before


def test_python_keywords():
    from nohuman_amd import Engine, engine
    for fn in (engine.run, Engine.run):
        p = inspect.signature(fn).parameters
        assert p["host_bases_only"].default is False and p["host_gap"].default == 0
    assert list(inspect.signature(Engine.cover_close_device).parameters)[1:] == [
        "d_cover", "text_len", "d_seq_starts", "d_seq_lens", "n_seq", "gap", "d_closed_bases", "stream"]


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flags(files):
    r = _cli(["--help"])
    assert r.returncode == 0
    for flag, word in (("--host-bases-only", "a masked run"), ("--host-gap", "34")):
        line = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith(flag)]
        assert len(line) == 1 and word in line[0] and "--mask" not in line[0], line
    assert sum("--mask" in ln for ln in r.stdout.splitlines()) == 1
    base = ["--db", DB, "-o", str(files / "o.fq"), str(files / "a.fq")]
    # with -H: as the masked run's own flag
    r = _cli(base + ["--host-bases-only", "-H"])
    assert r.returncode == 2 and "--host-bases-only" in r.stderr and "--human" in r.stderr and "dependencies" not in r.stderr, r.stderr
    # the gap needs the mode, a value, and a number in 0..4096
    r = _cli(base + ["--host-gap", "34"])
    assert r.returncode == 2 and "--host-gap" in r.stderr and "--host-bases-only" in r.stderr, r.stderr
    r = _cli(base + ["--host-bases-only", "--host-gap"])
    assert r.returncode == 2 and "--host-gap" in r.stderr, r.stderr
    for bad in ("4097", "-1", "x", "3x", ""):
        r = _cli(base + ["--host-bases-only", "--host-gap", bad])
        assert r.returncode == 2 and "--host-gap" in r.stderr and "dependencies" not in r.stderr, (bad, r.stderr)
    # beside --build-db
    (files / "g.fa").write_bytes(b">chr\n" + b"ACGT" * 30 + b"\n")
    for extra in (["--host-bases-only"], ["--host-bases-only", "--host-gap", "34"]):
        r = _cli(["--build-db", str(files / "db"), "--reference", str(files / "g.fa")] + extra)
        assert r.returncode == 2 and "--host-bases-only" in r.stderr and "--build-db" in r.stderr, (r.returncode, r.stderr)
    assert not (files / "db").exists() and not (files / "o.fq").exists()
