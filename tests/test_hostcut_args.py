"""--host-cut (nh_run_hostcut / nh_run_engine_hostcut, nh_host_cut_device, `--host-cut`, `--host-min-piece INT`): the entries are
declared, bound and exported; a struct too small, enable without a masked run, enable beside an enabled nh_host_bases, a gap above
NH_HOST_GAP_MAX, min_piece 0 and paired input are NH_EINVAL before a device is touched or a file created, through both entries,
through run() and through the CLI; hc == NULL or enable == 0 goes where nh_run_hostbases goes.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

from tests import bam_model as bm
from tests import bam_pair_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1
GAP_MAX = 4096
ENTRIES = ("nh_run_hostcut", "nh_run_engine_hostcut", "nh_host_cut_device")
COUNTS = ("host_bases", "pieces", "piece_bases", "cut_bases", "short_bases", "dropped_reads", "closed_bases")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    # nh_run_hostbases' argument list plus nh_host_cut *
    assert len(_lib.SYMBOLS["nh_run_hostcut"][1]) == len(_lib.SYMBOLS["nh_run_hostbases"][1]) + 1 == 14
    assert len(_lib.SYMBOLS["nh_run_engine_hostcut"][1]) == len(_lib.SYMBOLS["nh_run_engine_hostbases"][1]) + 1 == 15
    assert _lib.SYMBOLS["nh_run_hostcut"][1][:12] == _lib.SYMBOLS["nh_run_hostbases"][1][:12]
    assert len(_lib.SYMBOLS["nh_host_cut_device"][1]) == 18
    hc = _lib.nh_host_cut
    assert "} nh_host_cut;" in hdr and C.sizeof(hc) == 72
    assert (hc.enable.offset, hc.gap.offset, hc.min_piece.offset) == (4, 8, 12)
    assert [getattr(hc, k).offset for k in COUNTS] == [16, 24, 32, 40, 48, 56, 64]
    assert _lib.HOST_CUT_COUNTS == COUNTS[:6]
    # the fields in the header, in the struct's order
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} nh_host_cut;")):hdr.index("} nh_host_cut;")]
    at = [body.index(" " + k + ";") for k in ("struct_size", "enable", "gap", "min_piece") + COUNTS]
    assert at == sorted(at)
    # no existing struct changed size
    assert C.sizeof(_lib.nh_run_extras) == 40 and C.sizeof(_lib.nh_host_intervals) == 40 and C.sizeof(_lib.nh_read_dust) == 16
    assert C.sizeof(_lib.nh_host_bases) == 40


@pytest.fixture
def files(tmp_path):
    (tmp_path / "a.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "b.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    pair = b"".join(pm.forge_pair(b"p1", b"ACGTACGT", b"TTGCA", bytes(8), bytes(5), rev=(0, 1)))
    (tmp_path / "pairs.bam").write_bytes(bm.bgzf(bm.forge_header() + pair))
    return tmp_path


def _args(d, in1="a.fq", in2=None):
    from nohuman_amd import _lib
    a = _lib.nh_run_args()
    a.db_dir = DB.encode()
    a.in1 = str(d / in1).encode()
    a.out1 = str(d / "o.fq").encode()
    if in2:
        a.in2 = str(d / in2).encode()
    if in2 or in1.endswith("pairs.bam"):
        a.out2 = str(d / "o2.fq").encode()
    a.kraken_output = str(d / "k.txt").encode()
    a.report = str(d / "r.txt").encode()
    return a


def _extras(mask):
    from nohuman_amd import _lib
    x = _lib.nh_run_extras()
    x.struct_size = C.sizeof(_lib.nh_run_extras)
    x.mask = mask
    return x


def _hc(enable=1, gap=0, min_piece=35, size=None):
    from nohuman_amd import _lib
    return _lib.nh_host_cut(C.sizeof(_lib.nh_host_cut) if size is None else size, enable, gap, min_piece, 71, 72, 73, 74, 75, 76, 77)


def _hb(enable=1, gap=0):
    from nohuman_amd import _lib
    return _lib.nh_host_bases(C.sizeof(_lib.nh_host_bases), enable, gap, 0, 0, 0, 0)


def _both(files, x, hc, hb=None, hi=None, rd=None, minq=0, standalone=True, **inputs):
    """the two run entries with the same arguments -> their codes and messages (standalone False: the engine entry's alone, twice --
    a request that passes its checks would open the database through the other)"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    out = []
    if standalone:
        out.append((L.nh_run_hostcut(C.byref(_args(files, **inputs)), x, minq, None, None, None, 0, None, None, rd, hi, hb, hc, C.byref(s)), L.nh_last_error()))
    out.append((L.nh_run_engine_hostcut(None, C.byref(_args(files, **inputs)), x, minq, None, None, None, 0, None, None, rd, hi, hb, hc, C.byref(s)),
                L.nh_last_error()))
    return out if standalone else out * 2


def _names(files):
    return sorted(p.name for p in files.iterdir())


def test_struct_too_small_is_refused_before_any_device(files):
    before = _names(files)
    for size in (0, 8, 40, 71):
        for enable in (0, 1):
            hc = _hc(enable, 0, 35, size)
            for rc, msg in _both(files, C.byref(_extras(1)), C.byref(hc)):
                assert rc == NH_EINVAL and b"struct_size" in msg and b"nh_host_cut" in msg, msg
            assert [getattr(hc, k) for k in COUNTS] == [71, 72, 73, 74, 75, 76, 77]  # (a struct that small is not written to)
    assert _names(files) == before


def test_enable_without_a_masked_run_is_refused(files):
    before = _names(files)
    for x in (None, C.byref(_extras(0))):
        for rc, msg in _both(files, x, C.byref(_hc(1, 34))):
            assert rc == NH_EINVAL and b"nh_run_hostcut" in msg and b"mask" in msg, msg
    assert _names(files) == before


def test_enable_beside_an_enabled_host_bases_is_refused(files):
    before = _names(files)
    for rc, msg in _both(files, C.byref(_extras(1)), C.byref(_hc(1, 34)), hb=C.byref(_hb(1, 34))):
        assert rc == NH_EINVAL and b"nh_run_hostcut" in msg and b"nh_host_bases" in msg, msg
    # a host-bases struct that is not enabled is no obstacle: the request passes its checks
    rc, msg = _both(files, C.byref(_extras(1)), C.byref(_hc(1, 34)), hb=C.byref(_hb(0, 34)), standalone=False)[1]
    assert rc == NH_EINVAL and b"null engine" in msg
    assert _names(files) == before


def test_a_gap_above_the_cap_and_a_min_piece_of_zero_are_refused(files):
    before = _names(files)
    for gap in (GAP_MAX + 1, 2 ** 32 - 1):
        for rc, msg in _both(files, C.byref(_extras(1)), C.byref(_hc(1, gap))):
            assert rc == NH_EINVAL and b"nh_run_hostcut" in msg and b"NH_HOST_GAP_MAX" in msg and str(gap).encode() in msg, msg
    for m in (0, 2 ** 31, 2 ** 32 - 1):
        for rc, msg in _both(files, C.byref(_extras(1)), C.byref(_hc(1, 34, m))):
            assert rc == NH_EINVAL and b"nh_run_hostcut" in msg and b"min_piece" in msg and str(m).encode() in msg, msg
    # the caps themselves pass the request's checks: the engine entry's own refusal comes after them
    for m in (1, 2 ** 31 - 1):
        rc, msg = _both(files, C.byref(_extras(1)), C.byref(_hc(1, GAP_MAX, m)), standalone=False)[1]
        assert rc == NH_EINVAL and b"null engine" in msg
    # not enabled: neither is looked at
    rc, msg = _both(files, C.byref(_extras(1)), C.byref(_hc(0, GAP_MAX + 1, 0)), standalone=False)[1]
    assert rc == NH_EINVAL and b"null engine" in msg
    assert _names(files) == before


def test_paired_input_is_refused_and_the_reason_named(files):
    before = _names(files)
    for inputs, word in ((dict(in2="b.fq"), b"in2 is given"), (dict(in1="pairs.bam"), b"paired BAM")):
        for rc, msg in _both(files, C.byref(_extras(1)), C.byref(_hc(1, 34)), **inputs):
            assert rc == NH_EINVAL and b"nh_run_hostcut" in msg and b"single-end" in msg and word in msg, msg
    assert _names(files) == before


def test_null_or_not_enabled_goes_where_nh_run_hostbases_goes(files):
    """the refusals the entries share, in nh_run_hostbases' order and with its messages"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    small_hi = _lib.nh_host_intervals(8, 0, None, 0, 0, 0)
    small_rd = _lib.nh_read_dust(8, 1, 0)
    small_hb = _lib.nh_host_bases(8, 1, 0, 0, 0, 0, 0)
    cases = [dict(hi=C.byref(small_hi)), dict(rd=C.byref(small_rd)), dict(minq=94), dict(hb=C.byref(small_hb)), dict(hb=C.byref(_hb(1, GAP_MAX + 1)), x=1),
             dict(hb=C.byref(_hb(1, 3))), dict()]
    for hc in (None, C.byref(_hc(0, 5, 0))):
        for kw in cases:
            x = C.byref(_extras(1)) if kw.get("x") else None
            refused = bool(kw)  # (the case without a refusal of the request would open the database through the standalone entry)
            got = _both(files, x, hc, kw.get("hb"), kw.get("hi"), kw.get("rd"), kw.get("minq", 0), standalone=refused)
            a = _args(files)
            if refused:
                rc0 = L.nh_run_hostbases(C.byref(a), x, kw.get("minq", 0), None, None, None, 0, None, None, kw.get("rd"), kw.get("hi"), kw.get("hb"), C.byref(s))
                m0 = L.nh_last_error()
                assert got[0] == (rc0, m0) and rc0 == NH_EINVAL, (kw, got[0], m0)
            rc1 = L.nh_run_engine_hostbases(None, C.byref(a), x, kw.get("minq", 0), None, None, None, 0, None, None, kw.get("rd"), kw.get("hi"), kw.get("hb"),
                                            C.byref(s))
            m1 = L.nh_last_error()
            assert got[1] == (rc1, m1) and rc1 == NH_EINVAL, (kw, got[1], m1)
    assert not (files / "o.fq").exists()


def test_the_device_entry_refuses_bad_arguments():
    from nohuman_amd import _lib
    L = _lib.lib()
    assert L.nh_host_cut_device(None, None, 0, None, None, None, None, None, 0, 1, None, 35, None, 0, None, None, None, None) == NH_EINVAL
    assert b"nh_host_cut_device" in L.nh_last_error()


def test_run_refuses_through_the_python_entries(files):
    from nohuman_amd import EngineError, engine
    before = _names(files)
    a, o = str(files / "a.fq"), str(files / "o.fq")
    kw = dict(kraken_output=str(files / "k.txt"))

    def refused(*words, **more):
        with pytest.raises(EngineError) as ei:
            engine.run(DB, a, o, **dict(kw, **more))
        assert ei.value.code == NH_EINVAL, ei.value.message
        for w in words:
            assert w in ei.value.message, ei.value.message

    refused("NH_HOST_GAP_MAX", host_cut=True, host_gap=GAP_MAX + 1)  # host_cut implies mask: the library sees the gap
    refused("host_min_piece", host_cut=True, host_min_piece=0)
    refused("host_min_piece", host_cut=True, host_min_piece=2 ** 31)
    refused("host_min_piece", "host_cut", host_min_piece=40)
    refused("host_bases_only", host_gap=34)  # (today's message)
    refused("nh_host_bases", host_cut=True, host_bases_only=True)
    refused("single-end", host_cut=True, in2=str(files / "b.fq"), out2=str(files / "o2.fq"))
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "pairs.bam"), o, out2=str(files / "o2.fq"), host_cut=True, **kw)
    assert ei.value.code == NH_EINVAL and "single-end" in ei.value.message and "paired BAM" in ei.value.message
    refused("keep_human", host_cut=True, keep_human=True)  # a masked run's own refusal
    assert _names(files) == before


def test_python_keywords():
    from nohuman_amd import Engine, engine
    for fn in (engine.run, Engine.run):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters
        assert names[-3:] == ["host_gap", "host_cut", "host_min_piece"]
        assert p["host_cut"].default is False and p["host_min_piece"].default == 35
    assert list(inspect.signature(Engine.host_cut_device).parameters)[1:] == [
        "d_text", "text_len", "d_records", "d_seq_starts", "d_seq_lens", "d_idlen", "d_results", "n", "fastq", "d_cover", "min_piece",
        "d_out", "cap", "d_total", "d_error_bits", "d_counts", "stream"]


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flags(files):
    r = _cli(["--help"])
    assert r.returncode == 0
    for flag, word in (("--host-cut", "a masked run"), ("--host-min-piece", "35")):
        line = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith(flag)]
        assert len(line) == 1 and word in line[0] and "--mask" not in line[0], line
    assert sum("--mask" in ln for ln in r.stdout.splitlines()) == 1
    base = ["--db", DB, "-o", str(files / "o.fq"), str(files / "a.fq")]
    for extra, words in ((["--host-cut", "-H"], ("--host-cut", "--human")),
                         (["--host-cut", "--host-bases-only"], ("--host-cut", "--host-bases-only")),
                         (["--host-min-piece", "40"], ("--host-min-piece", "--host-cut")),
                         (["--host-gap", "34"], ("--host-gap", "--host-bases-only")),
                         (["--host-cut", "--host-min-piece"], ("--host-min-piece",)),
                         (["--host-cut", "--host-gap", "4097"], ("--host-gap",))):
        r = _cli(base + extra)
        assert r.returncode == 2 and all(w in r.stderr for w in words) and "dependencies" not in r.stderr, (extra, r.stderr)
    for bad in ("0", "-1", "2147483648", "x", "3x", ""):
        r = _cli(base + ["--host-cut", "--host-min-piece", bad])
        assert r.returncode == 2 and "--host-min-piece" in r.stderr and "dependencies" not in r.stderr, (bad, r.stderr)
    # two inputs
    r = _cli(["--db", DB, "-o", str(files / "o.fq"), "-O", str(files / "o2.fq"), "--host-cut", str(files / "a.fq"), str(files / "b.fq")])
    assert r.returncode == 2 and "--host-cut" in r.stderr and "two inputs" in r.stderr, r.stderr
    # beside --build-db
    (files / "g.fa").write_bytes(b">chr\n" + b"ACGT" * 30 + b"\n")
    for extra, word in ((["--host-cut"], "--host-cut"), (["--host-min-piece", "40"], "--host-min-piece")):
        r = _cli(["--build-db", str(files / "db"), "--reference", str(files / "g.fa")] + extra)
        assert r.returncode == 2 and word in r.stderr and "--build-db" in r.stderr, (r.returncode, r.stderr)
    assert not (files / "db").exists() and not (files / "o.fq").exists() and not (files / "o2.fq").exists()
