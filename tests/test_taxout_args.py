"""Per-taxon outputs (nh_run_taxa / nh_run_engine_taxa, `--taxon-out`): the entries are declared, bound and exported; every
argument the header calls NH_EINVAL is refused before a device is touched or a file created, with the offending field in the
message; n_outs = 0 runs nh_run_rstats' checks; the CLI's usage errors exit with 2 and leave nothing on disk.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1


def test_entries_are_declared_bound_and_exported():
    import nohuman_amd
    from nohuman_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ("nh_run_taxa", "nh_run_engine_taxa"):
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert len(_lib.SYMBOLS["nh_run_taxa"][1]) == 8 and len(_lib.SYMBOLS["nh_run_engine_taxa"][1]) == 9
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    assert "#define NH_MAX_TAXON_OUTS 8" in hdr and _lib.NH_MAX_TAXON_OUTS == 8
    assert "#define NH_TAXON_OTHER 0u" in hdr and _lib.NH_TAXON_OTHER == 0
    assert C.sizeof(_lib.nh_taxon_out) == 32
    assert C.sizeof(_lib.nh_run_extras) == 40 and C.sizeof(_lib.nh_run_args) == 96  # the structs callers pass keep their sizes
    for fn in (engine.run, nohuman_amd.Engine.run):
        assert "taxon_outs" in inspect.signature(fn).parameters


@pytest.fixture
def files(tmp_path):
    (tmp_path / "a.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (tmp_path / "b.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    return tmp_path


def _args(d, paired=False, keep_human=0):
    from nohuman_amd import _lib
    a = _lib.nh_run_args()
    a.db_dir = DB.encode()
    a.in1 = str(d / "a.fq").encode()
    a.out1 = str(d / "o.fq").encode()
    if paired:
        a.in2 = str(d / "b.fq").encode()
        a.out2 = str(d / "o2.fq").encode()
    a.kraken_output = str(d / "k.txt").encode()
    a.report = str(d / "r.txt").encode()
    a.keep_human = keep_human
    return a


def _outs(d, sel):
    """[(taxid, out1 name or None, out2 name or None), ...] -> the C array"""
    from nohuman_amd import _lib
    t = (_lib.nh_taxon_out * max(1, len(sel)))()
    for x, (taxid, o1, o2) in zip(t, sel):
        x.taxid = taxid
        x.out1 = str(d / o1).encode() if o1 is not None else None
        x.out2 = str(d / o2).encode() if o2 is not None else None
    return t


def _both(L, a, x, minq, rs, t, n):
    """the call through both entries: the same refusal; returns the message"""
    from nohuman_amd import _lib
    s = _lib.nh_stats()
    xr = C.byref(x) if x is not None else None
    assert L.nh_run_taxa(C.byref(a), xr, minq, rs, None, t, n, C.byref(s)) == NH_EINVAL, L.nh_last_error()
    msg = L.nh_last_error()
    assert L.nh_run_engine_taxa(None, C.byref(a), xr, minq, rs, None, t, n, C.byref(s)) == NH_EINVAL
    assert L.nh_last_error() == msg
    return msg


def test_selector_lists_that_are_refused(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    before = sorted(p.name for p in files.iterdir())
    nine = [(10 + i, "t%d.fq" % i, None) for i in range(9)]
    assert b"n_outs 9" in _both(L, _args(files), None, 0, None, _outs(files, nine), 9)
    assert b"outs is NULL" in _both(L, _args(files), None, 0, None, None, 1)
    assert b"outs[1].taxid 10 is given twice" in _both(L, _args(files), None, 0, None, _outs(files, [(10, "t0.fq", None), (10, "t1.fq", None)]), 2)
    msg = _both(L, _args(files), None, 0, None, _outs(files, [(0, "t0.fq", None), (11, "t1.fq", None), (0, "t2.fq", None)]), 3)
    assert b"outs[2].taxid" in msg and b"other" in msg
    assert b"outs[0].out1 is required" in _both(L, _args(files), None, 0, None, _outs(files, [(10, None, None)]), 1)
    assert b"outs[1].out2 is given without in2" in _both(L, _args(files), None, 0, None, _outs(files, [(10, "t0.fq", None), (11, "t1.fq", "t1b.fq")]), 2)
    assert b"paired input needs outs[0].out2" in _both(L, _args(files, paired=True), None, 0, None, _outs(files, [(10, "t0.fq", None)]), 1)
    assert b"keep_human" in _both(L, _args(files, keep_human=1), None, 0, None, _outs(files, [(10, "t0.fq", None)]), 1)
    assert sorted(p.name for p in files.iterdir()) == before  # no file created


def test_root_and_eight_selectors_pass_the_checks(files):
    """taxid 1 is a selector like any other, and eight are allowed: the next refusal is the null engine's"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    eight = [(1, "t0.fq", None), (0, "t1.fq", None)] + [(10 + i, "t%d.fq" % (2 + i), None) for i in range(6)]
    assert L.nh_run_engine_taxa(None, C.byref(_args(files)), None, 0, None, None, _outs(files, eight), 8, C.byref(s)) == NH_EINVAL
    assert b"null engine" in L.nh_last_error()
    assert not (files / "t0.fq").exists() and not (files / "o.fq").exists()


def test_paths_that_name_another_file_of_the_run(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), human_out1=str(files / "h1.fq").encode(),
                           human_out2=str(files / "h2.fq").encode(), calls=str(files / "c.txt").encode(),
                           human_ids=str(files / "i.txt").encode())
    rs = str(files / "s.tsv").encode()
    os.link(files / "b.fq", files / "same_inode.fq")  # an input under another name
    before = sorted(p.name for p in files.iterdir())
    for name, role in (("a.fq", "input"), ("b.fq", "input"), ("same_inode.fq", "input"), ("o.fq", "output"), ("o2.fq", "output"),
                       ("h1.fq", "output"), ("h2.fq", "output"), ("k.txt", "output"), ("r.txt", "output"), ("c.txt", "output"),
                       ("i.txt", "output"), ("s.tsv", "output")):
        for mate in (1, 2):
            sel = [(10, "t0_1.fq", "t0_2.fq"), (0, name if mate == 1 else "t1_1.fq", name if mate == 2 else "t1_2.fq")]
            msg = _both(L, _args(files, paired=True), x, 0, rs, _outs(files, sel), 2)
            assert ("outs[1].out%d" % mate).encode() in msg and str(files / name).encode() in msg and role.encode() in msg, msg
    # another selector's file, and a selector's own other mate
    msg = _both(L, _args(files, paired=True), x, 0, rs, _outs(files, [(10, "t0_1.fq", "t0_2.fq"), (0, "t1_1.fq", "t0_1.fq")]), 2)
    assert b"outs[1].out2" in msg and b"outs[0].out1" in msg
    msg = _both(L, _args(files, paired=True), x, 0, rs, _outs(files, [(10, "t0_1.fq", "t0_1.fq")]), 1)
    assert b"outs[0].out2" in msg and b"outs[0].out1" in msg
    assert sorted(p.name for p in files.iterdir()) == before  # no file created


def test_the_shared_arguments_are_checked_as_by_nh_run_rstats(files):
    """n_outs = 0 is nh_run_rstats: the same refusals with the same messages; and they come first with selectors"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode())
    t = _outs(files, [(10, "t0.fq", None)])
    for n in (0, 1):
        for extras in (None, C.byref(x)):
            assert L.nh_run_rstats(C.byref(_args(files)), extras, 94, None, None, C.byref(s)) == NH_EINVAL
            want = L.nh_last_error()
            assert b"93" in want
            assert L.nh_run_taxa(C.byref(_args(files)), extras, 94, None, None, t, n, C.byref(s)) == NH_EINVAL
            assert L.nh_last_error() == want
        assert L.nh_run_rstats(C.byref(_args(files)), C.byref(x), 0, x.calls, None, C.byref(s)) == NH_EINVAL
        want = L.nh_last_error()
        assert L.nh_run_taxa(C.byref(_args(files)), C.byref(x), 0, x.calls, None, t, n, C.byref(s)) == NH_EINVAL
        assert L.nh_last_error() == want and b"read statistics" in want
    x.struct_size -= 1
    assert L.nh_run_taxa(C.byref(_args(files)), C.byref(x), 0, None, None, t, 1, C.byref(s)) == NH_EINVAL and b"struct_size" in L.nh_last_error()
    assert L.nh_run_engine_taxa(None, C.byref(_args(files)), None, 0, None, None, None, 0, C.byref(s)) == NH_EINVAL and b"null engine" in L.nh_last_error()
    assert not (files / "o.fq").exists() and not (files / "t0.fq").exists()


def test_python_selectors(files):
    from nohuman_amd import engine
    with pytest.raises(engine.EngineError, match="taxid or"):
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), taxon_outs=[("human", str(files / "t.fq"), None)])
    with pytest.raises(engine.EngineError, match="given twice"):
        engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), taxon_outs=[("other", str(files / "t.fq"), None), ("other", str(files / "u.fq"), None)])
    assert sorted(p.name for p in files.iterdir()) == ["a.fq", "b.fq"]


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_usage_errors(files):
    a, b = str(files / "a.fq"), str(files / "b.fq")
    t = str(files / "t.fq")
    env = dict(os.environ)
    env.pop("NOHUMAN_DB", None)
    before = sorted(p.name for p in files.iterdir())
    eight = [x for i in range(8) for x in ("--taxon-out", "%d:%s" % (10 + i, str(files / ("t%d.fq" % i))))]
    cases = [
        ([a, "--taxon-out", t], "':'"),
        ([a, "--taxon-out", "human:" + t], "neither a taxid"),
        ([a, "--taxon-out", "-5:" + t], "neither a taxid"),
        ([a] + eight + ["--taxon-out", "other:" + t], "more than 8 times"),
        ([a, "--taxon-out", "10:" + t, "--taxon-out", "10:" + t + "2"], "more than once"),
        ([a, "--taxon-out", "other:" + t, "--taxon-out", "other:" + t + "2"], "more than once"),
        ([a, b, "--taxon-out", "10:" + t], "'#'"),
        ([a, "--taxon-out", "10:" + str(files / "t#.fq")], "two inputs"),
        ([a, "-H", "--taxon-out", "10:" + t], "--human"),
        (["--build-db", str(files / "db"), "--reference", a, "--taxon-out", "10:" + t], "--build-db"),
        ([a, "-o", t, "--taxon-out", "10:" + t], "--out1"),
        ([a, b, "-o", str(files / "x_1.fq"), "-O", str(files / "x_2.fq"), "--taxon-out", "10:" + str(files / "x#.fq")], "--out1"),
        ([a, "--human-out1", t, "--taxon-out", "10:" + t], "--human-out1"),
        ([a, "--calls", t, "--taxon-out", "10:" + t], "--calls"),
        ([a, "--human-ids", t, "--taxon-out", "10:" + t], "--human-ids"),
        ([a, "--read-stats", t, "--taxon-out", "10:" + t], "--read-stats"),
        ([a, "-k", t, "--taxon-out", "10:" + t], "--kraken-output"),
        ([a, "-r", t, "--taxon-out", "10:" + t], "--kraken-report"),
        ([a, "--taxon-out", "10:" + t, "--taxon-out", "other:" + t], "twice"),
        ([a, "--taxon-out", "10:" + a], "input"),
        ([a, "--taxon-out", "10:" + str(files / "a.nohuman.fq")], "same file as the output"),  # the DEFAULT output name
    ]
    for argv, what in cases:
        r = subprocess.run([BIN, "--db", DB] + argv, env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (argv, r.returncode, r.stderr[-500:])
        assert r.stderr.startswith("error: ") and what in r.stderr and "--help" in r.stderr, (argv, r.stderr)
        assert sorted(p.name for p in files.iterdir()) == before, argv
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--taxon-out <TAXID|other>:<PATH>" in r.stdout
