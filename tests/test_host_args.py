"""The host selection (nh_run_host / nh_run_engine_host, nh_host_table_image, nh_host_filter_device, `--host-taxid`,
`--keep-taxid`): the entries are declared, bound and exported; nh_host_filter has its size and no struct of an existing caller
changed; every argument error is NH_EINVAL before a device is touched or a file created; the CLI, the Python keywords and the runner
mirror carry the flags; the host-node table of a taxo.k2d image equals the model's byte for byte.  No GPU needed."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from oracle import minidb
from tests import host_model as hm
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL, NH_EDB = -1, -3
ENTRIES = ("nh_run_host", "nh_run_engine_host", "nh_host_table_image", "nh_host_filter_device")


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert "int " + name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5
    assert "#define NH_MAX_HOST_TAXA 16" in hdr and _lib.NH_MAX_HOST_TAXA == 16
    assert len(_lib.SYMBOLS["nh_run_host"][1]) == len(_lib.SYMBOLS["nh_run_mdata"][1]) + 1
    assert len(_lib.SYMBOLS["nh_run_engine_host"][1]) == len(_lib.SYMBOLS["nh_run_engine_mdata"][1]) + 1
    assert len(_lib.SYMBOLS["nh_host_table_image"][1]) == 6 and len(_lib.SYMBOLS["nh_host_filter_device"][1]) == 8


def test_struct_sizes():
    from nohuman_amd import _lib
    assert C.sizeof(_lib.nh_host_filter) == 4 * 4 + 2 * 8 + 2 * 8 == 48
    assert (_lib.nh_host_filter.n_host.offset, _lib.nh_host_filter.n_keep.offset) == (4, 8)
    assert (_lib.nh_host_filter.host_taxids.offset, _lib.nh_host_filter.keep_taxids.offset) == (16, 24)
    assert (_lib.nh_host_filter.host_fragments.offset, _lib.nh_host_filter.spared_fragments.offset) == (32, 40)
    # the structs that existing callers pass keep their sizes
    assert C.sizeof(_lib.nh_run_args) == 96 and C.sizeof(_lib.nh_run_extras) == 40 and C.sizeof(_lib.nh_result) == 16
    assert C.sizeof(_lib.nh_stats) == 48 and C.sizeof(_lib.nh_taxon_out) == 32 and C.sizeof(_lib.nh_minimizer_data) == 32


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


def _hf(host=(), keep=(), size=None, null_host=False, null_keep=False):
    from nohuman_amd import _lib
    hf = _lib.nh_host_filter()
    hf.struct_size = C.sizeof(_lib.nh_host_filter) if size is None else size
    hf._h = (C.c_uint64 * max(len(host), 1))(*host)
    hf._k = (C.c_uint64 * max(len(keep), 1))(*keep)
    hf.n_host, hf.n_keep = len(host), len(keep)
    if not null_host:
        hf.host_taxids = hf._h
    if not null_keep:
        hf.keep_taxids = hf._k
    return hf


def _both(a, x, md, hf, minq=0):
    """the two run entries (the engine one without an engine) -> their common (code, message)"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    got = []
    for engine in (False, True):
        pre = (None,) if engine else ()
        fn = L.nh_run_engine_host if engine else L.nh_run_host
        rc = fn(*pre, C.byref(a), C.byref(x) if x is not None else None, minq, None, None, None, 0,
                C.byref(md) if md is not None else None, C.byref(hf) if hf is not None else None, C.byref(s))
        got.append((rc, L.nh_last_error()))
    assert got[0] == got[1], got
    return got[0]


def test_every_argument_error_comes_before_a_device_and_creates_nothing(files):
    from nohuman_amd import _lib
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode())
    before = sorted(p.name for p in files.iterdir())
    rc, msg = _both(_args(files), x, None, _hf([9606], size=47))
    assert rc == NH_EINVAL and b"struct_size" in msg
    rc, msg = _both(_args(files), x, None, _hf([], [9606]))
    assert rc == NH_EINVAL and b"keep" in msg and b"host" in msg
    rc, msg = _both(_args(files), x, None, _hf(list(range(2, 12)), list(range(12, 19))))
    assert rc == NH_EINVAL and b"17" in msg and b"16" in msg
    rc, msg = _both(_args(files), x, None, _hf([9606], null_host=True))
    assert rc == NH_EINVAL and b"null" in msg
    rc, msg = _both(_args(files), x, None, _hf([9606], [10], null_keep=True))
    assert rc == NH_EINVAL and b"null" in msg
    for host, keep in (([0], []), ([9606, 0], []), ([9606], [0])):
        rc, msg = _both(_args(files), x, None, _hf(host, keep))
        assert rc == NH_EINVAL and b"taxid 0" in msg, msg
    for host, keep in (([10, 20, 10], []), ([1], [11, 11]), ([1, 9606], [9606])):
        rc, msg = _both(_args(files), x, None, _hf(host, keep))
        assert rc == NH_EINVAL and b"twice" in msg, msg
    # every check of nh_run_mdata, behind the selection's own: the minimum base quality, the extras, the minimizer data
    rc, msg = _both(_args(files), x, None, _hf([9606]), minq=94)
    assert rc == NH_EINVAL and b"93" in msg
    bad_x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "a.fq").encode())
    rc, msg = _both(_args(files), bad_x, None, _hf([9606]))
    assert rc == NH_EINVAL and b"a.fq" in msg
    md = _lib.nh_minimizer_data(struct_size=31, in_report=1)
    rc, msg = _both(_args(files), x, md, _hf([9606]))
    assert rc == NH_EINVAL and b"struct_size" in msg and b"nh_minimizer_data" in msg
    # sixteen taxids are allowed: the next refusal is the null engine
    L = _lib.lib()
    s = _lib.nh_stats()
    hf = _hf(list(range(2, 10)), list(range(10, 18)))
    assert L.nh_run_engine_host(None, C.byref(_args(files)), C.byref(x), 0, None, None, None, 0, None, C.byref(hf), C.byref(s)) == NH_EINVAL
    assert b"null engine" in L.nh_last_error()
    assert sorted(p.name for p in files.iterdir()) == before  # no file created


def test_without_a_selection_it_is_nh_run_mdata(files):
    """hf NULL, and hf that lists no taxid, reach nh_run_mdata's own checks with nh_run_mdata's messages"""
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras), calls=str(files / "c.txt").encode())
    for hf in (None, _hf()):
        hfp = C.byref(hf) if hf is not None else None
        md = _lib.nh_minimizer_data(struct_size=31, in_report=1)
        assert L.nh_run_mdata(C.byref(_args(files)), C.byref(x), 0, None, None, None, 0, C.byref(md), C.byref(s)) == NH_EINVAL
        want = L.nh_last_error()
        assert b"nh_run_mdata" in want
        assert L.nh_run_host(C.byref(_args(files)), C.byref(x), 0, None, None, None, 0, C.byref(md), hfp, C.byref(s)) == NH_EINVAL
        assert L.nh_last_error() == want
        assert L.nh_run_engine_host(None, C.byref(_args(files)), C.byref(x), 0, None, None, None, 0, C.byref(md), hfp, C.byref(s)) == NH_EINVAL
        assert L.nh_last_error() == want
        rc, msg = _both(_args(files), x, None, hf, minq=2 ** 32 - 1)
        assert rc == NH_EINVAL and b"93" in msg
        assert L.nh_run_engine_host(None, C.byref(_args(files)), C.byref(x), 0, None, None, None, 0, None, hfp, C.byref(s)) == NH_EINVAL
        assert b"null engine" in L.nh_last_error()
    assert not (files / "o.fq").exists() and not (files / "c.txt").exists()


def test_device_entry_refuses_null_arguments():
    from nohuman_amd import _lib
    L = _lib.lib()
    assert L.nh_host_filter_device(None, None, None, 0, None, 0, None, None) == NH_EINVAL
    assert L.nh_host_filter_device(None, 16, 16, 4, 16, 4, None, None) == NH_EINVAL and b"null" in L.nh_last_error()


def test_python_keywords(files):
    from nohuman_amd import Engine, EngineError, engine
    for fn in (engine.run, Engine.run):
        p = inspect.signature(fn).parameters
        assert p["host_taxids"].default is None and p["keep_taxids"].default is None
    assert callable(Engine.host_filter_device) and callable(engine.host_table)
    for kw, word in ((dict(keep_taxids=[10]), "keep"), (dict(host_taxids=[0]), "taxid 0"), (dict(host_taxids=[10, 10]), "twice"),
                     (dict(host_taxids=[1], keep_taxids=[1]), "twice"), (dict(host_taxids=list(range(1, 18))), "16")):
        with pytest.raises(EngineError) as ei:
            engine.run(DB, str(files / "a.fq"), str(files / "o.fq"), **kw)
        assert ei.value.code == NH_EINVAL and word in ei.value.message, (kw, ei.value.message)
    assert not (files / "o.fq").exists()


def test_runner_mirrors_the_flags():
    from nohuman_amd import CommandRunner
    o = CommandRunner.parse_argv(["--db", "d", "--host-taxid", "9606", "--keep-taxid", "10239", "--host-taxid", "10090",
                                  "--unclassified-out", "o.fq", "in.fq"])
    assert o["host_taxids"] == [9606, 10090] and o["keep_taxids"] == [10239] and o["inputs"] == ["in.fq"]
    o = CommandRunner.parse_argv(["--db", "d", "in.fq"])
    assert o["host_taxids"] == [] and o["keep_taxids"] == []
    for bad in ("x", "-1", "0", ""):
        with pytest.raises(OSError):
            CommandRunner.parse_argv(["--host-taxid", bad, "in.fq"])


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_flags(files):
    r = _cli(["--help"])
    assert r.returncode == 0 and "--host-taxid <TAXID>" in r.stdout and "--keep-taxid <TAXID>" in r.stdout
    tail = ["-o", str(files / "o.fq"), str(files / "a.fq")]

    def refused(args, *words):
        r = _cli(["--db", DB] + args + tail)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and "try '--help'" in r.stderr, (args, r.stderr)
        for w in words:
            assert w in r.stderr, (args, r.stderr)
    refused(["--host-taxid", "human"], "--host-taxid", "human")
    refused(["--host-taxid", "9606", "--keep-taxid", "1x"], "--keep-taxid", "1x")
    refused(["--host-taxid", "0"], "--host-taxid", "0")
    refused(["--host-taxid", "9606", "--host-taxid", "9606"], "9606", "more than once")
    refused(["--host-taxid", "9606", "--keep-taxid", "9606"], "9606", "more than once")
    many = []
    for t in range(2, 19):
        many += ["--host-taxid" if t % 2 else "--keep-taxid", str(t)]
    refused(many, "16")
    refused(["--keep-taxid", "10"], "--keep-taxid", "--host-taxid")
    r = _cli(["--host-taxid"])
    assert r.returncode == 2 and "a value is required" in r.stderr
    for flag in ("--host-taxid", "--keep-taxid"):
        r = _cli(["--build-db", str(files / "db"), "--reference", str(files / "a.fq"), flag, "10"])
        assert r.returncode == 2 and flag in r.stderr and "--build-db" in r.stderr
    assert not (files / "o.fq").exists() and not (files / "db").exists()


# ---- the host-node table of a taxo.k2d image against the model

def _table(taxo, host, keep, cap=None):
    from nohuman_amd import _lib
    L = _lib.lib()
    n = C.c_uint64(0)
    cap = int.from_bytes(taxo[8:16], "little") if cap is None else cap
    buf = (C.c_uint8 * max(cap, 1))(*([0xA5] * max(cap, 1)))
    hf = _hf(list(host), list(keep))
    rc = L.nh_host_table_image(taxo, len(taxo), C.byref(hf), buf, cap, C.byref(n))
    return rc, L.nh_last_error(), bytes(buf), int(n.value)


def _check_tree(edges, selections):
    from nohuman_amd import engine
    tax = minidb.Taxonomy(edges)
    taxo = tax.to_bytes()
    for host, keep in selections:
        want = hm.table(tax.external, hm.host_of(edges, host, keep))
        rc, msg, got, n = _table(taxo, host, keep)
        assert rc == 0, msg
        assert n == tax.node_count == len(want) and got == want, (host, keep)
        assert engine.host_table(taxo, host, keep) == want
    return tax, taxo


def test_table_of_the_toy_taxonomy():
    edges = dict(synth.TOY_EDGES)
    _check_tree(edges, [([1], []), ([9606], []), ([10, 20], []), ([10], [11]), ([1, 9606], [20]), ([1, 111], [10]), ([1], [10, 11])])
    taxo = open(os.path.join(DB, "taxo.k2d"), "rb").read()  # the database of the GPU tests holds the same tree
    rc, msg, got, n = _table(taxo, [10], [11])
    assert rc == 0 and n == 10
    ext = [int.from_bytes(taxo[32 + 56 * i + 40:32 + 56 * i + 48], "little") for i in range(n)]
    assert sorted(ext[1:]) == sorted(edges) and got == hm.table(ext, hm.host_of(edges, [10], [11]))


def test_table_of_a_caterpillar_of_depth_300():
    """a spine 1 - 2 - ... - 300 with a leaf 1000 + i hanging off every spine node"""
    edges = {1: 0}
    for i in range(2, 301):
        edges[i] = i - 1
    for i in range(1, 301):
        edges[1000 + i] = i
    _check_tree(edges, [([1], []), ([300], []), ([150], [200]), ([1, 250], [100, 275]), ([1100], []), ([2], [3, 1002]),
                        ([1, 3, 5, 7, 9, 11, 13, 15], [2, 4, 6, 8, 10, 12, 14, 16])])


def test_table_of_a_random_tree_of_5000_nodes_with_16_selectors():
    rng = np.random.default_rng(5000)
    edges = {1: 0}
    ids = [1]
    for t in rng.permutation(np.arange(2, 200000))[:4999].tolist():  # (external ids in no order: internal ids are the BFS's)
        edges[t] = ids[int(rng.integers(0, len(ids)))]
        ids.append(t)
    sels = []
    for _ in range(3):
        pick = [ids[i] for i in rng.permutation(len(ids))[:16].tolist()]
        sels.append((pick[:9], pick[9:]))
    sels.append(([1] + sels[0][0][:7], sels[0][1] + [sels[0][0][8]]))
    tax, taxo = _check_tree(edges, sels)
    assert tax.node_count == 5001
    m = hm.host_of(edges, *sels[3])
    assert 0 < sum(m.values()) < 5000


def test_what_the_table_refuses():
    taxo = minidb.Taxonomy(dict(synth.TOY_EDGES)).to_bytes()
    rc, msg, got, _ = _table(taxo, [4242], [])
    assert rc == NH_EINVAL and b"4242" in msg
    rc, msg, got, _ = _table(taxo, [1], [4243])
    assert rc == NH_EINVAL and b"4243" in msg
    rc, msg, got, n = _table(taxo, [1], [], cap=9)
    assert rc == NH_EINVAL and n == 10 and got == b"\xA5" * 9  # (a table too small is not written)
    for host, keep, word in (([], [10], b"keep"), ([0], [], b"taxid 0"), ([10, 10], [], b"twice")):
        rc, msg, _, _ = _table(taxo, host, keep)
        assert rc == NH_EINVAL and word in msg
    for cut in (taxo[:-1], taxo[:200], taxo[:31], b"", taxo + b"\0"):
        rc, msg, got, _ = _table(cut, [1], [], cap=10)
        assert rc == NH_EDB and got == b"\xA5" * 10, (len(cut), msg)
    rc, msg, _, _ = _table(b"K2TAXDAX" + taxo[8:], [1], [], cap=10)
    assert rc == NH_EDB and b"magic" in msg
