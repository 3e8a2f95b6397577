"""nh_extend_db / nh_extend_check / `nohuman --build-db OUT --extend-db BASE` without a device: the two new symbols and structs,
every refusal (through nh_extend_check and nh_extend_db: the code, a message that names the file or the line, out_dir as it was),
the internal-id order of a merged tree against the model, and the CLI's usage errors.  Bases are forged on the CPU with
oracle/minidb.py.  tests/test_gpu_extend_db.py extends."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import nohuman_amd
from nohuman_amd import EngineError, _lib
from oracle import minidb
from tests import build_taxa_util as t
from tests import extend_cases as xc
from tests import extend_model as xm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
EINVAL, EIO, EDB, EDEVICE = -1, -2, -3, -4
FASTA = b">chr1\n" + b"ACGTTGCAAGGCTTAACCGGTTACGATCGATTGCA" * 4 + b"\n"


def tiny_hash(tax, capacity=64, cells=((3, 0x1234, 2),), size=None, kb=None, vb=None):
    """a hash.k2d with the given (index, key, value) cells at the value bits of the taxonomy"""
    v = minidb.value_bits_for(tax.node_count)
    arr = np.zeros(capacity, dtype="<u4")
    for i, key, value in cells:
        arr[i] = key << v | value
    return struct.pack("<4Q", capacity, len(cells) if size is None else size, 32 - v if kb is None else kb, v if vb is None else vb) + arr.tobytes()


@pytest.fixture
def env(tmp_path):
    for name in ("a.fa", "b.fa"):
        (tmp_path / name).write_bytes(FASTA)
    tax = t.taxonomy_of(t.TREE_LINES)
    base = xc.write_base(tmp_path / "base", tax, tiny_hash(tax))
    return tmp_path, tax, base


def call(fn, base, taxa=None, out_dir=None, paths=(), x_size=None, xs_size=None, null_x=False, **kw):
    """nh_extend_db or nh_extend_check through ctypes -> (return code, message, build stats, extend stats, per-node array)"""
    a, s, keep = t.raw_args(taxa, out_dir, paths, **kw)
    x = _lib.nh_extend_args()
    x.struct_size = C.sizeof(x) if x_size is None else x_size
    x.base_dir = None if base is None else os.fsencode(base)
    xs = _lib.nh_extend_stats()
    xs.struct_size = C.sizeof(xs) if xs_size is None else xs_size
    rc = getattr(_lib.lib(), fn)(C.byref(a), None if null_x else C.byref(x), C.byref(s), C.byref(xs))
    return rc, _lib.lib().nh_last_error().decode(errors="replace"), s, xs, keep[1]


def both(*args, **kw):
    """the call through nh_extend_check and nh_extend_db: one code, one message -> (code, message)"""
    rc, msg, *_ = call("nh_extend_check", *args, **kw)
    rc2, msg2, *_ = call("nh_extend_db", *args, **kw)
    assert (rc, msg) == (rc2, msg2)
    return rc, msg


def test_header_binding_and_struct_sizes():
    header = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    for name in ("nh_extend_db", "nh_extend_check"):
        assert re.search(r"\bint %s\(const nh_build_args \*b, const nh_extend_args \*x, nh_build_stats \*bs, nh_extend_stats \*xs\);" % name, header)
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == 4 and getattr(_lib.lib(), name) is not None
    assert C.sizeof(_lib.nh_extend_args) == 24 and _lib.nh_extend_args.base_dir.offset == 8 and _lib.nh_extend_args.base_cells.offset == 16
    assert C.sizeof(_lib.nh_extend_stats) == 80 and _lib.nh_extend_stats.base_size.offset == 8 and _lib.nh_extend_stats.seconds_rekey.offset == 72
    assert "#define NH_ABI_VERSION 5" in header and _lib.lib().nh_abi_version() == 5
    assert nohuman_amd.extend_db is not None and "extend_db" in nohuman_amd.__all__
    # no existing struct has changed
    assert (C.sizeof(_lib.nh_build_args), C.sizeof(_lib.nh_build_args_v2), C.sizeof(_lib.nh_build_args_v3)) == (80, 88, 112)
    assert (C.sizeof(_lib.nh_build_stats), C.sizeof(_lib.nh_build_stats_v2), C.sizeof(_lib.nh_build_stats_v3)) == (88, 104, 112)
    assert C.sizeof(_lib.nh_build_taxon_stats) == 40 and C.sizeof(_lib.nh_db_info) == 96 and C.sizeof(_lib.nh_stats) == 48


def test_arguments_refused_before_any_device(env):
    tmp, tax, base = env
    out = tmp / "out"
    m = t.write_manifest(tmp / "add.tsv", [(40, 1, "D", "a.fa")])
    assert call("nh_extend_check", base, m, str(out))[0] == 0
    cases = {
        "no base": (dict(base=None), "base_dir"),
        "capacity": (dict(capacity=1000), "capacity 1000"),
        "args too small": (dict(struct_size=88), "struct_size 88"),
        "extend args too small": (dict(x_size=16), "struct_size 16"),
        "extend stats too small": (dict(xs_size=72), "struct_size 72"),
        "no extend args": (dict(null_x=True), "null"),
        "load factor": (dict(load_factor=0.96), "load factor"),
        "out_dir is the base": (dict(out_dir=base), "the base database itself"),
        "out_dir is the base, by another name": (dict(out_dir=os.path.join(str(tmp), "out", "..", "base", ".")), "the base database itself"),
        "taxa with fasta": (dict(paths=[str(tmp / "b.fa")]), "taxa_file cannot be combined"),
    }
    for name, (kw, what) in cases.items():
        kw = dict(dict(base=base, taxa=m, out_dir=str(out)), **kw)
        if name.endswith("another name"):
            out.mkdir()
        rc, msg = both(**kw)
        if name.endswith("another name"):
            out.rmdir()
        assert rc == EINVAL and what in msg, (name, rc, msg)
        assert not out.exists(), name
    for missing in ("hash.k2d", "opts.k2d", "taxo.k2d"):
        b2 = xc.write_base(tmp / ("base_without_" + missing), tax, tiny_hash(tax))
        os.unlink(os.path.join(b2, missing))
        rc, msg = both(b2, m, str(out))
        assert rc == EINVAL and missing in msg and b2 in msg and not out.exists()
    rc, msg = both(str(tmp / "nowhere"), m, str(out))
    assert rc == EINVAL and "nowhere" in msg and not out.exists()
    # a database already in out_dir needs `force`, as in a build
    xc.write_base(out, tax, tiny_hash(tax))
    rc, msg = both(base, m, str(out))
    assert rc == EINVAL and "force" in msg and sorted(os.listdir(out)) == ["hash.k2d", "opts.k2d", "taxo.k2d"]
    assert call("nh_extend_check", base, m, str(out), force=1)[0] == 0


def test_manifests_refused_against_the_base(env):
    tmp, tax, base = env
    out = tmp / "out"
    many = [(1000 + i, 1, "t%d" % i) for i in range(4092)]
    many[0] += ("a.fa",)
    refused = {
        "parent in neither": (["40\t41\tD\ta.fa"], 1, "41"),
        "parent in neither, behind a good line": (["40\t%d\tD\ta.fa" % t.A, "50\t60\tE\tb.fa"], 2, "60"),
        "existing taxid under another parent": (["%d\t1\ttaxon A\ta.fa" % t.A], 1, "under the parent %d" % t.G),
        "existing taxid under a new line": (["40\t1\tD", "%d\t40\ttaxon C\ta.fa" % t.C_], 2, "under the parent 1"),
        "taxid twice": (["40\t1\tD\ta.fa", "40\t1\tD\tb.fa"], 2, "twice"),
        "taxid 1": (["1\t1\troot\ta.fa"], 1, "root"),
        "no FASTA": (["40\t1\tD"], None, "no FASTA"),
        "a cycle among the lines": (["40\t50\tD\ta.fa", "50\t40\tE"], 1, "cycle"),
        "too many nodes": (many, None, "more than 4096 nodes"),  # the root, four taxa of the base and 4092 lines: 4097
    }
    for name, (lines, line_no, what) in refused.items():
        m = t.write_manifest(tmp / "add.tsv", lines)
        rc, msg = both(base, m, str(out))
        assert rc == EINVAL and m in msg and what in msg, (name, rc, msg)
        if line_no is not None:
            assert "line %d:" % line_no in msg, (name, msg)
        assert not out.exists(), name
    # 4091 lines fit: 4096 nodes with the root
    m = t.write_manifest(tmp / "add.tsv", many[:4091])
    rc, msg, s, xs, _ = call("nh_extend_check", base, m, str(out))
    assert rc == 0 and s.taxa == 4096 and xs.nodes_added == 4091, msg
    # one taxon without a manifest: taxid 1 is refused as in a build
    rc, msg = both(base, None, str(out), paths=[str(tmp / "a.fa")], taxid=1)
    assert rc == EINVAL and "taxid 1" in msg


def test_a_large_base_plus_ten_lines(tmp_path):
    (tmp_path / "a.fa").write_bytes(FASTA)
    lines = [(100 + i, 1, "t%d" % i) for i in range(4088)]  # the sentinel, the root and 4088 taxa: 4090 nodes
    tax = t.taxonomy_of(lines)
    assert tax.node_count == 4090
    base = xc.write_base(tmp_path / "base", tax, tiny_hash(tax))
    out = tmp_path / "out"
    m = t.write_manifest(tmp_path / "add.tsv", [(10 + i, 1, "new %d" % i) + (("a.fa",) if i == 0 else ()) for i in range(10)])
    rc, msg = both(base, m, str(out))
    assert rc == EINVAL and "more than 4096 nodes" in msg and m in msg and not out.exists()
    m = t.write_manifest(tmp_path / "add.tsv", [(10 + i, 1, "new %d" % i) + (("a.fa",) if i == 0 else ()) for i in range(7)])
    rc, msg, s, xs, per = call("nh_extend_check", base, m, str(out))
    assert rc == 0 and s.taxa == 4096 and (xs.base_nodes, xs.nodes_added, xs.base_value_bits) == (4090, 7, 12), msg
    assert [per[i].taxid for i in range(9)] == [1] + [10 + i for i in range(7)] + [100]


def test_bad_base_files_are_refused(env):
    tmp, tax, base = env
    out = tmp / "out"
    m = t.write_manifest(tmp / "add.tsv", [(40, 1, "D", "a.fa")])
    good = dict(hash=tiny_hash(tax), opts=minidb.opts_bytes(), taxo=xc.taxo_bytes(tax))
    twice = bytearray(good["taxo"])
    struct.pack_into("<Q", twice, 32 + 56 * 4 + 40, tax.external[3])  # node 4 with the external id of node 3
    above = bytearray(good["taxo"])
    struct.pack_into("<Q", above, 32 + 56 * 2, 5)  # node 2 with the parent 5
    bad = {
        "hash: no header": (dict(hash=good["hash"][:20]), "hash.k2d", "truncated"),
        "hash: truncated": (dict(hash=good["hash"][:-4]), "hash.k2d", "truncated"),
        "hash: bits": (dict(hash=tiny_hash(tax, kb=30)), "hash.k2d", "is not 32"),
        "hash: capacity": (dict(hash=struct.pack("<4Q", 1 << 33, 1, 29, 3)), "hash.k2d", "capacity"),
        "opts: k = 31": (dict(opts=minidb.opts_bytes(k=31)), "opts.k2d", "k is not"),
        "opts: l": (dict(opts=minidb.opts_bytes(l=29, spaced_mask=minidb.default_spaced_mask())), "opts.k2d", "l is not"),
        "opts: toggle": (dict(opts=minidb.opts_bytes(toggle=1)), "opts.k2d", "toggle_mask"),
        "opts: spaced": (dict(opts=minidb.opts_bytes(spaced_mask=0)), "opts.k2d", "spaced_seed_mask"),
        "opts: protein": (dict(opts=minidb.opts_bytes(dna_db=0)), "opts.k2d", "dna_db"),
        "opts: revcom": (dict(opts=minidb.opts_bytes(revcom_version=0)), "opts.k2d", "revcom_version"),
        "opts: minimum hash": (dict(opts=minidb.opts_bytes(min_hash=5)), "opts.k2d", "minimum_acceptable_hash_value"),
        "opts: truncated": (dict(opts=good["opts"][:40]), "opts.k2d", "truncated"),
        "taxo: magic": (dict(taxo=b"K2TAXDAX" + good["taxo"][8:]), "taxo.k2d", "magic"),
        "taxo: truncated": (dict(taxo=good["taxo"][:-3]), "taxo.k2d", "truncated"),
        "taxo: in the nodes": (dict(taxo=good["taxo"][:100]), "taxo.k2d", "truncated"),
        "taxo: an id twice": (dict(taxo=bytes(twice)), "taxo.k2d", "appears twice"),
        "taxo: a parent above": (dict(taxo=bytes(above)), "taxo.k2d", "does not lie below"),
    }
    for name, (files, which, what) in bad.items():
        f = dict(good, **files)
        b2 = str(tmp / "bad_base")
        minidb.write_db(b2, f["opts"], f["taxo"], f["hash"])
        rc, msg = both(b2, m, str(out))
        assert rc == EDB and os.path.join(b2, which) in msg and what in msg, (name, rc, msg)
        assert not out.exists(), name


def test_the_merged_tree_is_numbered_like_the_model(env):
    tmp, tax, base = env
    out = tmp / "out"
    lines = [(15, t.G, "between A and B", "a.fa"), (t.B, t.G, "never used", "b.fa"), (5, 1, "before C"), (7, 5, "below the new 5"), (200, t.A, "below A")]
    m = t.write_manifest(tmp / "add.tsv", lines)
    rc, msg, s, xs, per = call("nh_extend_check", base, m, str(out))
    want, remap = xm.merge(xc.taxo_bytes(tax), lines)
    assert rc == 0 and s.taxa == want.node_count - 1 and (xs.base_nodes, xs.nodes_added, xs.base_value_bits) == (6, 4, 3), msg
    assert [per[i].taxid for i in range(s.taxa)] == want.external[1:] == [1, 5, t.C_, t.G, 7, t.A, 15, t.B, 200]
    assert remap == [0, 1, 3, 4, 6, 8]
    # one taxon: a child of the root, or the node the base has, wherever it hangs
    for taxid, ext in ((25, [1, 25, t.C_, t.G, t.A, t.B]), (t.B, [1, t.C_, t.G, t.A, t.B]), (0, [1, t.C_, t.G, 9606, t.A, t.B])):
        rc, msg, s, xs, per = call("nh_extend_check", base, None, str(out), paths=[str(tmp / "a.fa")], taxid=taxid)
        assert rc == 0 and [per[i].taxid for i in range(s.taxa)] == ext and xs.nodes_added == len(ext) - 5, (taxid, msg)
    assert not out.exists()


def test_without_a_device_nothing_is_created(env):
    tmp, tax, base = env
    out = tmp / "out"
    m = t.write_manifest(tmp / "add.tsv", [(40, 1, "D", "a.fa")])
    before = {f: open(os.path.join(base, f), "rb").read() for f in os.listdir(base)}
    rc, msg, *_ = call("nh_extend_db", base, m, str(out))
    assert rc == EDEVICE and not out.exists(), msg
    with pytest.raises(EngineError) as ei:
        nohuman_amd.extend_db(base, out, taxa=m, device=t.NO_DEVICE)
    assert ei.value.code == EDEVICE and not out.exists()
    with pytest.raises(EngineError) as ei:
        nohuman_amd.extend_db(base, out, [tmp / "a.fa"], taxid=77, taxon_name="seventy-seven", device=t.NO_DEVICE)
    assert ei.value.code == EDEVICE and not out.exists()
    assert before == {f: open(os.path.join(base, f), "rb").read() for f in os.listdir(base)}


def _cli(*args):
    p = subprocess.run([BIN] + list(args), capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")


def test_cli_usage_errors(env):
    tmp, tax, base = env
    reads = tmp / "reads.fq"
    reads.write_bytes(b"@r\nACGT\n+\nIIII\n")
    d = str(tmp / "db")
    m = t.write_manifest(tmp / "add.tsv", [(40, 1, "D", "a.fa")])
    orphan = t.write_manifest(tmp / "orphan.tsv", [(40, 41, "D", "a.fa")])
    ref = str(tmp / "b.fa")
    for args, what in ((("--extend-db", base, "--taxa", m), "needs '--build-db <DIR>'"),
                       (("--extend-db", base, str(reads)), "needs '--build-db <DIR>'"),
                       (("--build-db", d, "--extend-db", base, "--taxa", m, str(reads)), "read inputs"),
                       (("--build-db", d, "--extend-db", base, "--taxa", m, "--capacity", "1000"), "--capacity <INT>"),
                       (("--build-db", d, "--extend-db", base, "--reference", ref, "--capacity", "1000"), "--capacity <INT>"),
                       (("--build-db", d, "--extend-db", base), "--reference <FILE>"),
                       (("--build-db", d, "--extend-db"), "--extend-db"),
                       (("--build-db", d, "--extend-db", str(tmp / "nowhere"), "--taxa", m), "does not exist"),
                       (("--build-db", d, "--extend-db", base, "--taxa", m, "--reference", ref), "--taxa <FILE>"),
                       (("--build-db", d, "--extend-db", base, "--taxa", orphan), "line 1:"),
                       (("--build-db", base, "--extend-db", base, "--taxa", m, "--force"), "the base database itself"),
                       (("--build-db", d, "--extend-db", base, "--reference", ref, "--taxid", "1"), "taxid 1")):
        rc, _, err = _cli(*args)
        assert rc == 2 and err.startswith("error: ") and "try '--help'" in err and what in err, (args, rc, err)
        assert "dependencies" not in err and not os.path.exists(d), args
    # what passes every check ends at the device probe, with nothing created
    rc, _, err = _cli("--build-db", d, "--extend-db", base, "--taxa", m)
    assert (rc != 2 or "dependencies" in err) and not os.path.exists(d) or nohuman_amd.device_count() > 0
    # a base that is no database of the default geometry: not a usage error, and before the device probe
    b2 = str(tmp / "k31")
    minidb.write_db(b2, minidb.opts_bytes(k=31), xc.taxo_bytes(tax), tiny_hash(tax))
    rc, _, err = _cli("--build-db", d, "--extend-db", b2, "--taxa", m)
    assert rc == 1 and "opts.k2d" in err and "dependencies" not in err and not os.path.exists(d)


def test_cli_help_has_one_line_for_the_flag():
    rc, out, _ = _cli("--help")
    assert rc == 0
    lines = [ln for ln in out.split("\n") if "--extend-db" in ln]
    assert len(lines) == 1 and "--extend-db <DIR>" in lines[0]
    for other in ("--build-db", "--reference", "--taxid", "--taxon-name", "--load-factor", "--capacity", "--force", "--mask", "--db ", "--taxa"):
        assert other not in lines[0], other
