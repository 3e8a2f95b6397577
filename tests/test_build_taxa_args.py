"""The taxa manifest of nh_build_db / `nohuman --build-db DIR --taxa FILE` without a device: every manifest that is refused, through
the ctypes binding (NH_EINVAL before any device is touched, out_dir as it was) and through the CLI (a usage error, exit 2, before
the device probe), what passes (it ends at the device check), and the three layouts of the two structs.
tests/test_gpu_build_db_taxa.py builds."""
import ctypes as C
import os
import subprocess

import pytest

import nohuman_amd
from nohuman_amd import EngineError, _lib
from tests import build_taxa_util as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB_FILES = ("hash.k2d", "opts.k2d", "taxo.k2d")
EINVAL, EIO, EDEVICE = -1, -2, -4
FASTA = b">chr1\n" + b"ACGTTGCAAGGCTTAACCGGTTACGATCGATTGCA" * 4 + b"\n"


@pytest.fixture
def fa(tmp_path):
    for name in ("a.fa", "b.fa"):
        (tmp_path / name).write_bytes(FASTA)
    return tmp_path


def refused_manifests(tmp):
    """name -> (manifest lines, the line number the message must name or None)"""
    many = [(10 + i, 1, "t%d" % i) for i in range(4096)]
    many[0] += ("a.fa",)
    return {
        "two fields": (["10\t1"], 1),
        "two fields, a comment before": (["# taxa", "", "10\t1\tA\ta.fa", "20\t1"], 4),
        "taxid not a number": (["x10\t1\tA\ta.fa"], 1),
        "taxid negative": (["-10\t1\tA\ta.fa"], 1),
        "taxid with a space": (["10 \t1\tA\ta.fa"], 1),
        "taxid beyond 64 bits": (["18446744073709551616\t1\tA\ta.fa"], 1),
        "taxid 0": (["0\t1\tA\ta.fa"], 1),
        "taxid 1": (["10\t1\tA\ta.fa", "1\t1\troot"], 2),
        "taxid twice": (["10\t1\tA\ta.fa", "20\t1\tB", "10\t20\tA again\tb.fa"], 3),
        "empty name": (["10\t1\t\ta.fa"], 1),
        "parent unknown": (["10\t1\tA\ta.fa", "20\t30\tB\tb.fa"], 2),
        "parent not a number": (["10\tone\tA\ta.fa"], 1),
        "parent 0": (["10\t0\tA\ta.fa"], 1),
        "its own parent": (["10\t10\tA\ta.fa"], 1),
        "cycle of two": (["10\t20\tA\ta.fa", "20\t10\tB"], 1),
        "cycle below the root's child": (["5\t1\tG", "10\t30\tA\ta.fa", "20\t10\tB", "30\t20\tC"], 2),
        "no FASTA": (["10\t1\tA", "20\t10\tB"], None),
        "no FASTA, trailing tab": (["10\t1\tA\t"], None),
        "empty manifest": (["# nothing"], None),
        "FASTA twice on a line": (["10\t1\tA\ta.fa\ta.fa"], 1),
        "FASTA twice by real path": (["10\t1\tA\ta.fa", "20\t1\tB\t%s" % os.path.join(str(tmp), ".", "a.fa")], 2),
        "4096 taxa": (many, 4096),
    }


def test_struct_sizes_of_the_three_layouts():
    assert (C.sizeof(_lib.nh_build_args), C.sizeof(_lib.nh_build_args_v2), C.sizeof(_lib.nh_build_args_v3)) == (80, 88, 112)
    assert (C.sizeof(_lib.nh_build_stats), C.sizeof(_lib.nh_build_stats_v2), C.sizeof(_lib.nh_build_stats_v3)) == (88, 104, 112)
    assert C.sizeof(_lib.nh_build_taxon_stats) == 40
    assert [getattr(_lib.nh_build_args_v3, f).offset for f in ("mask_low_complexity", "taxa_file", "taxon_stats", "taxon_stats_cap")] \
        == [80, 88, 96, 104]
    assert _lib.nh_build_stats_v3.taxa.offset == 104
    header = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    assert "#define NH_BUILD_ARGS_SIZE_V2 88u" in header and "#define NH_BUILD_ARGS_SIZE_V1 80u" in header


def test_every_bad_manifest_is_refused_before_any_device(fa):
    out = fa / "db"
    for name, (lines, line_no) in refused_manifests(fa).items():
        m = t.write_manifest(fa / "taxa.tsv", lines)
        for fn in ("nh_build_db", "nh_build_check"):
            rc, msg, _, _ = t.raw_call(fn, m, str(out))
            assert rc == EINVAL and msg.startswith("nh_build_db:") and m in msg, (name, fn, rc, msg)
            if line_no is not None:
                assert "line %d:" % line_no in msg, (name, msg)
            assert not out.exists(), name
    # CRLF changes nothing
    m = t.write_manifest(fa / "crlf.tsv", ["10\t1\tA\ta.fa", "20\t1"], crlf=True)
    rc, msg, _, _ = t.raw_call("nh_build_db", m, str(out))
    assert rc == EINVAL and "line 2:" in msg


def test_taxa_exclude_the_one_taxon_arguments(fa):
    out = fa / "db"
    m = t.write_manifest(fa / "taxa.tsv", [(10, 1, "A", "a.fa")])
    for name, kw in (("fasta", dict(paths=[str(fa / "b.fa")])), ("taxid", dict(taxid=10)), ("taxon_name", dict(taxon_name=b"A")),
                     ("load factor", dict(load_factor=0.96))):
        rc, msg, _, _ = t.raw_call("nh_build_db", m, str(out), **kw)
        assert rc == EINVAL and msg.startswith("nh_build_db:"), (name, rc, msg)
        assert not out.exists()
    for kw in (dict(fasta_paths=[str(fa / "b.fa")]), dict(taxid=10), dict(taxon_name="A")):
        with pytest.raises(EngineError) as ei:
            nohuman_amd.build_db(kw.pop("fasta_paths", None), str(out), taxa=m, device=t.NO_DEVICE, **kw)
        assert ei.value.code == EINVAL and not out.exists()
    with pytest.raises(EngineError) as ei:  # neither
        nohuman_amd.build_db(None, str(out), device=t.NO_DEVICE)
    assert ei.value.code == EINVAL
    # a caller of an earlier layout does not have the field: what lies behind its struct_size is not read
    rc, msg, _, _ = t.raw_call("nh_build_db", m, str(out), struct_size=88)
    assert rc == EINVAL and "n_fasta" in msg
    rc, msg, _, _ = t.raw_call("nh_build_db", m, str(out), paths=[str(fa / "a.fa")], struct_size=88)
    assert rc == EDEVICE, msg


def test_unreadable_inputs_are_io_errors(fa):
    out = fa / "db"
    rc, msg, _, _ = t.raw_call("nh_build_db", str(fa / "none.tsv"), str(out))
    assert rc == EIO and "none.tsv" in msg
    m = t.write_manifest(fa / "taxa.tsv", [(10, 1, "A", "a.fa"), (20, 1, "B", "missing.fa")])
    rc, msg, _, _ = t.raw_call("nh_build_db", m, str(out))
    assert rc == EIO and "line 2:" in msg and "missing.fa" in msg and not out.exists()


def test_manifest_or_fasta_inside_the_output_is_refused(fa):
    d = fa / "db"
    d.mkdir()
    for name in DB_FILES:
        (d / name).write_bytes(FASTA)
        m = t.write_manifest(fa / "taxa.tsv", [(10, 1, "A", "a.fa"), (20, 1, "B", os.path.join("db", ".", name))])
        rc, msg, _, _ = t.raw_call("nh_build_db", m, str(d), force=1)
        assert rc == EINVAL and "line 2:" in msg and "input" in msg, (name, rc, msg)
        # the manifest itself under one of the three names
        m = t.write_manifest(d / name, [(10, 1, "A", str(fa / "a.fa"))])
        rc, msg, _, _ = t.raw_call("nh_build_db", m, str(d), force=1)
        assert rc == EINVAL and "manifest" in msg, (name, rc, msg)
        (d / name).unlink()
    assert os.listdir(d) == []
    # an existing database still needs force
    (d / "hash.k2d").write_bytes(b"old")
    m = t.write_manifest(fa / "taxa.tsv", [(10, 1, "A", "a.fa")])
    rc, msg, _, _ = t.raw_call("nh_build_db", m, str(d))
    assert rc == EINVAL and "force" in msg and (d / "hash.k2d").read_bytes() == b"old"


def test_good_manifests_end_at_the_device_check(fa):
    out = fa / "db"
    sub = fa / "sub"
    sub.mkdir()
    (sub / "c.fa").write_bytes(FASTA)
    good = {
        "one taxon": ["10\t1\tA\ta.fa"],
        "comments, empty lines, inner nodes, a node with children and sequences": [
            "# taxid\tparent\tname\tfiles", "", "100\t1\tgroup\tb.fa", "10\t100\tname with spaces\ta.fa\tsub/c.fa", "30\t1\tinner", "40\t30\tD\t",
        ],
        "children before parents, an absolute path": ["20\t100\tB\t%s" % (fa / "b.fa"), "100\t1\tG", "10\t100\tA\ta.fa"],
        "4095 taxa": [(10 + i, 1 if i == 0 else 10 + (i - 1) // 2, "t%d" % i) + (("a.fa",) if i == 7 else ()) for i in range(4095)],
    }
    for name, lines in good.items():
        for crlf in (False, True):
            m = t.write_manifest(fa / "taxa.tsv", lines, crlf=crlf)
            rc, msg, _, _ = t.raw_call("nh_build_db", m, str(out))
            assert rc == EDEVICE and not out.exists(), (name, rc, msg)
            rc, msg, st, per = t.raw_call("nh_build_check", m, str(out))
            assert rc == 0 and not out.exists(), (name, rc, msg)
            n = sum(1 for ln in lines if not isinstance(ln, str) or (ln and not ln.startswith("#")))
            assert st.taxa == n + 1 and per[0].taxid == 1
    with pytest.raises(EngineError) as ei:
        nohuman_amd.build_db(None, out, taxa=m, device=t.NO_DEVICE)
    assert ei.value.code == EDEVICE and not out.exists()


def _cli(*args):
    p = subprocess.run([BIN] + list(args), capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")


def test_cli_refuses_every_bad_manifest_as_a_usage_error(fa):
    d = str(fa / "db")
    for name, (lines, line_no) in refused_manifests(fa).items():
        m = t.write_manifest(fa / "taxa.tsv", lines)
        rc, _, err = _cli("--build-db", d, "--taxa", m)
        assert rc == 2 and err.startswith("error: ") and "try '--help'" in err and "--taxa <FILE>" in err, (name, rc, err)
        if line_no is not None:
            assert "line %d:" % line_no in err, (name, err)
        assert "dependencies" not in err  # (the device probe's failure: never reached)
        assert not os.path.exists(d), name


def test_cli_usage_errors(fa):
    reads = fa / "reads.fq"
    reads.write_bytes(b"@r\nACGT\n+\nIIII\n")
    d = str(fa / "db")
    m = t.write_manifest(fa / "taxa.tsv", [(10, 1, "A", "a.fa")])
    ref = str(fa / "b.fa")
    for args in (("--build-db", d, "--taxa", m, "--reference", ref), ("--build-db", d, "--taxa", m, "--taxid", "10"),
                 ("--build-db", d, "--taxa", m, "--taxon-name", "A"), ("--taxa", m, str(reads)), ("--taxa", m),
                 ("--build-db", d, "--taxa"), ("--build-db", d, "--taxa", str(fa / "none.tsv")),
                 ("--build-db", d, "--taxa", m, str(reads)), ("--build-db", d, "--taxa", m, "-o", "o.fq")):
        rc, _, err = _cli(*args)
        assert rc == 2 and err.startswith("error: ") and "try '--help'" in err, (args, rc, err)
        assert not os.path.exists(d), args


def test_cli_help_has_one_line_for_the_flag():
    rc, out, _ = _cli("--help")
    assert rc == 0
    lines = [ln for ln in out.split("\n") if "--taxa <FILE>" in ln]
    assert len(lines) == 1
    for other in ("--build-db", "--reference", "--taxid", "--taxon-name", "--load-factor", "--capacity", "--force", "--mask", "--db"):
        assert other not in lines[0], other
