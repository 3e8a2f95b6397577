"""nh_build_db / `nohuman --build-db` without a device: what is refused before any device is touched (NH_EINVAL, nothing
created), the CLI's usage errors, and the no-GPU failure (NH_EDEVICE, no files).  tests/test_gpu_build_db.py builds."""
import ctypes as C
import os
import subprocess

import pytest

import nohuman_amd
from nohuman_amd import EngineError, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB_FILES = ("hash.k2d", "opts.k2d", "taxo.k2d")
NO_DEVICE = 1 << 20  # a device id no machine has: the call ends at the device check, with or without a GPU


def _has_gpu():
    n = C.c_int(0)
    return _lib.lib().nh_device_count(C.byref(n)) == 0 and n.value > 0


@pytest.fixture
def fa(tmp_path):
    p = tmp_path / "g.fa"
    p.write_bytes(b">chr1\n" + b"ACGTTGCAAGGCTTAACCGGTTACGATCGATTGCA" * 4 + b"\n")
    return str(p)


def _raw(paths, out_dir, struct_size=None, n_fasta=None, **kw):
    """nh_build_db through ctypes, every field settable -> (return code, message)"""
    a = _lib.nh_build_args()
    a.struct_size = C.sizeof(_lib.nh_build_args) if struct_size is None else struct_size
    arr = (C.c_char_p * max(len(paths), 1))(*[None if p is None else os.fsencode(p) for p in paths])
    a.n_fasta = len(paths) if n_fasta is None else n_fasta
    a.fasta = arr
    a.out_dir = None if out_dir is None else os.fsencode(out_dir)
    a.device = NO_DEVICE
    for k, v in kw.items():
        setattr(a, k, v)
    s = _lib.nh_build_stats()
    rc = _lib.lib().nh_build_db(C.byref(a), C.byref(s))
    return rc, _lib.lib().nh_last_error().decode(errors="replace")


def test_binding_matches_the_header():
    """the two structs as the header lays them out (LP64): 80 and 88 bytes, the fields at their offsets"""
    assert C.sizeof(_lib.nh_build_args) == 80 and C.sizeof(_lib.nh_build_stats) == 88
    assert [getattr(_lib.nh_build_args, f).offset for f in ("fasta", "out_dir", "taxid", "load_factor", "capacity", "piece_kmers",
                                                             "device", "threads", "force")] == [8, 16, 24, 40, 48, 56, 64, 68, 72]
    assert "nh_build_db" in _lib.SYMBOLS and nohuman_amd.build_db is not None


def test_invalid_arguments_are_refused_before_any_device(tmp_path, fa):
    out = tmp_path / "db"
    cases = {
        "struct_size": _raw([fa], str(out), struct_size=C.sizeof(_lib.nh_build_args) - 4),
        "n_fasta 0": _raw([], str(out)),
        "null path": _raw([fa, None], str(out)),
        "null list": _raw([], str(out), n_fasta=1, fasta=None),
        "no out_dir": _raw([fa], None),
        "load factor 0.96": _raw([fa], str(out), load_factor=0.96),
        "load factor -0.5": _raw([fa], str(out), load_factor=-0.5),
        "load factor nan": _raw([fa], str(out), load_factor=float("nan")),
        "taxid 1": _raw([fa], str(out), taxid=1),
    }
    for name, (rc, msg) in cases.items():
        assert rc == -1 and msg.startswith("nh_build_db:"), (name, rc, msg)
        assert not out.exists(), name
    # what passes these checks ends at the device check (a device no machine has), still without creating anything
    for kw in (dict(), dict(load_factor=0.95), dict(load_factor=0.01), dict(taxid=2), dict(capacity=1000, piece_kmers=7)):
        rc, msg = _raw([fa], str(out), **kw)
        assert rc == -4 and not out.exists(), (kw, rc, msg)


def test_an_existing_database_needs_force(tmp_path, fa):
    for held in DB_FILES:
        d = tmp_path / ("has_" + held)
        d.mkdir()
        (d / held).write_bytes(b"old")
        rc, msg = _raw([fa], str(d))
        assert rc == -1 and held in msg and "force" in msg, (rc, msg)
        rc, msg = _raw([fa], str(d), force=1)
        assert rc == -4, (rc, msg)
        assert os.listdir(d) == [held] and (d / held).read_bytes() == b"old"
    f = tmp_path / "a_file"
    f.write_bytes(b"")
    assert _raw([fa], str(f))[0] == -1  # not a directory


def test_an_input_inside_the_output_is_refused(tmp_path, fa):
    d = tmp_path / "db"
    d.mkdir()
    for name in DB_FILES:
        p = d / name
        p.write_bytes(open(fa, "rb").read())
        for path in (str(p), str(d / "." / name), str(tmp_path / "db" / ".." / "db" / name)):
            rc, msg = _raw([fa, path], str(d), force=1)
            assert rc == -1 and "input" in msg, (path, rc, msg)
        link = tmp_path / ("link_" + name)  # the same file under another name
        os.link(p, link)
        assert _raw([str(link)], str(d), force=1)[0] == -1
        link.unlink()
        p.unlink()
        # the name alone, the file not there yet: the build would write over its own input's path
        assert _raw([str(p)], str(d))[0] == -1
    assert os.listdir(d) == []


def test_python_entry_without_a_usable_device(tmp_path, fa):
    out = tmp_path / "db"
    with pytest.raises(EngineError) as ei:
        nohuman_amd.build_db(fa, out, device=NO_DEVICE)
    assert ei.value.code == -4 and not out.exists()
    with pytest.raises(EngineError) as ei:
        nohuman_amd.build_db([fa], out, taxid=1)
    assert ei.value.code == -1 and not out.exists()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback_without_a_device(tmp_path, fa):
    out = tmp_path / "db"
    with pytest.raises(EngineError) as ei:
        nohuman_amd.build_db([fa], out)
    assert ei.value.code == -4 and not out.exists()  # NH_EDEVICE
    assert os.listdir(tmp_path) == ["g.fa"]


def _cli(*args):
    p = subprocess.run([BIN] + list(args), capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")


def test_cli_help_lists_the_flags():
    rc, out, _ = _cli("--help")
    assert rc == 0
    for flag in ("--build-db <DIR>", "--reference <FILE>", "--taxid <INT>", "--taxon-name <NAME>", "--load-factor <FLOAT>",
                 "--capacity <INT>", "--force"):
        assert flag in out, flag


def test_cli_usage_errors(tmp_path, fa):
    reads = tmp_path / "reads.fq"
    reads.write_bytes(b"@r\nACGT\n+\nIIII\n")
    d = str(tmp_path / "db")
    cases = [
        ("--build-db", d),                                          # no --reference
        ("--reference", fa, str(reads)),                            # --reference without --build-db
        ("--reference", fa),
        ("--build-db", d, "--reference", fa, str(reads)),           # read inputs
        ("--build-db", d, "--reference", str(tmp_path / "none.fa")),
        ("--force", str(reads)), ("--taxid", "9606", str(reads)), ("--capacity", "100", str(reads)),
        ("--build-db", d, "--reference", fa, "--taxid", "0"),
        ("--build-db", d, "--reference", fa, "--taxid", "x"),
        ("--build-db", d, "--reference", fa, "--load-factor", "0.96"),
        ("--build-db", d, "--reference", fa, "--load-factor", "0"),
        ("--build-db", d, "--reference", fa, "--capacity", "-5"),
    ]
    for flag in (("-o", "o.fq"), ("-O", "o2.fq"), ("--human-out1", "h.fq"), ("--human-out2", "h2.fq"), ("-k", "k.txt"), ("-r", "r.txt"),
                 ("--calls", "c.tsv"), ("--human-ids", "i.txt"), ("--read-stats", "s.tsv"), ("-F", "g"), ("--bgzf",), ("--mask",), ("-H",)):
        cases.append(("--build-db", d, "--reference", fa) + flag)
    for args in cases:
        rc, _, err = _cli(*args)
        assert rc == 2 and err.startswith("error: ") and "try '--help'" in err, (args, rc, err)
        assert not os.path.exists(d), args
