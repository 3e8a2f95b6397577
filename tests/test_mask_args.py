"""Masked runs (nh_run_mask / nh_run_engine_mask, `--mask`): the entries are declared, bound and exported, and every
argument error is found before a device is touched -- NH_EINVAL from the library, exit code 2 from the CLI host.  No GPU
needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1


def test_mask_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ("nh_run_mask", "nh_run_engine_mask"):
        assert name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None


@pytest.fixture
def files(tmp_path):
    for n in ("a_1.fq", "a_2.fq"):
        (tmp_path / n).write_bytes(b"@r\nACGT\n+\nIIII\n")
    return tmp_path


def _args(d, paired=False, **kw):
    from nohuman_amd import _lib
    a = _lib.nh_run_args()
    a.db_dir = DB.encode()
    a.in1 = str(d / "a_1.fq").encode()
    a.in2 = str(d / "a_2.fq").encode() if paired else None
    a.out1 = str(d / "o_1.fq").encode()
    a.out2 = str(d / "o_2.fq").encode() if paired else None
    a.kraken_output = str(d / "k.txt").encode()
    a.report = str(d / "r.txt").encode()
    for k, v in kw.items():
        setattr(a, k, v.encode() if isinstance(v, str) else v)
    return a


def _p(d, name):
    return str(d / name).encode() if name else None


def _bad_cases(d):
    link = d / "link_to_input.fq"
    if not link.exists():
        os.link(d / "a_1.fq", link)
    i1, i2 = str(d / "a_1.fq"), str(d / "a_2.fq")
    return [
        ("keep_human set", _args(d, keep_human=1), None, None),
        ("keep_human set, with human outputs", _args(d, keep_human=1), "h_1.fq", None),
        # the split run's checks, when human outputs are given
        ("human_out2 without human_out1", _args(d), None, "h_2.fq"),
        ("human_out2 without in2", _args(d), "h_1.fq", "h_2.fq"),
        ("in2 without human_out2", _args(d, paired=True), "h_1.fq", None),
        ("human output names in1", _args(d), "a_1.fq", None),
        ("human output same inode as in1", _args(d), "link_to_input.fq", None),
        ("human output names out1", _args(d), "o_1.fq", None),
        ("human output names the report", _args(d), "r.txt", None),
        ("human outputs are the same file", _args(d, paired=True), "h.fq", "h.fq"),
        # an output that names an input
        ("out1 names in1", _args(d, out1=i1), None, None),
        ("out2 names in2", _args(d, paired=True, out2=i2), None, None),
        ("out1 same inode as in1", _args(d, out1=str(link)), None, None),
        ("kraken_output names in1", _args(d, kraken_output=i1), None, None),
        ("report names in2", _args(d, paired=True, report=i2), None, None),
    ]


def test_mask_argument_errors_come_before_any_device(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    for why, a, h1, h2 in _bad_cases(files):
        rc = L.nh_run_mask(C.byref(a), _p(files, h1), _p(files, h2), C.byref(s))
        assert rc == NH_EINVAL, (why, rc, L.nh_last_error())
        assert "nh_run_mask" in L.nh_last_error().decode(), why
        rc = L.nh_run_engine_mask(None, C.byref(a), _p(files, h1), _p(files, h2), C.byref(s))
        assert rc == NH_EINVAL, (why, rc, L.nh_last_error())
        assert "nh_run_mask" in L.nh_last_error().decode(), why
    assert not any(p.name.startswith(("h", "o_", "k.", "r.")) for p in files.iterdir())  # nothing was created
    assert (files / "a_1.fq").read_bytes() == b"@r\nACGT\n+\nIIII\n"  # no input was emptied


def test_python_mask_keyword_reaches_the_mask_entry(files):
    from nohuman_amd import EngineError, engine
    with pytest.raises(EngineError) as ei:  # keep_human with mask: refused by nh_run_mask, not run as -H
        engine.run(DB, str(files / "a_1.fq"), str(files / "o.fq"), keep_human=True, mask=True)
    assert ei.value.code == NH_EINVAL and "nh_run_mask" in ei.value.message
    with pytest.raises(EngineError) as ei:  # an output that is the input: refused before the database is opened
        engine.run(DB, str(files / "a_1.fq"), str(files / "a_1.fq"), mask=True)
    assert ei.value.code == NH_EINVAL and "nh_run_mask" in ei.value.message
    assert (files / "a_1.fq").read_bytes() == b"@r\nACGT\n+\nIIII\n"


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_help_lists_mask():
    r = _cli(["--help"])
    assert r.returncode == 0
    line = [ln for ln in r.stdout.splitlines() if "--mask" in ln]
    assert len(line) == 1, r.stdout
    assert "Replace the bases of human reads with N instead of removing them" in line[0]
    assert not line[0].lstrip().startswith("-m")  # long form only


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_mask_with_human_exits_2(files):
    i1, i2 = str(files / "a_1.fq"), str(files / "a_2.fq")
    for args in (["--mask", "-H", i1], ["-H", "--mask", i1, i2], ["--human", "--mask", "-o", str(files / "o.fq"), i1]):
        r = _cli(args)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "the argument '--mask' cannot be used with '--human'" in r.stderr, (args, r.stderr)
        assert "dependencies" not in r.stderr  # found while parsing, before the device probe
    assert not any(p.name.startswith("o") or "nohuman" in p.name for p in files.iterdir())
