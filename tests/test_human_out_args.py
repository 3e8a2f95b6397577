"""Split runs (nh_run_split / nh_run_engine_split, `--human-out1` / `--human-out2`): the entries are declared, bound and
exported, and every argument error is found before a device is touched -- NH_EINVAL from the library, exit code 2 from
the CLI host.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1


def test_split_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ("nh_run_split", "nh_run_engine_split"):
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
        setattr(a, k, v)
    return a


def _p(d, name):
    return str(d / name).encode() if name else None


def _bad_cases(d):
    link = d / "link_to_input.fq"
    if not link.exists():
        os.link(d / "a_1.fq", link)
    return [
        ("human_out1 missing", _args(d), None, None),
        ("keep_human set", _args(d, keep_human=1), "h_1.fq", None),
        ("human_out2 without in2", _args(d), "h_1.fq", "h_2.fq"),
        ("in2 without human_out2", _args(d, paired=True), "h_1.fq", None),
        ("names in1", _args(d), "a_1.fq", None),
        ("names in2", _args(d, paired=True), "h_1.fq", "a_2.fq"),
        ("same inode as in1", _args(d), "link_to_input.fq", None),
        ("names out1", _args(d), "o_1.fq", None),
        ("names out2", _args(d, paired=True), "h_1.fq", "o_2.fq"),
        ("names kraken_output", _args(d), "k.txt", None),
        ("names report", _args(d), "r.txt", None),
    ]


def test_split_argument_errors_come_before_any_device(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    for why, a, h1, h2 in _bad_cases(files):
        rc = L.nh_run_split(C.byref(a), _p(files, h1), _p(files, h2), C.byref(s))
        assert rc == NH_EINVAL, (why, rc, L.nh_last_error())
        rc = L.nh_run_engine_split(None, C.byref(a), _p(files, h1), _p(files, h2), C.byref(s))
        assert rc == NH_EINVAL, (why, rc, L.nh_last_error())
        assert "nh_run_split" in L.nh_last_error().decode(), why
    assert not (files / "h_1.fq").exists() and not (files / "o_1.fq").exists()  # nothing was created


def test_python_keywords_reach_the_split_entry(files):
    from nohuman_amd import EngineError, engine
    with pytest.raises(EngineError) as ei:  # keep_human with a human output: refused by nh_run_split, not run as -H
        engine.run(DB, str(files / "a_1.fq"), str(files / "o.fq"), keep_human=True, human_out1=str(files / "h.fq"))
    assert ei.value.code == NH_EINVAL and "keep_human" in ei.value.message
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a_1.fq"), str(files / "o.fq"), human_out2=str(files / "h.fq"))
    assert ei.value.code == NH_EINVAL and "human_out1" in ei.value.message


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_help_lists_the_human_outputs():
    r = _cli(["--help"])
    assert r.returncode == 0
    assert "--human-out1 <PATH>" in r.stdout and "--human-out2 <PATH>" in r.stdout


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_human_output_conflicts_exit_2(files):
    i1, i2 = str(files / "a_1.fq"), str(files / "a_2.fq")
    h1, h2 = str(files / "h_1.fq"), str(files / "h_2.fq")
    cases = [
        (["-H", "--human-out1", h1, i1], "--human"),
        (["--human-out1", h1, "--human-out2", h2, i1], "--human-out2"),
        (["--human-out1", h1, i1, i2], "--human-out2"),
        (["--human-out2", h2, i1, i2], "--human-out1"),
        (["-o", h1, "--human-out1", h1, i1], "--human-out1"),
        (["-o", str(files / "o_1.fq"), "-O", h2, "--human-out1", h1, "--human-out2", h2, i1, i2], "--human-out2"),
    ]
    # a human output equal to the DEFAULT output name (beside the input, "<stem>.nohuman.fq")
    cases.append((["--human-out1", str(files / "a_1.nohuman.fq"), i1], "--human-out1"))
    for args, flag in cases:
        r = _cli(args)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert flag in r.stderr, (args, r.stderr)
        assert "dependencies" not in r.stderr  # found while parsing, before the device probe
    assert not any(p.name.startswith("h_") for p in files.iterdir())
