"""Read lists (nh_run_ex / nh_run_engine_ex, `--calls` / `--human-ids`): the entries and the struct are declared, bound and
exported, and every argument error is found before a device is touched -- NH_EINVAL from the library, nothing created at
the offending path.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
NH_EINVAL = -1


def test_entries_are_declared_bound_and_exported():
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    L = _lib.lib()
    for name in ("nh_run_ex", "nh_run_engine_ex"):
        assert name + "(" in hdr
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert "#define NH_ABI_VERSION 5" in hdr and L.nh_abi_version() == 5


def test_header_and_binding_agree_on_the_struct():
    """the struct of the header, compiled by the C compiler of the build, has the size and the offsets of the binding's"""
    from nohuman_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} nh_run_extras;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].replace("char", "").split(",")]
    assert names == [f[0] for f in _lib.nh_run_extras._fields_]
    assert C.sizeof(_lib.nh_run_extras) == 4 + 4 + 4 * C.sizeof(C.c_char_p) == 40
    assert _lib.nh_run_extras.human_out1.offset == 8 and _lib.nh_run_extras.human_ids.offset == 32
    # the library was built from that header: a struct_size one byte short is refused, the binding's size is not
    L = _lib.lib()
    a, s = _lib.nh_run_args(), _lib.nh_stats()
    x = _lib.nh_run_extras(struct_size=C.sizeof(_lib.nh_run_extras) - 1)
    assert L.nh_run_ex(C.byref(a), C.byref(x), C.byref(s)) == NH_EINVAL and b"struct_size" in L.nh_last_error()
    x.struct_size += 1
    assert L.nh_run_ex(C.byref(a), C.byref(x), C.byref(s)) == NH_EINVAL and b"struct_size" not in L.nh_last_error()


@pytest.fixture
def files(tmp_path):
    for n in ("a_1.fq", "a_2.fq"):
        (tmp_path / n).write_bytes(b"@r\nACGT\n+\nIIII\n")
    os.link(tmp_path / "a_1.fq", tmp_path / "link_to_input.fq")
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


def _extras(d, size=None, mask=0, h1=None, h2=None, calls=None, ids=None):
    from nohuman_amd import _lib
    x = _lib.nh_run_extras()
    x.struct_size = C.sizeof(_lib.nh_run_extras) if size is None else size
    x.mask = mask
    for k, v in (("human_out1", h1), ("human_out2", h2), ("calls", calls), ("human_ids", ids)):
        setattr(x, k, str(d / v).encode() if v else None)
    return x


def _bad_cases(d):
    """(why, args, extras, the offending path's name or None)"""
    cases = [("struct_size too small", _args(d), _extras(d, size=16, calls="c.txt"), "c.txt"),
             ("struct_size zero", _args(d), _extras(d, size=0, ids="i.txt"), "i.txt"),
             ("calls and human_ids the same", _args(d), _extras(d, calls="c.txt", ids="c.txt"), "c.txt")]
    for field in ("calls", "ids"):
        def ex(name, **kw):
            return _extras(d, **dict(kw, **{field: name}))
        cases += [
            (field + " names in1", _args(d), ex("a_1.fq"), None),
            (field + " names in2", _args(d, paired=True), ex("a_2.fq"), None),
            (field + " same inode as in1", _args(d), ex("link_to_input.fq"), None),
            (field + " names out1", _args(d), ex("o_1.fq"), "o_1.fq"),
            (field + " names out2", _args(d, paired=True), ex("o_2.fq"), "o_2.fq"),
            (field + " names kraken_output", _args(d), ex("k.txt"), "k.txt"),
            (field + " names report", _args(d), ex("r.txt"), "r.txt"),
            (field + " names human_out1", _args(d), ex("h_1.fq", h1="h_1.fq"), "h_1.fq"),
            (field + " names human_out2", _args(d, paired=True), ex("h_2.fq", h1="h_1.fq", h2="h_2.fq"), "h_2.fq"),
            (field + " names a masked run's human_out1", _args(d), ex("h_1.fq", mask=1, h1="h_1.fq"), "h_1.fq"),
            # the checks of nh_run_split / nh_run_mask for the fields they share
            (field + ": keep_human with a human output", _args(d, keep_human=1), ex("l.txt", h1="h_1.fq"), "l.txt"),
            (field + ": human_out2 without human_out1", _args(d, paired=True), ex("l.txt", h2="h_2.fq"), "l.txt"),
            (field + ": human_out2 without in2", _args(d), ex("l.txt", h1="h_1.fq", h2="h_2.fq"), "l.txt"),
            (field + ": in2 without human_out2", _args(d, paired=True), ex("l.txt", h1="h_1.fq"), "l.txt"),
            (field + ": human output names in1", _args(d), ex("l.txt", h1="a_1.fq"), "l.txt"),
            (field + ": human output names out1", _args(d), ex("l.txt", h1="o_1.fq"), "l.txt"),
            (field + ": mask with keep_human", _args(d, keep_human=1), ex("l.txt", mask=1), "l.txt"),
            (field + ": mask whose output names in1", _args(d, out1=str(d / "a_1.fq").encode()), ex("l.txt", mask=1), "l.txt"),
            (field + ": mask whose human output names report", _args(d), ex("l.txt", mask=1, h1="r.txt"), "l.txt"),
        ]
    return cases


def test_argument_errors_come_before_any_device(files):
    from nohuman_amd import _lib
    L = _lib.lib()
    s = _lib.nh_stats()
    before = {p.name: p.read_bytes() for p in files.iterdir()}
    for why, a, x, path in _bad_cases(files):
        for rc in (L.nh_run_ex(C.byref(a), C.byref(x), C.byref(s)), L.nh_run_engine_ex(None, C.byref(a), C.byref(x), C.byref(s))):
            assert rc == NH_EINVAL, (why, rc, L.nh_last_error())
        if path:
            assert not (files / path).exists(), why
    assert L.nh_run_ex(C.byref(_args(files)), None, C.byref(s)) == NH_EINVAL  # no extras at all
    assert {p.name: p.read_bytes() for p in files.iterdir()} == before  # nothing was created, no input touched


def test_python_keywords_reach_the_extended_entry(files):
    from nohuman_amd import Engine, EngineError, engine
    import inspect
    for fn in (engine.run, Engine.run):
        assert {"calls", "human_ids"} <= set(inspect.signature(fn).parameters)
    with pytest.raises(EngineError) as ei:
        engine.run(DB, str(files / "a_1.fq"), str(files / "o.fq"), calls=str(files / "c"), human_ids=str(files / "c"))
    assert ei.value.code == NH_EINVAL and "nh_run_ex" in ei.value.message
    with pytest.raises(EngineError) as ei:  # the other fields select the run: a split run's check
        engine.run(DB, str(files / "a_1.fq"), str(files / "o.fq"), keep_human=True, human_out1=str(files / "h.fq"), human_ids=str(files / "i"))
    assert ei.value.code == NH_EINVAL and "keep_human" in ei.value.message
    assert not (files / "c").exists() and not (files / "i").exists()


def test_runner_mirrors_the_flags():
    from nohuman_amd import CommandRunner
    o = CommandRunner.parse_argv(["--db", "d", "--calls", "c.tsv", "--human-ids", "i.txt", "--unclassified-out", "o.fq", "in.fq"])
    assert (o["calls"], o["human_ids"], o["inputs"]) == ("c.tsv", "i.txt", ["in.fq"])
    o = CommandRunner.parse_argv(["--db", "d", "in.fq"])
    assert o["calls"] is None and o["human_ids"] is None


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_help_lists_the_read_lists(files):
    r = _cli(["--help"])
    assert r.returncode == 0
    assert "--calls <FILE>" in r.stdout and "--human-ids <FILE>" in r.stdout
    c = str(files / "c.txt")
    r = _cli(["--calls", c, "--human-ids", c, str(files / "a_1.fq")])
    assert r.returncode == 2 and "--human-ids" in r.stderr and "dependencies" not in r.stderr
    assert not (files / "c.txt").exists() and not (files / "c.txt.partial").exists()
