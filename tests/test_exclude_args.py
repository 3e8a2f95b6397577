"""nh_build_db_exclude / nh_exclude_check / `nohuman --build-db OUT --exclude FILE` without a device: the two new symbols and
structs, every refusal (through nh_exclude_check and nh_build_db_exclude: the code, a message that names the reason, out_dir as it
was), the call without a list, the CLI's usage errors and the forms engine.build_db takes the list in.
tests/test_gpu_build_db_exclude.py builds."""
import ctypes as C
import os
import re
import subprocess

import pytest

import nohuman_amd
from nohuman_amd import EngineError, _lib
from nohuman_amd.runner import CommandRunner
from tests import build_taxa_util as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
EINVAL, EIO, EDB, EDEVICE = -1, -2, -3, -4
FASTA = b">chr1\n" + b"ACGTTGCAAGGCTTAACCGGTTACGATCGATTGCA" * 4 + b"\n"


@pytest.fixture
def env(tmp_path):
    for name in ("host.fa", "host2.fa", "x.fa", "y.fa"):
        (tmp_path / name).write_bytes(FASTA)
    return tmp_path


def call(fn, out_dir, host=(), exclude=(), taxa=None, x_size=None, xs_size=None, null_x=False, null_xs=False, null_list=False, **kw):
    """nh_build_db_exclude or nh_exclude_check through ctypes, on a device no machine has -> (code, message, build stats,
    exclude stats)"""
    a, s, keep = t.raw_args(taxa, out_dir, [str(p) for p in host], **kw)
    x = _lib.nh_exclude_args()
    x.struct_size = C.sizeof(x) if x_size is None else x_size
    arr = (C.c_char_p * max(len(exclude), 1))(*[None if p is None else os.fsencode(str(p)) for p in exclude])
    x.n_fasta = len(exclude)
    if not null_list:
        x.fasta = arr
    xs = _lib.nh_exclude_stats()
    xs.struct_size = C.sizeof(xs) if xs_size is None else xs_size
    rc = getattr(_lib.lib(), fn)(C.byref(a), None if null_x else C.byref(x), C.byref(s), None if null_xs else C.byref(xs))
    return rc, _lib.lib().nh_last_error().decode(errors="replace"), s, xs


def both(*args, **kw):
    """the call through nh_exclude_check and nh_build_db_exclude: one code, one message -> (code, message)"""
    rc, msg, *_ = call("nh_exclude_check", *args, **kw)
    rc2, msg2, *_ = call("nh_build_db_exclude", *args, **kw)
    assert (rc, msg) == (rc2, msg2)
    return rc, msg


def test_header_binding_and_struct_sizes():
    header = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    for name in ("nh_build_db_exclude", "nh_exclude_check"):
        assert re.search(r"\bint %s\(const nh_build_args \*b, const nh_exclude_args \*x, nh_build_stats \*bs, nh_exclude_stats \*xs\);" % name, header)
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == 4 and getattr(_lib.lib(), name) is not None
    X, S = _lib.nh_exclude_args, _lib.nh_exclude_stats
    assert C.sizeof(X) == 16 and (X.struct_size.offset, X.n_fasta.offset, X.fasta.offset) == (0, 4, 8)
    assert C.sizeof(S) == 80 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    assert [n for n, _ in S._fields_] == ["struct_size", "reserved", "sequences", "bases", "kmers", "ambiguous_kmers", "lookups",
                                          "excluded_minimizers", "kept_minimizers", "seconds_read", "seconds_exclude"]
    assert "#define NH_ABI_VERSION 5" in header and _lib.lib().nh_abi_version() == 5
    # no existing struct has changed
    assert (C.sizeof(_lib.nh_build_args), C.sizeof(_lib.nh_build_args_v2), C.sizeof(_lib.nh_build_args_v3)) == (80, 88, 112)
    assert (C.sizeof(_lib.nh_build_stats), C.sizeof(_lib.nh_build_stats_v2), C.sizeof(_lib.nh_build_stats_v3)) == (88, 104, 112)
    assert C.sizeof(_lib.nh_extend_args) == 24 and C.sizeof(_lib.nh_extend_stats) == 80 and C.sizeof(_lib.nh_build_taxon_stats) == 40


def test_arguments_refused_before_any_device(env):
    out = env / "out"
    host, x, y = env / "host.fa", env / "x.fa", env / "y.fa"
    assert call("nh_exclude_check", str(out), [host], [x, y])[0] == 0
    os.symlink(str(x), str(env / "x_again.fa"))
    os.symlink(str(host), str(env / "host_again.fa"))
    cases = {
        "exclude args too small": (dict(x_size=8), "struct_size 8 is smaller than nh_exclude_args"),
        "exclude stats too small": (dict(xs_size=72), "struct_size 72 is smaller than nh_exclude_stats"),
        "exclude stats too small, an empty list": (dict(xs_size=72, exclude=[]), "struct_size 72 is smaller than nh_exclude_stats"),
        "a null list": (dict(null_list=True), "fasta is null"),
        "a null path": (dict(exclude=[x, None]), "exclusion file 1 is a null path"),
        "the file twice": (dict(exclude=[x, y, x]), "x.fa is given twice"),
        "the file twice, by a link": (dict(exclude=[x, env / "x_again.fa"]), "x_again.fa is given twice"),
        "a host input": (dict(exclude=[x, host]), "host.fa is also an input of the build"),
        "a host input, by a link": (dict(exclude=[env / "host_again.fa"]), "host_again.fa is also an input of the build"),
        "a host input, by another spelling": (dict(exclude=[str(env) + "/./host.fa"]), "is also an input of the build"),
        # whatever nh_build_db refuses
        "args too small": (dict(struct_size=40), "struct_size 40"),
        "no host input": (dict(host=[]), "no input"),
        "load factor": (dict(load_factor=0.96), "load factor"),
        "taxid 1": (dict(taxid=1), "taxid 1"),
        "capacity": (dict(capacity=1 << 33), "is not below 2^33"),
    }
    for name, (kw, what) in cases.items():
        kw = dict(dict(out_dir=str(out), host=[host], exclude=[x]), **kw)
        rc, msg = both(**kw)
        assert rc == EINVAL and what in msg, (name, rc, msg)
        assert not out.exists(), name
    # a database already in out_dir needs `force`, as ever; an exclusion file that IS one of its files is refused whatever `force` says
    out.mkdir()
    for name in ("hash.k2d", "opts.k2d", "taxo.k2d"):
        (out / name).write_bytes(FASTA)
    before = {n: (out / n).read_bytes() for n in os.listdir(out)}
    rc, msg = both(str(out), [host], [x])
    assert rc == EINVAL and "force" in msg
    rc, msg = both(str(out), [host], [out / "opts.k2d"], force=1)
    assert rc == EINVAL and "opts.k2d is a database file of the output directory" in msg
    os.link(str(out / "taxo.k2d"), str(env / "elsewhere.fa"))
    rc, msg = both(str(out), [host], [env / "elsewhere.fa"], force=1)
    assert rc == EINVAL and "elsewhere.fa is a database file of the output directory" in msg
    assert call("nh_exclude_check", str(out), [host], [x], force=1)[0] == 0
    assert before == {n: (out / n).read_bytes() for n in os.listdir(out)}


def test_a_manifest_fasta_is_no_exclusion_file(env):
    out = env / "out"
    m = t.write_manifest(env / "taxa.tsv", [(40, 1, "D", "host.fa"), (50, 1, "E", "host2.fa")])
    rc, msg, s, _ = call("nh_exclude_check", str(out), [], [env / "x.fa"], taxa=m)
    assert rc == 0 and s.taxa == 3, msg
    rc, msg = both(str(out), [], [env / "x.fa", env / "host2.fa"], taxa=m)
    assert rc == EINVAL and "host2.fa is also an input of the build" in msg and not out.exists()
    bad = t.write_manifest(env / "bad.tsv", [(40, 41, "D", "host.fa")])
    rc, msg = both(str(out), [], [env / "x.fa"], taxa=bad)
    assert rc == EINVAL and "line 1:" in msg and not out.exists()


def test_without_a_list_it_is_nh_build_db(env):
    out = env / "out"
    host = [env / "host.fa"]
    want = t.raw_call("nh_build_check", None, str(out), [str(h) for h in host])[:2]
    for kw in (dict(null_x=True), dict(exclude=[]), dict(null_x=True, null_xs=True), dict(exclude=[], null_list=True)):
        rc, msg, *_ = call("nh_exclude_check", str(out), host, **kw)
        assert rc == want[0] == 0, (kw, msg)
        rc, msg, *_ = call("nh_build_db_exclude", str(out), host, **kw)
        assert rc == EDEVICE and not out.exists(), (kw, msg)  # (every check passed: the device is asked for, and there is none)
    bad = t.raw_call("nh_build_check", None, str(out), [str(h) for h in host], taxid=1)[:2]
    for fn in ("nh_exclude_check", "nh_build_db_exclude"):
        assert call(fn, str(out), host, null_x=True, taxid=1)[:2] == bad and bad[0] == EINVAL
    # with a list: past every check, the device
    rc, msg, *_ = call("nh_build_db_exclude", str(out), host, [env / "x.fa", env / "y.fa"])
    assert rc == EDEVICE and not out.exists(), msg
    # an exclusion file that is not there: NH_EIO with its name, before the host is counted
    rc, msg, *_ = call("nh_build_db_exclude", str(out), host, [env / "x.fa", env / "missing.fa"])
    assert rc == EIO and "missing.fa" in msg and not out.exists(), msg


def test_python_argument_forms(env):
    out = env / "out"
    host = env / "host.fa"
    # what is given reaches the library: a host input as an exclusion file is refused, in every form the list takes
    for form in (str(host), host, os.fsencode(str(host)), [host], [env / "x.fa", str(host)], (str(host),)):
        with pytest.raises(EngineError) as ei:
            nohuman_amd.build_db([host], out, exclude=form, device=t.NO_DEVICE)
        assert ei.value.code == EINVAL and "also an input of the build" in ei.value.message, form
    # a list that is fine, an empty one and none: the device
    for form in (env / "x.fa", [env / "x.fa", env / "y.fa"], [], (), None):
        with pytest.raises(EngineError) as ei:
            nohuman_amd.build_db([host], out, exclude=form, device=t.NO_DEVICE)
        assert ei.value.code == EDEVICE, form
    assert not out.exists()
    import inspect
    assert inspect.signature(nohuman_amd.build_db).parameters["exclude"].default is None
    assert "exclude" not in inspect.signature(nohuman_amd.extend_db).parameters


def _cli(*args):
    p = subprocess.run([BIN] + list(args), capture_output=True, timeout=120)
    return p.returncode, p.stdout.decode(errors="replace"), p.stderr.decode(errors="replace")


def test_cli_usage_errors(env):
    reads = env / "reads.fq"
    reads.write_bytes(b"@r\nACGT\n+\nIIII\n")
    d = str(env / "db")
    host, x = str(env / "host.fa"), str(env / "x.fa")
    m = t.write_manifest(env / "taxa.tsv", [(40, 1, "D", "host.fa")])
    base = env / "base"
    base.mkdir()
    for args, what in ((("--exclude", x, str(reads)), "'--exclude <FILE>' needs '--build-db <DIR>'"),
                       (("--exclude", x, "--reference", host), "needs '--build-db <DIR>'"),
                       (("--build-db", d, "--reference", host, "--exclude"), "--exclude"),
                       (("--build-db", d, "--reference", host, "--exclude", str(env / "nowhere.fa")), "does not exist"),
                       (("--build-db", d, "--reference", host, "--exclude", x, "--extend-db", str(base)),
                        "'--exclude <FILE>' cannot be used with '--extend-db <DIR>'"),
                       (("--build-db", d, "--taxa", m, "--exclude", x, "--extend-db", str(base)), "cannot be used with '--extend-db <DIR>'"),
                       (("--build-db", d, "--reference", host, "--exclude", x, "--exclude", x), "given twice"),
                       (("--build-db", d, "--reference", host, "--exclude", host), "also an input of the build"),
                       (("--build-db", d, "--taxa", m, "--exclude", host), "also an input of the build"),
                       (("--build-db", d, "--reference", host, "--exclude", x, "--taxid", "1"), "taxid 1"),
                       (("--build-db", d, "--reference", host, "--exclude", x, str(reads)), "read inputs")):
        rc, _, err = _cli(*args)
        assert rc == 2 and err.startswith("error: ") and "try '--help'" in err and what in err, (args, rc, err)
        assert "dependencies" not in err and not os.path.exists(d), args
    # what passes every check ends at the device probe (or builds, where there is a device)
    rc, _, err = _cli("--build-db", d, "--reference", host, "--exclude", x, "--exclude", str(env / "y.fa"))
    assert (rc != 2 or "dependencies" in err) and not os.path.exists(d) or nohuman_amd.device_count() > 0


def test_cli_help_has_one_line_for_the_flag():
    rc, out, _ = _cli("--help")
    assert rc == 0
    lines = [ln for ln in out.split("\n") if "--exclude" in ln]
    assert len(lines) == 1 and "--exclude <FILE>" in lines[0]
    for other in ("--build-db", "--reference", "--taxid", "--taxon-name", "--load-factor", "--capacity", "--force", "--mask", "--db ", "--taxa",
                  "--extend-db"):
        assert other not in lines[0], other


def test_the_runner_mirror_knows_the_flag():
    o = CommandRunner.parse_argv(["--db", "d", "--exclude", "a.fa", "--exclude", "b.fa", "reads.fq"])
    assert o["exclude"] == ["a.fa", "b.fa"] and o["inputs"] == ["reads.fq"] and o["db"] == "d"
    assert CommandRunner.parse_argv(["--db", "d", "reads.fq"])["exclude"] == []
    with pytest.raises(OSError) as ei:
        CommandRunner().run(["--db", "d", "--exclude", "a.fa", "--unclassified-out", "o.fq", "reads.fq"])
    assert "--exclude needs --build-db" in str(ei.value)
