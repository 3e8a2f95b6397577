"""BAM output's argument checks and names (NH_CODEC_BAM = 6): every refusal comes before any device is touched -- the same with and
without a GPU -- creates nothing and names its reason; the host compress stage refuses the codec; the header, the binding and the
Python surface agree; `nohuman --bam-out` refuses what it does not go with as the CLI refuses everything else.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import nohuman_amd
from nohuman_amd import EngineError, _lib, engine
from tests import bam_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
EINVAL = -1


@pytest.fixture()
def files(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    (d / "reads.bam").write_bytes(bm.bgzf(bm.forge_header() + bm.forge_record(b"r1", b"ACGTACGT", bytes(8), tags=b"MMZC+m,1;\0")))
    (d / "reads.fq").write_bytes(b"@r1\nACGTACGT\n+\nIIIIIIII\n")
    (d / "reads.fq.gz").write_bytes(bm.bgzf(b"@r1\nACGTACGT\n+\nIIIIIIII\n"))  # (BGZF, but no BAM inside)
    out = tmp_path / "out"
    out.mkdir()
    return d, out


def _refused(out, *words, **kw):
    """engine.run on a database that is never opened -> the message of the refusal"""
    with pytest.raises(EngineError) as ei:
        engine.run(str(out / "no_such_db"), kw.pop("in1"), str(out / "o.bam"), out_codec=kw.pop("codec", engine.CODEC_BAM), **kw)
    assert ei.value.code == EINVAL, ei.value.message
    for w in words:
        assert w in ei.value.message, ei.value.message
    assert os.listdir(out) == [], os.listdir(out)
    return ei.value.message


def test_codec_6_is_refused_where_it_cannot_work_before_any_device(files):
    d, out = files
    bam, fq = str(d / "reads.bam"), str(d / "reads.fq")
    assert engine.CODEC_BAM == 6
    # an in1 that is not a BAM: plain FASTQ, BGZF FASTQ, a file that is not there
    for in1 in (fq, str(d / "reads.fq.gz"), str(d / "nope.bam")):
        _refused(out, "out_codec 6", "not a BAM file", os.path.basename(in1), in1=in1)
    # a second input
    _refused(out, "out_codec 6", "in2", "single-end", in1=bam, in2=fq, out2=str(out / "o2.bam"))
    # a masked run, per-taxon outputs: each with its own words
    m = _refused(out, "out_codec 6", "masked run", in1=bam, mask=True)
    t = _refused(out, "out_codec 6", "per-taxon outputs", in1=bam, taxon_outs=[(9606, str(out / "t.bam"), None)])
    assert "per-taxon" not in m and "masked" not in t
    # with the other outputs of a run around it, and a split run: the same refusal of a FASTQ in1
    _refused(out, "not a BAM file", in1=fq, human_out1=str(out / "h.bam"), calls=str(out / "c.tsv"), read_stats=str(out / "s.tsv"),
             host_taxids=[9606])
    # a codec there is none of keeps its message
    assert _refused(out, in1=bam, codec=99) == "nh_run: unknown out_codec 99"
    assert _refused(out, in1=fq, codec=7) == "nh_run: unknown out_codec 7"
    assert _refused(out, in1=fq, codec=-1) == "nh_run: unknown out_codec -1"


def test_the_engine_entries_check_the_same_before_they_look_at_the_engine(files):
    d, out = files
    L = _lib.lib()
    a = _lib.nh_run_args()
    a.in1, a.out1, a.out_codec, a.n_devices = os.fsencode(str(d / "reads.fq")), os.fsencode(str(out / "o.bam")), 6, 1
    st = _lib.nh_stats()
    assert L.nh_run_engine(None, C.byref(a), C.byref(st)) == EINVAL and b"not a BAM file" in L.nh_last_error()
    assert L.nh_run_engine_split(None, C.byref(a), os.fsencode(str(out / "h.bam")), None, C.byref(st)) == EINVAL
    assert b"not a BAM file" in L.nh_last_error()
    a.in1 = os.fsencode(str(d / "reads.bam"))
    assert L.nh_run_engine_mask(None, C.byref(a), None, None, C.byref(st)) == EINVAL and b"masked run" in L.nh_last_error()
    # a good request gets as far as the engine
    assert L.nh_run_engine(None, C.byref(a), C.byref(st)) == EINVAL and L.nh_last_error() == b"null engine"
    a.out_codec = 99
    assert L.nh_run_engine(None, C.byref(a), C.byref(st)) == EINVAL and L.nh_last_error() == b"nh_run: unknown out_codec 99"
    assert os.listdir(out) == []


def test_the_host_compress_stage_refuses_codec_6(files):
    d, out = files
    L = _lib.lib()
    src, dst = os.fsencode(str(d / "reads.fq")), os.fsencode(str(out / "x.bam"))
    assert L.nh_compress_file(src, dst, 6, 2) == EINVAL
    assert b"cannot be made a BAM" in L.nh_last_error()
    assert L.nh_compress_file_device(src, dst, 6, 2, 0) == EINVAL
    assert b"cannot be made a BAM" in L.nh_last_error()
    assert L.nh_compress_file(src, dst, 99, 2) == EINVAL and b"unknown codec 99" in L.nh_last_error()
    assert os.listdir(out) == []
    assert L.nh_compress_file(src, dst, 5, 2) == 0  # (codec 5 is untouched)


def test_header_binding_and_python_names_agree():
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    assert "NH_CODEC_BAM = 6" in hdr and "NH_CODEC_BGZF = 5" in hdr
    assert "nh_bam_select_device(" in hdr and len(_lib.SYMBOLS["nh_bam_select_device"][1]) == 12
    assert getattr(_lib.lib(), "nh_bam_select_device") is not None
    assert "#define NH_ABI_VERSION 5" in hdr and _lib.lib().nh_abi_version() == 5
    assert C.sizeof(_lib.nh_run_args) == 96 and C.sizeof(_lib.nh_run_extras) == 40  # (no struct changes size)
    assert callable(nohuman_amd.Engine.bam_select_device)
    for word in ("no @PG line", "NOWHERE", "cannot be made a BAM"):
        assert word in hdr, word


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


def test_cli_bam_out_conflicts_are_argument_errors(files):
    assert os.path.exists(BIN), "the CLI host is not built"
    d, out = files
    bam, fq = str(d / "reads.bam"), str(d / "reads.fq")
    h = _cli(["--help"])
    assert h.returncode == 0 and "--bam-out" in h.stdout and "@PG" in h.stdout and "--bgzf" in h.stdout

    def refused(args, *words):
        r = _cli(["--db", str(out / "no_such_db"), "--bam-out"] + args)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and "try '--help'" in r.stderr, (args, r.stderr)
        for w in ("--bam-out",) + words:
            assert w in r.stderr, (args, r.stderr)
    refused(["-F", "g", bam], "--output-type")
    refused(["--bgzf", bam], "--bgzf")
    refused(["--mask", bam], "--mask")
    refused(["--taxon-out", "9606:" + str(out / "t.bam"), bam], "--taxon-out")
    refused([bam, fq], "two inputs")
    refused([fq], "needs a BAM input", "reads.fq")
    refused([str(d / "reads.fq.gz")], "needs a BAM input")
    # without a conflict the flag is no argument error: the run gets as far as its device or its database (neither is there)
    r = _cli(["--db", str(out / "no_such_db"), "--bam-out", "--human-out1", str(out / "h.bam"), "-o", str(out / "o.bam"), bam])
    assert r.returncode == 1 and not r.stderr.startswith("error: "), r.stderr
    assert os.listdir(out) == [] and sorted(os.listdir(d)) == ["reads.bam", "reads.fq", "reads.fq.gz"]
