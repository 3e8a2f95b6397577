"""A paired BAM's argument checks: a paired BAM makes a paired run without an in2, and every refusal that follows from that comes
before any device is touched -- the same with and without a GPU --, creates nothing and names its reason; the header, the binding
and the Python surface agree; `nohuman` refuses what a paired BAM does not go with as argument errors and names its default
outputs `<stem>.nohuman_1.fq[.ext]` / `<stem>.nohuman_2.fq[.ext]`.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import nohuman_amd
from nohuman_amd import EngineError, _lib, engine
from tests import bam_model as bm
from tests import bam_pair_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
EINVAL = -1


@pytest.fixture()
def files(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    pair = b"".join(pm.forge_pair(b"p1", b"ACGTACGT", b"TTGCA", bytes(8), bytes(5), rev=(0, 1)))
    (d / "pairs.bam").write_bytes(bm.bgzf(bm.forge_header() + pair))
    (d / "single.bam").write_bytes(bm.bgzf(bm.forge_header() + bm.forge_record(b"r1", b"ACGTACGT", bytes(8))))
    (d / "reads.fq").write_bytes(b"@r1\nACGTACGT\n+\nIIIIIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    return d, out


def _refused(out, *words, **kw):
    """engine.run on a database that is never opened -> the message of the refusal"""
    with pytest.raises(EngineError) as ei:
        engine.run(str(out / "no_such_db"), kw.pop("in1"), str(out / "o"), **kw)
    assert ei.value.code == EINVAL, ei.value.message
    for w in words:
        assert w in ei.value.message, ei.value.message
    assert os.listdir(out) == [], os.listdir(out)
    return ei.value.message


def test_a_paired_bam_is_a_paired_run_and_is_checked_as_one(files):
    d, out = files
    pairs, single, fq = str(d / "pairs.bam"), str(d / "single.bam"), str(d / "reads.fq")
    o2, h1, h2 = str(out / "o2"), str(out / "h1"), str(out / "h2")
    assert nohuman_amd.bam_paired(pairs) and not nohuman_amd.bam_paired(single)
    # beside an in2, as in1 or as in2: today's messages
    _refused(out, "is a BAM file and in2 is given", in1=pairs, in2=fq, out2=o2)
    _refused(out, "in2", "is a BAM file", in1=fq, in2=pairs, out2=o2)
    # a FASTQ codec: the second mate needs its files
    for codec in (0, 2, 5):
        _refused(out, "paired input needs out2", in1=pairs, out_codec=codec)
        _refused(out, "paired input needs human_out2", in1=pairs, out2=o2, human_out1=h1, out_codec=codec)
        _refused(out, "paired input needs human_out2", in1=pairs, out2=o2, human_out1=h1, mask=True, out_codec=codec)
        _refused(out, "paired input needs outs[0].out2", in1=pairs, out2=o2, taxon_outs=[(9606, str(out / "t1"), None)], out_codec=codec)
    # BAM output: one BAM holds both mates
    _refused(out, "out_codec 6", "out2", "one BAM file holds both mates", in1=pairs, out2=o2, out_codec=engine.CODEC_BAM)
    _refused(out, "out_codec 6", "human_out2", "one BAM file holds both mates", in1=pairs, human_out1=h1, human_out2=h2, out_codec=engine.CODEC_BAM)
    # ... and what BAM output never went with stays refused, with its own words
    _refused(out, "out_codec 6", "masked run", in1=pairs, mask=True, out_codec=engine.CODEC_BAM)
    _refused(out, "out_codec 6", "per-taxon outputs", in1=pairs, taxon_outs=[(9606, str(out / "t.bam"), str(out / "t2.bam"))], out_codec=engine.CODEC_BAM)
    # a single-end BAM is checked as it was: a second human output has nothing to go with
    _refused(out, "human_out2 is given without in2", in1=single, human_out1=h1, human_out2=h2)


def test_good_requests_get_as_far_as_the_engine(files):
    d, out = files
    L = _lib.lib()
    st = _lib.nh_stats()
    a = _lib.nh_run_args()
    a.in1, a.out1, a.out2, a.n_devices = os.fsencode(str(d / "pairs.bam")), os.fsencode(str(out / "o1")), os.fsencode(str(out / "o2")), 1
    assert L.nh_run_engine(None, C.byref(a), C.byref(st)) == EINVAL and L.nh_last_error() == b"null engine"
    assert L.nh_run_engine_split(None, C.byref(a), os.fsencode(str(out / "h1")), os.fsencode(str(out / "h2")), C.byref(st)) == EINVAL
    assert L.nh_last_error() == b"null engine"
    assert L.nh_run_engine_split(None, C.byref(a), os.fsencode(str(out / "h1")), None, C.byref(st)) == EINVAL
    assert b"paired input needs human_out2" in L.nh_last_error()
    a.out2, a.out_codec = None, 6
    assert L.nh_run_engine(None, C.byref(a), C.byref(st)) == EINVAL and L.nh_last_error() == b"null engine"
    assert L.nh_run_engine_split(None, C.byref(a), os.fsencode(str(out / "h.bam")), None, C.byref(st)) == EINVAL
    assert L.nh_last_error() == b"null engine"
    a.out_codec = 0
    assert L.nh_run_engine(None, C.byref(a), C.byref(st)) == EINVAL and b"paired input needs out2" in L.nh_last_error()
    assert os.listdir(out) == []


def test_header_binding_and_python_names_agree():
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    for name, nargs in (("nh_bam_scan_pairs", 4), ("nh_bam_paired", 1), ("nh_bam_select_pairs_device", 12)):
        assert name + "(" in hdr and len(_lib.SYMBOLS[name][1]) == nargs and getattr(_lib.lib(), name) is not None
    assert C.sizeof(_lib.nh_bam_pair_info) == 48 and C.sizeof(_lib.nh_bam_info) == 72  # (nh_bam_info keeps its layout)
    assert C.sizeof(_lib.nh_run_args) == 96 and C.sizeof(_lib.nh_run_extras) == 40
    assert callable(nohuman_amd.bam_scan_pairs) and callable(nohuman_amd.bam_paired) and callable(nohuman_amd.Engine.bam_select_pairs_device)
    info = _lib.nh_bam_info()
    pinfo = _lib.nh_bam_pair_info()
    info.struct_size, pinfo.struct_size = C.sizeof(info), 47
    assert _lib.lib().nh_bam_scan_pairs(b"/nonexistent", 1, C.byref(info), C.byref(pinfo)) == EINVAL
    assert b"nh_bam_pair_info" in _lib.lib().nh_last_error()
    assert _lib.lib().nh_bam_scan_pairs(b"/nonexistent", 1, C.byref(info), None) == EINVAL
    for word in ("Paired BAM", "samtools collate", "samtools fastq -n -1 -2"):
        assert word in hdr, word
    assert "single-end:" not in hdr  # (BAM input is no longer said to be single-end)


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


def test_cli_argument_errors_and_default_names(files):
    assert os.path.exists(BIN), "the CLI host is not built"
    d, out = files
    pairs, single, fq = str(d / "pairs.bam"), str(d / "single.bam"), str(d / "reads.fq")
    h = _cli(["--help"])
    assert h.returncode == 0 and "collated pairs" in h.stdout and "samtools collate" in h.stdout

    def refused(args, *words):
        r = _cli(["--db", str(out / "no_such_db")] + args)
        assert r.returncode == 2 and r.stderr.startswith("error: ") and "try '--help'" in r.stderr, (args, r.stderr)
        for w in words:
            assert w in r.stderr, (args, r.stderr)
    refused(["--bam-out", "-O", str(out / "o2.bam"), pairs], "--bam-out", "--out2", "one BAM file holds both mates")
    refused(["--bam-out", "--human-out1", str(out / "h1.bam"), "--human-out2", str(out / "h2.bam"), pairs], "--bam-out", "--human-out2")
    refused(["--bam-out", pairs, fq], "--bam-out", "two inputs")
    # a paired BAM wants what two inputs want
    refused(["--human-out1", str(out / "h1.fq"), pairs], "--human-out2 <PATH>")
    refused(["--taxon-out", "9606:" + str(out / "t.fq"), pairs], "--taxon-out", "'#'")
    # ... and a single-end BAM what one input wants
    refused(["--human-out1", str(out / "h1.fq"), "--human-out2", str(out / "h2.fq"), single], "--human-out2 <PATH>", "needs two inputs")
    refused(["--taxon-out", "9606:" + str(out / "t#.fq"), single], "--taxon-out", "'#'")
    # the default names: a human output that names one of them is an argument error that spells it
    for mate in (1, 2):
        name = str(d / ("pairs.nohuman_%d.fq.gz" % mate))
        refused(["--human-out1", name if mate == 1 else str(out / "h1.fq"), "--human-out2", name if mate == 2 else str(out / "h2.fq"), pairs],
                "names the same file as the output", "pairs.nohuman_%d.fq.gz" % mate)
    refused(["-F", "u", "--human-out1", str(d / "pairs.nohuman_1.fq"), "--human-out2", str(out / "h2.fq"), pairs], "pairs.nohuman_1.fq")
    refused(["--bam-out", "--human-out1", str(d / "pairs.nohuman.bam"), pairs], "pairs.nohuman.bam")
    refused(["--human-out1", str(d / "single.nohuman.fq.gz"), single], "single.nohuman.fq.gz")  # (a single-end BAM's is what it was)
    # without a conflict nothing is an argument error: the run gets as far as its device or its database (neither is there)
    for args in (["-o", str(out / "o1.fq"), "-O", str(out / "o2.fq"), pairs], [pairs], ["--bam-out", pairs],
                 ["--bam-out", "--human-out1", str(out / "h.bam"), pairs],
                 ["--human-out1", str(out / "h1.fq"), "--human-out2", str(out / "h2.fq"), "--taxon-out", "9606:" + str(out / "t#.fq"), pairs]):
        r = _cli(["--db", str(out / "no_such_db")] + args)
        assert r.returncode == 1 and not r.stderr.startswith("error: "), (args, r.stderr)
    assert os.listdir(out) == [] and sorted(os.listdir(d)) == ["pairs.bam", "reads.fq", "single.bam"]
