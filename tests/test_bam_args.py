"""BAM input's argument checks and names: a BAM beside a second input is refused before any device is touched (so the refusal is
the same with and without a GPU), and the header, the binding and the Python surface agree on the two new entries.  No GPU."""
import ctypes as C
import os

import pytest

import nohuman_amd
from nohuman_amd import EngineError, _lib
from tests import bam_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture()
def files(tmp_path):
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bm.bgzf(bm.forge_header() + bm.forge_record(b"r1", b"ACGTACGT", bytes(8))))
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r1\nACGTACGT\n+\nIIIIIIII\n")
    return str(bam), str(fq), tmp_path


def test_bam_with_a_second_input_is_refused_before_any_device(files):
    bam, fq, tmp = files
    db = str(tmp / "no_such_db")  # (never opened: the refusal comes first)
    for in1, in2, what in ((bam, fq, "in1"), (fq, bam, "in2"), (bam, bam, "in2")):
        with pytest.raises(EngineError) as ei:
            nohuman_amd.engine.run(db, in1, str(tmp / "o1.fq"), in2=in2, out2=str(tmp / "o2.fq"))
        assert ei.value.code == EINVAL and "BAM" in ei.value.message and what in ei.value.message, ei.value.message
        assert not (tmp / "o1.fq").exists() and not (tmp / "o2.fq").exists()
    # every entry point of the family goes through the same check
    with pytest.raises(EngineError) as ei:
        nohuman_amd.engine.run(db, bam, str(tmp / "o1.fq"), in2=fq, out2=str(tmp / "o2.fq"), mask=True)
    assert ei.value.code == EINVAL and "BAM" in ei.value.message


def test_header_binding_and_python_names_agree():
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    for name in ("nh_bam_scan", "nh_bam_to_fastq_device"):
        assert name + "(" in hdr and name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
    assert len(_lib.SYMBOLS["nh_bam_scan"][1]) == 3 and len(_lib.SYMBOLS["nh_bam_to_fastq_device"][1]) == 10
    assert "#define NH_ABI_VERSION 5" in hdr and _lib.lib().nh_abi_version() == 5
    fields = [f for f, _ in _lib.nh_bam_info._fields_]
    assert fields == ["struct_size", "reserved", "records", "reads", "bases", "skipped_secondary", "skipped_empty", "reverse_complemented",
                      "missing_qualities", "digest"]
    assert C.sizeof(_lib.nh_bam_info) == 8 + 8 * 8
    for f in fields:
        assert f in hdr
    assert nohuman_amd.bam_scan is not None and "bam_scan" in nohuman_amd.__all__
    assert callable(nohuman_amd.Engine.bam_to_fastq_device)


def test_struct_size_and_null_arguments(files):
    bam = files[0]
    L = _lib.lib()
    info = _lib.nh_bam_info()
    info.struct_size = 8
    assert L.nh_bam_scan(os.fsencode(bam), 1, C.byref(info)) == EINVAL and b"struct_size" in L.nh_last_error()
    assert L.nh_bam_scan(None, 1, C.byref(info)) == EINVAL
    assert L.nh_bam_scan(os.fsencode(bam), 1, None) == EINVAL
    info.struct_size = C.sizeof(info)
    assert L.nh_bam_scan(os.fsencode(bam), 0, C.byref(info)) == 0 and (info.records, info.reads, info.bases) == (1, 1, 8)
