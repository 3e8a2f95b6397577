"""nh_bam_scan -- the host side of the BAM reader (nohuman_amd/csrc/nh_bam.cpp: the record chain, its validation, the scalar
transcoder) -- against tests/bam_model.py: counts and digest of the forged corpus, the same stream framed as BGZF members of 64,
1000 and 65280 bytes with the window filled a few bytes at a time (so that every field is cut at every offset), with and
without bgzip's EOF member, every refusal by code and message, and files that are no BAM.  No GPU."""
import gzip
import os
import struct
import subprocess
import sys

import pytest

import nohuman_amd
from nohuman_amd import EngineError
from tests import bam_model as bm
from tests import record_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EIO = -1, -2


def model_digest(text):
    """nh_fastx_scan's digest of a canonical FASTQ text"""
    lines = text.split(b"\n")
    parts = []
    for i in range(0, len(lines) - 1, 4):
        parts += [lines[i], lines[i + 1], lines[i + 3]]
    return rm.fnv(parts)


@pytest.fixture(scope="module")
def corpus():
    stream = bm.corpus_stream()
    text, counts, _, _ = bm.to_fastq(stream)
    return stream, text, counts, model_digest(text)


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_counts_and_digest_of_the_corpus(tmp_path, corpus):
    stream, text, counts, digest = corpus
    info = nohuman_amd.bam_scan(write(tmp_path, "c.bam", bm.bgzf(stream)))
    assert info[:7] == tuple(counts)
    assert info.digest == digest
    # the same digest nh_fastx_scan gives the FASTQ the model transcodes the file to
    import ctypes as C
    from nohuman_amd import _lib
    n, nb, dg = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert _lib.lib().nh_fastx_scan(os.fsencode(write(tmp_path, "c.fq", text)), C.byref(n), C.byref(nb), C.byref(dg)) == 0
    assert (n.value, nb.value, dg.value) == (counts.reads, counts.bases, info.digest)


SCAN = """
import sys
import nohuman_amd
for p in sys.argv[1:]:
    print(*nohuman_amd.bam_scan(p, threads=2))
"""


@pytest.mark.parametrize("chunk", [1, 7, 4096])
def test_every_framing_and_every_cut(tmp_path, corpus, chunk):
    """members of 64, 1000 and 65280 inflated bytes, with and without the EOF member, the chain's window filled `chunk` bytes at a
    time: block_size fields, fixed parts, names and bases all straddle reads of the source"""
    stream, _, counts, digest = corpus
    paths = [write(tmp_path, "m%d_%d.bam" % (m, eof), bm.bgzf(stream, m, bool(eof))) for m in (64, 1000, 65280) for eof in (1, 0)]
    env = dict(os.environ, NOHUMAN_BAM_CHUNK=str(chunk), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", SCAN] + paths, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = " ".join(str(x) for x in tuple(counts) + (digest,))
    assert r.stdout.split("\n")[:-1] == [want] * len(paths)


def _bad_files():
    hdr = bm.forge_header(refs=[(b"chr1", 100)])
    good = bm.forge_record(b"ok", b"ACGT", bytes(4))
    rec = bytearray(bm.forge_record(b"name", b"ACGTACGT", bytes(8)))
    out = {}
    out["negative l_text"] = (b"BAM\1" + struct.pack("<i", -5), "negative l_text")
    out["negative n_ref"] = (b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", -1), "negative n_ref")
    r = bytearray(rec)
    r[4 + 8] = 0
    out["l_read_name 0"] = (hdr + good + bytes(r), "record 2: l_read_name is 0")
    r = bytearray(rec)
    r[36 + 4] = ord("x")
    out["no NUL"] = (hdr + good + good + bytes(r), "record 3: the read name is not NUL-terminated")
    r = bytearray(rec)
    struct.pack_into("<I", r, 4 + 16, 9)  # l_seq 9: one more quality byte and half a packed byte more than block_size holds
    out["block_size"] = (hdr + bytes(r), "record 1: block_size")
    r = bytearray(rec)
    struct.pack_into("<i", r, 0, 31)
    out["block_size below 32"] = (hdr + good + bytes(r), "record 2: block_size 31")
    out["ends in header"] = (hdr[:len(hdr) - 3], "ends inside the header")
    out["ends in header text"] = (hdr[:10], "ends inside the header")
    out["ends in block_size"] = (hdr + good + bytes(rec[:2]), "ends inside record 2")
    out["ends in fixed part"] = (hdr + good + bytes(rec[:30]), "ends inside record 2")
    out["ends in record"] = (hdr + good + bytes(rec[:-1]), "ends inside record 2")
    out["paired"] = (hdr + good + bm.forge_record(b"mate", b"ACGT", bytes(4), flag=bm.PAIRED | 0x40), "record 2 (mate) is paired")
    out["line feed in name"] = (hdr + bm.forge_record(b"a\nb", b"ACGT", bytes(4)), "record 1: the read name")
    return out


BAD = _bad_files()


@pytest.mark.parametrize("case", sorted(BAD))
def test_refusals(tmp_path, case):
    data, message = BAD[case]
    with pytest.raises(bm.BamError):
        bm.records(data)  # (the model refuses it as well)
    for eof in (True, False):
        with pytest.raises(EngineError) as ei:
            nohuman_amd.bam_scan(write(tmp_path, "bad.bam", bm.bgzf(data, 1000, eof)))
        assert ei.value.code == EIO and message in ei.value.message, ei.value.message
    if case == "paired":
        assert "samtools fastq -1" in ei.value.message


def test_a_damaged_member_is_an_io_error(tmp_path, corpus):
    raw = bytearray(bm.bgzf(corpus[0], 1000))
    raw[len(raw) // 2] ^= 0x55
    with pytest.raises(EngineError) as ei:
        nohuman_amd.bam_scan(write(tmp_path, "damaged.bam", bytes(raw)))
    assert ei.value.code == EIO


def test_skipped_records_only(tmp_path):
    stream = bm.forge_header() + bm.forge_record(b"s", b"ACGT", bytes(4), flag=bm.SECONDARY) + bm.forge_record(b"e", b"", b"")
    info = nohuman_amd.bam_scan(write(tmp_path, "skipped.bam", bm.bgzf(stream)))
    assert info[:7] == (2, 0, 0, 1, 1, 0, 0) and info.digest == rm.FNV0
    assert nohuman_amd.bam_scan(write(tmp_path, "header.bam", bm.bgzf(bm.forge_header()))).records == 0


def test_not_a_bam(tmp_path, corpus):
    stream, text, _, _ = corpus
    cases = {"fastq.gz": gzip.compress(text), "plain_gzip.bam": gzip.compress(stream), "bgzf_fastq.bam": bm.bgzf(text),
             "plain.bam": stream, "empty.bam": b""}
    for name, data in cases.items():
        with pytest.raises(EngineError) as ei:
            nohuman_amd.bam_scan(write(tmp_path, name, data))
        assert ei.value.code == EINVAL and "not a BAM" in ei.value.message, name
    with pytest.raises(EngineError) as ei:
        nohuman_amd.bam_scan(str(tmp_path / "missing.bam"))
    assert ei.value.code == EIO
