"""BGZF (bgzip's blocked gzip, NH_CODEC_BGZF) for the tests: a parser that walks a file member by member and checks every field
the container defines, and the corpus both encoders are driven with (tests/test_bgzf_host.py, tests/test_gpu_bgzf.py)."""
import gzip
import struct
import zlib

import numpy as np

BGZF_TEXT = 65280  # bytes of text in every data member but the last
EOF_MEMBER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HEADER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])  # ..., then BSIZE (16 bits)


def members(raw):
    """-> [(text, isize)] of every member, the EOF member included; every header and trailer field checked on the way"""
    out = []
    at = 0
    while at < len(raw):
        assert at + 28 <= len(raw), "bytes behind the last member: %d" % (len(raw) - at)
        # 1f 8b | deflate | FEXTRA only | mtime 0 | XFL 0 | OS ff | XLEN 6 | 'B' 'C' | SLEN 2
        assert raw[at:at + 16] == HEADER, (at, raw[at:at + 18].hex())
        bsize = struct.unpack_from("<H", raw, at + 16)[0]
        size = bsize + 1
        assert 28 <= size <= 65536 and at + size <= len(raw), (at, bsize)
        cdata = raw[at + 18:at + size - 8]
        crc, isize = struct.unpack_from("<II", raw, at + size - 8)
        d = zlib.decompressobj(-15)
        text = d.decompress(cdata)
        assert d.eof and d.unused_data == b"", at          # one complete deflate stream, nothing behind it: BSIZE is the member's real size - 1
        assert len(text) == isize and zlib.crc32(text) == crc, (at, len(text), isize)
        assert isize <= BGZF_TEXT
        out.append((text, isize))
        at += size
    return out


def check_bgzf(raw, want):
    """the whole file: members as bgzip cuts them, the EOF member last and nowhere else, the text equal to `want`.
    -> the ISIZE sequence of the data members"""
    ms = members(raw)
    assert raw[-28:] == EOF_MEMBER
    assert ms and ms[-1][1] == 0
    sizes = [n for _, n in ms[:-1]]
    assert all(n > 0 for n in sizes), "an empty member before the EOF member"
    assert all(n == BGZF_TEXT for n in sizes[:-1]), "a short member in mid-file: %r" % [n for n in sizes[:-1] if n != BGZF_TEXT][:4]
    assert len(sizes) == (len(want) + BGZF_TEXT - 1) // BGZF_TEXT
    assert b"".join(t for t, _ in ms) == want
    assert gzip.decompress(raw) == want
    return sizes


def fastq_corpus_text(tmp_path, genomes, n_reads=3100):
    """about 1 MB of FASTQ: reads drawn from the toy genomes, written by the fixtures' writer"""
    from tests import synth
    from tests.fastq_util import write_fastq
    rng = np.random.default_rng(17)
    reads = synth.sample_reads(rng, genomes, n_reads, len_jitter=30)
    p = tmp_path / "corpus.fq"
    write_fastq(str(p), (("r%d/1 lane:%d" % (i, i % 8), s) for i, s in enumerate(reads)))
    return p.read_bytes()


def corpus(tmp_path, genomes):
    """name -> text: the sizes around one and two members, FASTQ, bytes that do not shrink, one byte repeated"""
    rng = np.random.default_rng(4)
    fq = fastq_corpus_text(tmp_path, genomes)
    assert 900_000 < len(fq) < 1_300_000
    c = {"n%d" % n: (fq * (n // len(fq) + 1))[:n] for n in (0, 1, 65279, 65280, 65281, 130560, 130561)}
    c["fastq"] = fq
    c["random"] = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    c["run"] = b"G" * 200_000
    return c
