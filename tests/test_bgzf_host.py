"""BGZF output (NH_CODEC_BGZF = 5) without a GPU: the host encoder through nh_compress_file writes exactly bgzip's container
-- checked member by member with the parser of tests/bgzf_util.py -- and the CLI refuses `--bgzf` with any output format
but gzip before it looks for a device."""
import ctypes as C
import os
import subprocess

import pytest

from nohuman_amd import _lib
from tests import bgzf_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
NH_CODEC_BGZF = 5
NAMES = ["n0", "n1", "n65279", "n65280", "n65281", "n130560", "n130561", "fastq", "random", "run"]


@pytest.fixture(scope="module")
def texts(tmp_path_factory, toy):
    return bgzf_util.corpus(tmp_path_factory.mktemp("bgzf_corpus"), toy[3])


def host_bgzf(tmp_path, data, threads):
    src, dst = tmp_path / "in.bin", tmp_path / ("out_%d.gz" % threads)
    src.write_bytes(data)
    L = _lib.lib()
    rc = L.nh_compress_file(os.fsencode(str(src)), os.fsencode(str(dst)), NH_CODEC_BGZF, threads)
    assert rc == 0, L.nh_last_error().decode()
    return dst.read_bytes()


def test_the_corpus_is_the_one_the_issue_names(texts):
    assert sorted(texts) == sorted(NAMES)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_host_encoder_writes_what_bgzip_writes(tmp_path, texts, name, threads):
    data = texts[name]
    raw = host_bgzf(tmp_path, data, threads)
    sizes = bgzf_util.check_bgzf(raw, data)
    if not data:
        assert raw == bgzf_util.EOF_MEMBER  # an empty text: the EOF member alone
    if name == "fastq":
        assert len(sizes) > 14 and len(raw) < len(data) / 2.5  # zlib level 6 on FASTQ text
    if name == "random":
        # stored blocks: zlib at level 6 closes one every 16383 literals, four a member at 5 bytes each (3 bits, padding, LEN, NLEN),
        # one more byte where the first one's padding starts; 26 bytes of framing a member, the EOF member
        assert len(raw) <= len(data) + len(sizes) * (4 * 5 + 1 + 26) + 28, len(raw) - len(data)


def test_threads_do_not_change_the_file(tmp_path, texts):
    assert host_bgzf(tmp_path, texts["fastq"], 1) == host_bgzf(tmp_path, texts["fastq"], 4)


def test_abi_enum_symbol_and_python_constant():
    import nohuman_amd
    hdr = open(os.path.join(ROOT, "include", "nohuman_engine.h")).read()
    assert "NH_CODEC_BGZF = 5" in hdr
    assert "nh_bgzf_gpu_file(" in hdr and "nh_bgzf_gpu_file" in _lib.SYMBOLS
    assert _lib.SYMBOLS["nh_bgzf_gpu_file"] == _lib.SYMBOLS["nh_gzip_gpu_file"]  # the same arguments
    assert getattr(_lib.lib(), "nh_bgzf_gpu_file") is not None
    assert nohuman_amd.CODEC_BGZF == 5 and nohuman_amd.CODEC_GZIP == 2 and nohuman_amd.engine.CODEC_BGZF == 5
    assert _lib.lib().nh_abi_version() == 5  # one enum value and one function: additive


def _cli(args):
    e = dict(os.environ)
    e.pop("NOHUMAN_DB", None)
    return subprocess.run([BIN] + args, env=e, capture_output=True, text=True)


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_help_lists_bgzf():
    r = _cli(["--help"])
    assert r.returncode == 0
    line = [ln for ln in r.stdout.splitlines() if "--bgzf" in ln]
    assert len(line) == 1 and "BGZF" in line[0], r.stdout


@pytest.mark.skipif(not os.path.exists(BIN), reason="CLI host not built")
def test_cli_bgzf_with_another_output_format_exits_2(tmp_path):
    i1 = tmp_path / "a.fq"
    i1.write_bytes(b"@r\nACGT\n+\nIIII\n")
    cases = [(["--bgzf", "-F", "z", str(i1)], "z (Zstd)"),
             (["-F", "u", "--bgzf", str(i1)], "u (uncompressed)"),
             (["--bgzf", "-o", str(tmp_path / "o.fq.zst"), str(i1)], "z (Zstd)"),
             (["--bgzf", str(i1)], "u (uncompressed)")]  # resolved from the plain input
    for args, what in cases:
        r = _cli(args)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert r.stderr.startswith("error: the argument '--bgzf' needs the output format g (Gzip), but the output format is " + what), r.stderr
        assert "For more information, try '--help'." in r.stderr
        assert "dependencies" not in r.stderr  # before the device probe
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.fq"]  # nothing was created


def test_host_reader_takes_members_of_several_blocks_closed_by_an_empty_final_one(tmp_path, texts):
    """What the GPU encoder's members look like -- coded blocks of 32 KiB, then an empty stored block with BFINAL -- built here
    with zlib (a sync flush per 32 KiB, the final empty stored block appended): the host's parallel reader, the fallback of the
    reader on the GPU, inflates such a file like any other."""
    import struct
    import zlib
    data = texts["fastq"]
    parts = []
    for i in range(0, len(data), bgzf_util.BGZF_TEXT):
        blk = data[i:i + bgzf_util.BGZF_TEXT]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(blk[:32768]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(blk[32768:]) + co.flush(zlib.Z_SYNC_FLUSH)
        assert body[-4:] == b"\x00\x00\xff\xff"   # byte-aligned behind the flush's empty stored block
        body += b"\x01\x00\x00\xff\xff"           # BFINAL 1, BTYPE 0, padding, LEN 0, NLEN 0xFFFF: what closes a region's stream
        parts.append(bgzf_util.HEADER + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(blk), len(blk)))
    raw = b"".join(parts) + bgzf_util.EOF_MEMBER
    bgzf_util.check_bgzf(raw, data)
    src, dst = tmp_path / "m.gz", tmp_path / "m.txt"
    src.write_bytes(raw)
    L = _lib.lib()
    for threads, chunk in ((1, 0), (4, 100_000)):
        rc = L.nh_gunzip_file(os.fsencode(str(src)), os.fsencode(str(dst)), threads, chunk, None)
        assert rc == 0, L.nh_last_error().decode()
        assert dst.read_bytes() == data
