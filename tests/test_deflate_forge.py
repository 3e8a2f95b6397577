"""The forged DEFLATE streams (tests/deflate_forge.py) against zlib and against the host decoders, without a GPU.

The forge writes what zlib never writes -- repeat codes across the literal/distance boundary, 15-bit codes, a single
distance code, 258 as 284 + 31, stored blocks at every bit alignment, every member header field -- and knows each
stream's text from its own tokens.  Here: zlib agrees with that text on every valid case and refuses every invalid one (so
the corpus says what it claims), the corpus really contains every construct it is meant to (REQUIRED), it stays inside the
room the GPU decoder has, and the sequential / multi-threaded host decoder and RangeGunzip do what zlib does."""
import gzip
import zlib

import pytest

from tests import deflate_forge as forge
from tests.test_gunzip import gunzip
from tests.test_gunzip_ranges import ranges

CORPUS = forge.corpus()
VALID = [c for c in CORPUS if c.text is not None]
INVALID = [c for c in CORPUS if c.text is None]


def is_member_header(data):
    """what gzip goes on with behind a member: the magic, method 8, no reserved flag bit"""
    return len(data) >= 4 and data[:3] == b"\x1f\x8b\x08" and not data[3] & 0xE0


def zlib_members(gz):
    """zlib.decompressobj(31), chained over the members like gzip -dc: (text, members); raises zlib.error.  Bytes behind
    a member that do not begin another are ignored, a member that begins and is damaged is an error."""
    out, n, data = [], 0, gz
    while n == 0 or is_member_header(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        if not d.eof:
            raise zlib.error("the stream ends inside a member")
        n += 1
        data = d.unused_data
    return b"".join(out), n


@pytest.mark.parametrize("case", VALID, ids=lambda c: c.name)
def test_zlib_inflates_every_valid_case_to_the_replayed_text(case):
    got, n = zlib_members(case.gz)
    assert got == case.text and n == case.members
    if "reserved_flg_tail" in case.features:
        return  # (Python's gzip module does not look at the reserved flag bits: it reads the tail as a member, gzip does not)
    assert gzip.decompress(case.gz) == case.text


@pytest.mark.parametrize("case", INVALID, ids=lambda c: c.name)
def test_zlib_refuses_every_invalid_case(case):
    with pytest.raises(zlib.error):
        zlib_members(case.gz)


def test_the_corpus_contains_what_it_claims():
    have = set()
    for c in VALID:
        have |= c.features
    missing = [f for f in forge.REQUIRED if f not in have]
    assert not missing, missing
    names = {c.name for c in INVALID}
    assert not [n for n in forge.REQUIRED_INVALID if n not in names]
    assert sum(1 for c in VALID if c.name.startswith("sweep_")) >= 20


def test_the_corpus_stays_inside_the_gpu_decoders_room_and_small():
    """check_room() asserts, case by case as the corpus is built, that no aligned 1 KiB of stream holds more than 16 KiB of
    text and that the Huffman blocks of multi-stretch cases are 1 KiB at the most; here the limits themselves and the size"""
    assert forge.RATIO_TEXT == 16 * forge.RATIO_BYTES and forge.BLOCK_BYTES <= 1024
    assert sum(len(c.gz) for c in CORPUS) < 5 << 19  # a couple of megabytes
    multi = [c for c in VALID if forge.multi_stretch(c.name)]
    small = [c.name for c in multi if len(c.gz) <= 3 * 2048]
    assert len(multi) >= 30 and not small, small  # several stretches of 2 KiB each


SHAPES = [(1, 0), (4, 3000), (3, 70000)]


@pytest.mark.parametrize("threads,chunk", SHAPES)
def test_host_decoder_on_the_corpus(tmp_path, threads, chunk):
    src, dst = tmp_path / "x.gz", tmp_path / "x.out"
    bad = []
    for c in VALID:
        src.write_bytes(c.gz)
        try:
            gunzip(src, dst, threads, chunk)
            if dst.read_bytes() != c.text:
                bad.append((c.name, "wrong bytes"))
        except RuntimeError as e:
            bad.append((c.name, str(e)))
    for c in INVALID:
        src.write_bytes(c.gz)
        try:
            gunzip(src, dst, threads, chunk)
            bad.append((c.name, "accepted"))
        except RuntimeError:
            pass
    assert not bad, bad


@pytest.mark.parametrize("threads,chunk", SHAPES)
def test_range_gunzip_on_the_corpus(tmp_path, threads, chunk):
    """the same through RangeGunzip: the file as a chain of cells (every second one by the sequential decoder)"""
    src, dst = tmp_path / "x.gz", tmp_path / "x.out"
    cell = max(4 * chunk, 20_000)
    bad = []
    for c in VALID:
        src.write_bytes(c.gz)
        try:
            ranges(src, dst, threads, cell, chunk or cell, 2)
            if dst.read_bytes() != c.text:
                bad.append((c.name, "wrong bytes"))
        except RuntimeError as e:
            bad.append((c.name, str(e)))
    for c in INVALID:
        src.write_bytes(c.gz)
        try:
            ranges(src, dst, threads, cell, chunk or cell, 2)
            bad.append((c.name, "accepted"))
        except RuntimeError:
            pass
    assert not bad, bad

