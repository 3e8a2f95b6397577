"""tests/bamout_model.py, the specification of BAM output, against tests/bam_model.py on the shared corpus: header + chosen
records, lengths that add up, skipped records never present, an empty selection the header alone.  No GPU."""
import struct

import numpy as np

from tests import bam_model as bm
from tests import bamout_model as bo


def _flags(n, seed=2):
    return [bool(x) for x in np.random.default_rng(seed).integers(0, 2, n)]


def test_header_is_the_bytes_in_front_of_the_first_record():
    stream = bm.corpus_stream()
    h = bo.header_bytes(stream)
    want = bm.forge_header(b"@HD\tVN:1.6\n@SQ\tSN:chrT\tLN:5000\n@SQ\tSN:chrU\tLN:70000\n", [(b"chrT", 5000), (b"chrU", 70000)])
    assert h == want and stream.startswith(h)
    # a stream without records is its own header
    assert bo.header_bytes(want) == want and bo.select(want, [], True) == want


def test_select_against_the_record_parser():
    stream = bm.corpus_stream()
    recs = bm.records(stream)
    keep = [r for r in recs if bm.kept(r)]
    assert 0 < len(keep) < len(recs)
    flags = _flags(len(keep))
    assert any(flags) and not all(flags)
    outs = {}
    for want in (False, True):
        out = bo.select(stream, flags, want)
        head, got = bo.parse(out)
        assert head == bo.header_bytes(stream)
        chosen = [r for r, h in zip(keep, flags) if h == want]
        # every record as it lies in the input: block_size field, fixed part, name, CIGAR, bases, qualities, tags, padding
        assert got == [stream[r.offset:r.offset + 4 + r.block_size] for r in chosen]
        for raw, r in zip(got, chosen):
            assert struct.unpack_from("<i", raw)[0] == r.block_size == len(raw) - 4
        # the output parses to the same fields, in input order
        again = bm.records(out)
        assert [(r.flag, r.name, r.packed, r.l_seq, r.qual) for r in again] == [(r.flag, r.name, r.packed, r.l_seq, r.qual) for r in chosen]
        assert all(bm.kept(r) for r in again)
        outs[want] = got
    # the lengths add up: the two selections are a partition of the kept records
    kept_bytes = sum(4 + r.block_size for r in keep)
    assert sum(len(x) for x in outs[False]) + sum(len(x) for x in outs[True]) == kept_bytes
    assert len(bo.selected_bytes(stream, flags, False)) + len(bo.selected_bytes(stream, flags, True)) == kept_bytes
    assert kept_bytes < len(stream) - len(bo.header_bytes(stream))  # (the skipped records are in neither)


def test_skipped_records_are_never_present():
    stream = bm.corpus_stream()
    recs = bm.records(stream)
    skipped = [stream[r.offset:r.offset + 4 + r.block_size] for r in recs if not bm.kept(r)]
    assert len(skipped) > 10
    n = len(recs) - len(skipped)
    both = bo.selected_bytes(stream, [True] * n, True) + bo.selected_bytes(stream, [True] * n, False)
    for raw in skipped:
        assert raw not in both
    names = {r.name for r in bm.records(bo.select(stream, [True] * n, True))}
    assert names == {r.name for r in recs if bm.kept(r)} and not names & {r.name for r in recs if not bm.kept(r)}


def test_an_empty_selection_is_the_header_alone():
    stream = bm.corpus_stream()
    n = len(bo.kept_records(stream))
    assert bo.select(stream, [False] * n, True) == bo.header_bytes(stream) == bo.select(stream, [True] * n, False)
    assert bo.selected_bytes(stream, [True] * n, False) == b""
    assert bm.records(bo.select(stream, [False] * n, True)) == []


def test_tags_and_reverse_strand_records_are_untouched():
    tags = b"MMZC+m,5,12,0;\0MLB\x43\x03\0\0\0\xc8\x10\xff" + b"mvB\x63\x02\0\0\0\x05\x01"
    rec = bm.forge_record(b"read1", b"ACGTTGCA", bytes(range(8)), flag=bm.REVERSE | 0x4, tags=tags)
    sec = bm.forge_record(b"read1", b"ACGT", None, flag=bm.SECONDARY)
    stream = bm.forge_header() + sec + rec
    out = bo.select(stream, [True], True)
    assert out == bm.forge_header() + rec and out.endswith(tags)
    assert bm.records(out)[0].flag & bm.REVERSE  # (the record keeps its orientation: nothing is reverse-complemented)


def test_kernel_table_names_the_kept_records():
    stream = b"\0\0\0" + bm.corpus_stream()
    t = bo.kernel_table(stream[3:], base=-3)
    keep = bo.kept_records(stream[3:])
    assert t.shape == (len(keep), 2) and [int(x) for x in t[:, 0]] == [r.offset + 3 for r in keep]
    for off, r in zip(t[:, 0], keep):
        assert struct.unpack_from("<i", stream, int(off))[0] == r.block_size
