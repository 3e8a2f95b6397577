"""k_bam_fastq on the GPU (nh_bam_to_fastq_device, nohuman_amd/csrc/nh_bam.hip) against tests/bam_model.py, byte for byte: the
length and name ladder of the shared corpus (record offsets and text offsets of every residue mod 4), reads of 70 000 bases at
the default span, a 300-base read at a span of 64 bytes, tables that point outside the BAM bytes or the text, and an empty
table.  The text lies between two guards of 256 bytes and is prefilled: no byte outside what the table names may change."""
import struct

import numpy as np
import pytest

from tests import bam_model as bm

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xEE, 256
ERR_FIELDS, ERR_TEXT = 1, 2


def launch(eng, bam, table, text_len, text_cap=None):
    """-> (the whole buffer: guard, text_cap bytes, guard; the error bits)"""
    import torch
    text_cap = text_len if text_cap is None else text_cap
    raw = np.zeros((len(bam) + 3) // 4 * 4 + 8, np.uint8)
    raw[:len(bam)] = np.frombuffer(bytes(bam), np.uint8)
    d_bam = torch.from_numpy(raw).cuda()
    d_buf = torch.full((GUARD + (text_cap + 3) // 4 * 4 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 2)
    d_tab = torch.from_numpy(t.view(np.int64).copy()).cuda() if len(t) else torch.zeros(2, dtype=torch.int64, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert d_bam.data_ptr() % 4 == 0 and d_buf.data_ptr() % 4 == 0 and d_tab.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    eng.bam_to_fastq_device(d_bam.data_ptr(), len(bam), d_tab.data_ptr(), len(t), d_buf.data_ptr() + GUARD, text_cap, text_len,
                            d_err.data_ptr())
    torch.cuda.synchronize()
    return d_buf.cpu().numpy(), int(d_err.cpu()[0])


def expect(text, text_cap=None, holes=()):
    """the buffer the launch must leave: the text between the guards, the ranges in `holes` as they were"""
    cap = len(text) if text_cap is None else text_cap
    want = np.full(GUARD + (cap + 3) // 4 * 4 + GUARD, FILL, np.uint8)
    want[GUARD:GUARD + len(text)] = np.frombuffer(text, np.uint8)
    for a, b in holes:
        want[GUARD + a:GUARD + b] = FILL
    return want


def same(got, want):
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, "%d bytes differ, first at text offset %d: got %r, want %r" % (
        diff.size, diff[0] - GUARD, bytes(got[diff[0]:diff[0] + 12]), bytes(want[diff[0]:diff[0] + 12]))


def check(eng, stream, **kw):
    text, _, texts, keep = bm.to_fastq(stream)
    got, err = launch(eng, stream, bm.kernel_table(keep, texts), len(text), **kw)
    same(got, expect(text, kw.get("text_cap")))
    assert err == 0
    return keep, texts


def test_the_ladder_at_every_residue(toy_engine):
    keep, texts = check(toy_engine, bm.corpus_stream())
    starts = np.cumsum([0] + [len(x) for x in texts[:-1]])
    for L in (4, 5, 9, 65, 257):  # (tests/test_bam_model.py asserts the residues of the corpus as a whole)
        assert any(r.l_seq == L for r in keep)
    assert {r.offset % 4 for r in keep} == {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    # the same records in a buffer with room behind the text: nothing behind text_len is written
    check(toy_engine, bm.corpus_stream(seed=6), text_cap=len(b"".join(texts)) + 4096)


def _long_stream(rng, L, with_short=True):
    iupac = np.frombuffer(bm.ALPHABET, np.uint8)
    recs = []
    for k, flag in enumerate((0, bm.REVERSE, 0, bm.REVERSE)):
        seq = iupac[rng.integers(0, 16, L + k)].tobytes()
        qual = None if k == 2 else rng.integers(0, 94, L + k, dtype=np.uint8).tobytes()
        recs.append(bm.forge_record(b"long%d/%s" % (k, b"x" * k), seq, qual, flag=flag, tags=b"NMC\x01" * k))
        if with_short:
            recs.append(bm.forge_record(b"s%d" % k, b"ACGTN"[:1 + k], bytes(1 + k), flag=flag))
    return bm.forge_header() + b"".join(recs)


def test_reads_of_70000_bases_at_the_default_span(toy_engine):
    check(toy_engine, _long_stream(np.random.default_rng(70), 70_000))


@pytest.mark.parametrize("span", [16, 64, 100])
def test_a_300_base_read_over_several_spans(toy_engine, monkeypatch, span):
    monkeypatch.setenv("NOHUMAN_BAM_SPAN", str(span))
    check(toy_engine, _long_stream(np.random.default_rng(span), 300))
    check(toy_engine, bm.corpus_stream())


def test_bad_table_entries_set_their_bit_and_write_nothing(toy_engine):
    stream = bytearray(bm.corpus_stream())
    text, _, texts, keep = bm.to_fastq(bytes(stream))
    table = bm.kernel_table(keep, texts)
    ends = np.cumsum([len(x) for x in texts])
    # (a) an entry that points 10 bytes before the end of the BAM bytes
    t = table.copy()
    t[7, 0] = len(stream) - 10
    got, err = launch(toy_engine, stream, t, len(text))
    same(got, expect(text, holes=[(int(ends[7]) - len(texts[7]), int(ends[7]))]))
    assert err == ERR_FIELDS
    # (b) a record whose l_seq overruns the buffer: the long read 255 of the ladder claims to be longer than the BAM bytes
    k = next(i for i, r in enumerate(keep) if r.l_seq == 255)
    bad = bytearray(stream)
    struct.pack_into("<I", bad, keep[k].offset + 20, len(stream))
    got, err = launch(toy_engine, bad, table, len(text))
    same(got, expect(text, holes=[(int(ends[k]) - len(texts[k]), int(ends[k]))]))
    assert err == ERR_FIELDS
    # (c) a record without bases or without a name in the table (the host never lists one)
    bad = bytearray(stream)
    bad[keep[3].offset + 12] = 0
    got, err = launch(toy_engine, bad, table, len(text))
    same(got, expect(text, holes=[(int(ends[3]) - len(texts[3]), int(ends[3]))]))
    assert err == ERR_FIELDS
    # (d) a text shorter than the last record needs: that record stays out
    short = len(text) - 3
    got, err = launch(toy_engine, stream, table, short, text_cap=len(text))
    same(got, expect(text, holes=[(int(ends[-1]) - len(texts[-1]), len(text))]))
    assert err == ERR_TEXT
    # (e) an entry whose text offset lies behind the text
    t = table.copy()
    t[-1, 1] = len(text) + 1000
    got, err = launch(toy_engine, stream, t, len(text))
    same(got, expect(text, holes=[(int(ends[-1]) - len(texts[-1]), len(text))]))
    assert err == ERR_TEXT


def test_no_records(toy_engine):
    got, err = launch(toy_engine, bm.corpus_stream(), np.zeros((0, 2), np.uint64), 0, text_cap=64)
    same(got, expect(b"", text_cap=64))
    assert err == 0
