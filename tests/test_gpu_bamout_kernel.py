"""BAM output's kernels on the GPU (nh_bam_select_device, nohuman_amd/csrc/nh_bamout.hip) against tests/bamout_model.py, byte for
byte: record lengths of every residue mod 4 from the 36-byte minimum past one wave round, source offsets of every residue, record
counts around the builder's block size, every kind of selection, both values of `want` on the same results, skipped records
between the table's entries, a buffer of exactly the total and of one byte less, table entries outside the BAM bytes -- and, in a
child process with NOHUMAN_BAM_SPAN=64, records of 1-3 kB that are many spans each; at the default span one record of 40 kB.
The output lies between two guards of 64 bytes and is prefilled: no byte outside what the selection names may change."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_model as bm
from tests import bamout_model as bo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, GUARD = 0xEE, 64
ERR_FIELDS, ERR_OUT = 1, 4
BLOCK = 256 * 4  # records of one block of the builder: OB_THREADS x BO_PER_THREAD (nh_bamout.hip)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def launch(eng, bam, table, calls, want, out_cap):
    """bam: the bytes at d_bam (the table's offsets point into them) -> (the whole buffer: guard, out_cap bytes rounded up to a
    dword, guard; the total; the error bits)"""
    import torch
    raw = np.zeros((len(bam) + 3) // 4 * 4 + 8, np.uint8)
    raw[:len(bam)] = np.frombuffer(bytes(bam), np.uint8)
    d_bam = torch.from_numpy(raw).cuda()
    d_buf = torch.full((GUARD + (out_cap + 3) // 4 * 4 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 2)
    d_tab = torch.from_numpy(t.view(np.int64).copy()).cuda() if len(t) else torch.zeros(2, dtype=torch.int64, device="cuda")
    res = np.zeros((max(len(t), 1), 4), np.uint32)  # nh_result: call, total_kmers, clade_hits, hit_groups
    res[:len(t), 0] = np.asarray(calls, np.uint32)
    res[:, 1:] = 0xA5A5A5A5
    d_res = torch.from_numpy(res.view(np.int32).copy()).cuda()
    d_tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert d_bam.data_ptr() % 4 == 0 and d_buf.data_ptr() % 4 == 0 and d_tab.data_ptr() % 8 == 0 and d_tot.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    eng.bam_select_device(d_bam.data_ptr(), len(bam), d_tab.data_ptr(), len(t), d_res.data_ptr(), want, d_buf.data_ptr() + GUARD, out_cap,
                          d_tot.data_ptr(), d_err.data_ptr())
    torch.cuda.synchronize()
    return d_buf.cpu().numpy(), int(d_tot.cpu()[0]), int(d_err.cpu()[0])


def expect(data, out_cap):
    want = np.full(GUARD + (out_cap + 3) // 4 * 4 + GUARD, FILL, np.uint8)
    want[GUARD:GUARD + len(data)] = np.frombuffer(data, np.uint8)
    return want


def same(got, want):
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, "%d bytes differ, first at output offset %d: got %r, want %r" % (
        diff.size, diff[0] - GUARD, bytes(got[diff[0]:diff[0] + 12]), bytes(want[diff[0]:diff[0] + 12]))


def chosen(bam, table, calls, want, skip=()):
    """the model on a table: the bytes of the listed records whose call != 0 is `want`, in table order"""
    out = []
    for i, ((off, _), c) in enumerate(zip(table, calls)):
        if (c != 0) == bool(want) and i not in skip:
            off = int(off)
            out.append(bytes(bam[off:off + 4 + struct.unpack_from("<i", bam, off)[0]]))
    return b"".join(out)


def check(eng, bam, table, calls, extra=0):
    """both values of `want` on the same results, in buffers of exactly the total (+ extra) -> the two totals"""
    totals = []
    for want in (0, 1):
        data = chosen(bam, table, calls, want)
        got, total, err = launch(eng, bam, table, calls, want, len(data) + extra)
        same(got, expect(data, len(data) + extra))
        assert (total, err) == (len(data), 0), (want, total, len(data), err)
        totals.append(total)
    # the two outputs are a partition of the listed records
    assert sum(totals) == sum(4 + struct.unpack_from("<i", bam, int(off))[0] for off, _ in table)
    return totals


def selections(n, rng):
    """name -> calls (0: not host, else an internal taxon id) for n records"""
    s = {"all": np.full(n, 3), "none": np.zeros(n, int), "alternating": np.arange(n) % 2 * 7, "runs": (np.arange(n) // 5 % 2) * 2,
         "random": rng.integers(0, 3, n)}
    if n:
        first, last = np.zeros(n, int), np.zeros(n, int)
        first[0], last[-1] = 9, 1
        s["first only"], s["last only"] = first, last
    return s


def ladder(rng, prefix):
    """(the bytes at d_bam, the table of the listed records): records of every length mod 4 from the 36-byte minimum past one wave
    round (256 bytes), names of every length mod 4, pad 0..3, tags, with secondary / empty records between the listed ones; the
    stream starts `prefix` bytes into the buffer, so the source offsets take every residue as well"""
    recs, listed = [], []
    # the minimum: block_size 32, the fixed part and nothing else -- 36 bytes (no reader lists such a record; the kernels copy it)
    recs.append(struct.pack("<i", 32) + bm.forge_record(b"", b"", b"")[4:36])
    listed.append(True)
    for k in range(48):
        L = (1, 2, 3, 5, 8, 30, 61, 100, 140, 141, 142, 143, 144, 145, 146, 147, 150, 300, 511, 700)[k % 20]
        seq = _ACGT[rng.integers(0, 4, L)].tobytes()
        name = b"n" * (k % 9)
        tags = (b"", b"NMC\x03", b"RGZgroup1\0MMZC+m,1;\0", b"MLBC\x05\0\0\0\x01\x02\x03\x04\x05")[k % 4]
        recs.append(bm.forge_record(name, seq, None if k % 5 == 0 else bytes(L), flag=bm.REVERSE if k % 3 == 0 else 0, tags=tags, pad=k % 4))
        listed.append(True)
        if k % 4 == 1:
            recs.append(bm.forge_record(b"sec%d" % k, b"ACGTAC", None, flag=bm.SECONDARY, pad=k % 3))
            listed.append(False)
        if k % 7 == 2:
            recs.append(bm.forge_record(b"empty%d" % k, b"", b"", pad=1))
            listed.append(False)
    head = bm.forge_header()
    table, at = [], prefix + len(head)
    for r, l in zip(recs, listed):
        if l:
            table.append((at, 2 ** 64 - 1))
        at += len(r)
    return b"\x5a" * prefix + head + b"".join(recs), np.array(table, np.uint64)


def test_the_ladder_at_every_residue_and_every_selection(toy_engine):
    rng = np.random.default_rng(11)
    lengths, src, dst = set(), set(), set()
    for prefix in range(4):
        bam, table = ladder(rng, prefix)
        sizes = [4 + struct.unpack_from("<i", bam, int(off))[0] for off, _ in table]
        lengths |= {s % 4 for s in sizes}
        src |= {int(off) % 4 for off, _ in table}
        assert min(sizes) == 36 and max(sizes) > 1000 and any(256 < s < 300 for s in sizes)
        for name, calls in selections(len(table), rng).items():
            if prefix and name in ("all", "none"):
                continue
            check(toy_engine, bam, table, calls)
            dst |= {int(x) % 4 for x in np.cumsum([s for s, c in zip(sizes, calls) if c == 0])}
    assert lengths == src == dst == {0, 1, 2, 3}


def test_against_the_model_on_the_shared_corpus(toy_engine):
    """the reader's own table of the corpus' kept records (skipped records between its entries): bamout_model.selected_bytes"""
    stream = bm.corpus_stream()
    table = bo.kernel_table(stream)
    n = len(table)
    assert n == len(bo.kept_records(stream)) < len(bm.records(stream))
    flags = np.random.default_rng(4).integers(0, 2, n)
    for want in (0, 1):
        data = bo.selected_bytes(stream, flags, want)
        assert data == chosen(stream, table, flags, want)
        got, total, err = launch(toy_engine, stream, table, flags * 5, want, len(data) + 100)  # (room behind the total: untouched)
        same(got, expect(data, len(data) + 100))
        assert (total, err) == (len(data), 0)
        head, recs = bo.parse(bo.header_bytes(stream) + bytes(got[GUARD:GUARD + total]))
        assert head == bo.header_bytes(stream) and b"".join(recs) == data


@pytest.fixture(scope="module")
def many():
    """2 * BLOCK + 1 short records, a secondary record after every 50th: the bytes, the table of the others"""
    rng = np.random.default_rng(23)
    recs, table, at = [], [], 0
    head = bm.forge_header()
    at = len(head)
    for i in range(2 * BLOCK + 1):
        L = 1 + i % 13
        r = bm.forge_record(b"r%d" % i, _ACGT[rng.integers(0, 4, L)].tobytes(), bytes([i % 40]) * L, tags=b"NMC\x01" if i % 3 == 0 else b"", pad=i % 4)
        table.append((at, at))
        recs.append(r)
        at += len(r)
        if i % 50 == 49:
            recs.append(bm.forge_record(b"s%d" % i, b"ACGT", None, flag=bm.SUPPLEMENTARY))
            at += len(recs[-1])
    return head + b"".join(recs), np.array(table, np.uint64)


@pytest.mark.parametrize("n", [0, 1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1])
def test_record_counts_around_the_block_size(toy_engine, many, n):
    bam, table = many
    rng = np.random.default_rng(n)
    sel = selections(n, rng)
    for name in ("random", "alternating", "all") + (("first only", "last only") if n else ()):
        totals = check(toy_engine, bam, table[:n], sel[name])
        if name == "all":
            assert totals[0] == 0 and (totals[1] > 0) == (n > 0)


def test_out_cap_exactly_the_total_and_one_byte_less(toy_engine, many):
    bam, table = many
    n = BLOCK + 7
    calls = np.arange(n) % 3
    data = chosen(bam, table[:n], calls, 1)
    got, total, err = launch(toy_engine, bam, table[:n], calls, 1, len(data))
    same(got, expect(data, len(data)))
    assert (total, err) == (len(data), 0)
    got, total, err = launch(toy_engine, bam, table[:n], calls, 1, len(data) - 1)
    same(got, expect(b"", len(data) - 1))  # (nothing is written, the guards are untouched)
    assert (total, err) == (0, ERR_OUT)
    got, total, err = launch(toy_engine, bam, table[:n], calls, 1, 0)
    same(got, expect(b"", 0))
    assert (total, err) == (0, ERR_OUT)


def test_bad_table_entries_set_the_fields_bit_and_write_nothing_of_the_record(toy_engine, many):
    bam, table = many
    n = BLOCK + 50
    calls = np.ones(n, int)
    calls[::4] = 0
    for bad_at, off in ((5, len(bam)), (BLOCK + 3, len(bam) - 3), (17, len(bam) + 12345), (BLOCK - 1, 2 ** 63)):
        t = table[:n].copy()
        t[bad_at, 0] = off  # at or beyond bam_len, or so near the end that the block_size field does not fit
        want = int(calls[bad_at] != 0)
        data = chosen(bam, t, calls, want, skip={bad_at})
        got, total, err = launch(toy_engine, bam, t, calls, want, len(data) + 64)
        same(got, expect(data, len(data) + 64))
        assert (total, err) == (len(data), ERR_FIELDS)
    # a block_size that reaches past bam_len: the record's own field, read on the device
    k = 33
    for bs in (len(bam), 0x7FFFFFFF, 0xFFFFFFFF, len(bam) - int(table[k, 0]) - 3):
        bad = bytearray(bam)
        struct.pack_into("<I", bad, int(table[k, 0]), bs)
        want = int(calls[k] != 0)
        data = chosen(bam, table[:n], calls, want, skip={k})
        got, total, err = launch(toy_engine, bytes(bad), table[:n], calls, want, len(data) + 64)
        same(got, expect(data, len(data) + 64))
        assert (total, err) == (len(data), ERR_FIELDS)
    # the last record of the BAM bytes ends exactly at bam_len: inside
    last = len(table) - 1
    assert int(table[last, 0]) + 4 + struct.unpack_from("<i", bam, int(table[last, 0]))[0] == len(bam)
    check(toy_engine, bam, table[last - 3:], [1, 0, 1, 1])


def long_records(rng, sizes):
    """records of about `sizes` bytes each -- a Z tag and a B array that fill them -- with short ones between"""
    recs, table = [], []
    head = bm.forge_header()
    at = len(head)
    for k, size in enumerate(sizes):
        L = 40 + k
        body = rng.integers(33, 127, max(size - 200, 8), dtype=np.uint8).tobytes()
        half = len(body) // 2
        tags = b"MMZ" + body[:half] + b"\0" + b"MLBC" + struct.pack("<I", len(body) - half) + body[half:]
        for r in (bm.forge_record(b"long%d" % k, _ACGT[rng.integers(0, 4, L)].tobytes(), bytes(L), flag=bm.REVERSE if k % 2 else 0, tags=tags, pad=k % 4),
                  bm.forge_record(b"s%d" % k, b"ACGTN"[:1 + k % 5], bytes(1 + k % 5), pad=(k + 1) % 4)):
            table.append((at, 0))
            recs.append(r)
            at += len(r)
    return head + b"".join(recs), np.array(table, np.uint64)


def test_a_record_of_40_kb_at_the_default_span(toy_engine):
    rng = np.random.default_rng(40)
    assert "NOHUMAN_BAM_SPAN" not in os.environ
    bam, table = long_records(rng, [40_001, 3000, 16_384 + 36, 16_383])
    for calls in ([1, 1, 0, 0, 1, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1, 0], [0, 1, 1, 1, 0, 1, 0, 0]):
        check(toy_engine, bam, table, calls)


def span_cases():
    """what the child process runs under NOHUMAN_BAM_SPAN=64: records of 1-3 kB, every one many spans, and the many short ones"""
    from nohuman_amd import Engine
    from tests import synth
    ob, tb, hb, _, _ = synth.toy_db()
    eng = Engine.from_images(ob, tb, hb)
    rng = np.random.default_rng(64)
    n = 0
    for prefix in range(4):
        bam, table = long_records(rng, [1000 + 257 * k + prefix for k in range(8)])
        bam, table = b"\0" * prefix + bam, table + np.array([prefix, 0], np.uint64)
        for name, calls in selections(len(table), rng).items():
            check(eng, bam, table, calls)
            n += 1
    bam, table = ladder(rng, 1)
    for name, calls in selections(len(table), rng).items():
        check(eng, bam, table, calls)
        n += 1
    eng.close()
    return n


def test_records_of_many_spans_at_a_span_of_64_bytes():
    env = dict(os.environ, NOHUMAN_BAM_SPAN="64")
    src = "import sys; sys.path.insert(0, %r)\nfrom tests import test_gpu_bamout_kernel as t\nprint('RESULT ' + str(t.span_cases()))" % ROOT
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert int(out.stdout.split("RESULT ")[1]) == 4 * 7 + 7


def test_null_and_misaligned_arguments_are_refused(toy_engine):
    import torch
    from nohuman_amd import EngineError
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = d.data_ptr()
    good = dict(d_bam=p, bam_len=64, d_table=p + 64, n_records=1, d_results=p + 128, want=0, d_out=p + 256, out_cap=64, d_total=p + 320, d_error_bits=p + 328)
    for bad in (dict(d_bam=p + 1), dict(d_out=p + 258), dict(d_table=p + 68), dict(d_total=p + 324), dict(want=2), dict(d_error_bits=0), dict(d_results=0)):
        with pytest.raises(EngineError) as ei:
            toy_engine.bam_select_device(**dict(good, **bad))
        assert ei.value.code == -1, (bad, ei.value.message)
