"""BAM output of pairs on the GPU (nh_bam_select_pairs_device, nohuman_amd/csrc/nh_bamout.hip) against
tests/bam_pair_model.select_pairs, byte for byte: both records of a pair go out together, by the pair's call, in the order they
have in the file (mate 2 first where it is stored first), skipped records between two mates nowhere -- for pair counts 0, 1, 511,
512, 513 and 1025 around the builder's block of 1024 records, all pairs host, none and alternating, both values of `want`; the
shared corpus with its pair of a few bases beside 40 kb, in child processes with NOHUMAN_BAM_SPAN at 16 and 64 as well, so that the
long record is many spans; a forged table entry outside the BAM bytes -- its bit is set, its PAIR is absent, the others are intact --
and a buffer one byte short -- the total bit is set, nothing is written.  The output lies between two guards and is prefilled."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_pair_model as pm
from tests.test_gpu_bamout_kernel import ERR_FIELDS, ERR_OUT, FILL, GUARD, expect, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 511, 512, 513, 1025)


def launch(eng, bam, table, calls, want, out_cap):
    """table: (pairs, 2) uint64, calls: one a pair -> (the whole buffer with its guards, the total, the error bits)"""
    import torch
    raw = np.zeros((len(bam) + 3) // 4 * 4 + 8, np.uint8)
    raw[:len(bam)] = np.frombuffer(bytes(bam), np.uint8)
    d_bam = torch.from_numpy(raw).cuda()
    d_buf = torch.full((GUARD + (out_cap + 3) // 4 * 4 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 2)
    d_tab = torch.from_numpy(t.view(np.int64).copy()).cuda() if len(t) else torch.zeros(2, dtype=torch.int64, device="cuda")
    res = np.zeros((max(len(t), 1), 4), np.uint32)  # nh_result, one a pair
    res[:len(t), 0] = np.asarray(calls, np.uint32)
    res[:, 1:] = 0xA5A5A5A5
    d_res = torch.from_numpy(res.view(np.int32).copy()).cuda()
    d_tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.bam_select_pairs_device(d_bam.data_ptr(), len(bam), d_tab.data_ptr(), len(t), d_res.data_ptr(), want, d_buf.data_ptr() + GUARD, out_cap,
                                d_tot.data_ptr(), d_err.data_ptr())
    torch.cuda.synchronize()
    return d_buf.cpu().numpy(), int(d_tot.cpu()[0]), int(d_err.cpu()[0])


def check(eng, stream, calls):
    """both values of `want` on the same results, in buffers of exactly the total -> the two totals"""
    table = pm.pair_table(stream)
    assert len(table) == len(calls)
    totals = []
    for want in (0, 1):
        data = pm.selected_pair_bytes(stream, calls, want)
        assert pm.select_pairs(stream, calls, want) == pm.header_bytes(stream) + data
        got, total, err = launch(eng, stream, table, calls, want, len(data))
        same(got, expect(data, len(data)))
        assert (total, err) == (len(data), 0), (want, total, len(data), err)
        head, recs = pm.parse(pm.header_bytes(stream) + bytes(got[GUARD:GUARD + total]))
        assert head == pm.header_bytes(stream) and b"".join(recs) == data and len(recs) == 2 * sum(bool(c) == bool(want) for c in calls)
        totals.append(total)
    kept = sum(4 + r.block_size for _, _, a, b in pm.pairs(stream) for r in (a, b))
    assert sum(totals) == kept  # (a partition of the kept records; the skipped ones are nowhere)
    return totals


def selections(n):
    return {"all": np.full(n, 3), "none": np.zeros(n, int), "alternating": np.arange(n) % 2 * 7}


@pytest.fixture(scope="module")
def streams():
    return {n: pm.many_pairs(n) for n in COUNTS}


@pytest.mark.parametrize("n", COUNTS)
def test_pair_counts_around_the_block_size(toy_engine, streams, n):
    stream = streams[n]
    ps = pm.pairs(stream)
    assert len(ps) == n and (n < 3 or (any(a is m2 for _, m2, a, _ in ps) and any(a is m1 for m1, _, a, _ in ps)))
    for name, calls in selections(n).items():
        totals = check(toy_engine, stream, calls)
        if name == "all":
            assert totals[0] == 0 and (totals[1] > 0) == (n > 0)
        if name == "none":
            assert totals[1] == 0


def corpus_cases(eng):
    """the shared corpus (a few bases beside 40 kb, skipped records before, between and after mates) under every selection"""
    stream = pm.corpus_stream()
    n = len(pm.pairs(stream))
    sel = selections(n)
    sel["long pair only"] = np.array([int(m2.l_seq >= 40_000) for _, m2, _, _ in pm.pairs(stream)])
    assert sel["long pair only"].sum() == 1
    for calls in sel.values():
        check(eng, stream, calls)
    return len(sel)


def test_the_corpus_at_the_default_span(toy_engine):
    assert "NOHUMAN_BAM_SPAN" not in os.environ
    assert corpus_cases(toy_engine) == 4


def _span_child():
    from nohuman_amd import Engine
    from tests import synth
    ob, tb, hb, _, _ = synth.toy_db()
    eng = Engine.from_images(ob, tb, hb)
    n = corpus_cases(eng)
    check(eng, pm.many_pairs(513), selections(513)["alternating"])
    eng.close()
    return n


@pytest.mark.parametrize("span", [16, 64])
def test_the_long_record_as_many_spans(span):
    env = dict(os.environ, NOHUMAN_BAM_SPAN=str(span))
    src = "import sys; sys.path.insert(0, %r)\nfrom tests import test_gpu_bam_pair_kernel as t\nprint('RESULT ' + str(t._span_child()))" % ROOT
    out = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert int(out.stdout.split("RESULT ")[1]) == 4


def test_a_forged_entry_outside_the_bam_bytes_takes_its_pair_out_and_no_other(toy_engine, streams):
    stream = streams[1025]
    table = pm.pair_table(stream)
    calls = np.ones(1025, int)
    calls[::4] = 0
    for bad_pair, word, off in ((5, 0, len(stream)), (5, 1, len(stream) - 3), (512, 1, len(stream) + 12345), (511, 0, 2 ** 63), (1024, 1, 2 ** 64 - 1)):
        t = table.copy()
        t[bad_pair, word] = off  # at or beyond bam_len, or so near the end that the block_size field does not fit
        want = int(calls[bad_pair] != 0)
        data = pm.selected_pair_bytes(stream, calls, want, skip={bad_pair})  # (neither the record nor its mate)
        got, total, err = launch(toy_engine, stream, t, calls, want, len(data) + 64)
        same(got, expect(data, len(data) + 64))
        assert (total, err) == (len(data), ERR_FIELDS)
        # the other output does not hold the pair either, and is whole
        data = pm.selected_pair_bytes(stream, calls, 1 - want)
        got, total, err = launch(toy_engine, stream, t, calls, 1 - want, len(data))
        same(got, expect(data, len(data)))
        assert (total, err) == (len(data), ERR_FIELDS)


def test_a_cap_one_byte_short_sets_the_total_bit_and_writes_nothing(toy_engine, streams):
    stream = streams[513]
    table = pm.pair_table(stream)
    calls = np.arange(513) % 3
    data = pm.selected_pair_bytes(stream, calls, 1)
    got, total, err = launch(toy_engine, stream, table, calls, 1, len(data))
    same(got, expect(data, len(data)))
    assert (total, err) == (len(data), 0)
    got, total, err = launch(toy_engine, stream, table, calls, 1, len(data) - 1)
    same(got, expect(b"", len(data) - 1))  # (nothing is written, the guards are untouched)
    assert (total, err) == (0, ERR_OUT)


def test_null_and_misaligned_arguments_are_refused(toy_engine):
    import torch
    from nohuman_amd import EngineError
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = d.data_ptr()
    good = dict(d_bam=p, bam_len=64, d_table=p + 64, n_pairs=1, d_results=p + 128, want=0, d_out=p + 256, out_cap=64, d_total=p + 320, d_error_bits=p + 328)
    for bad in (dict(d_bam=p + 1), dict(d_out=p + 258), dict(d_table=p + 68), dict(d_total=p + 324), dict(want=2), dict(d_error_bits=0), dict(d_results=0)):
        with pytest.raises(EngineError) as ei:
            toy_engine.bam_select_pairs_device(**dict(good, **bad))
        assert ei.value.code == -1, (bad, ei.value.message)
