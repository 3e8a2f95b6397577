"""k_host_filter on the GPU (nh_host_filter_device; nohuman_amd/csrc/nh_host.hip) alone, on forged nh_result arrays over a forged
table of 5000 nodes: the output is the input with call = 0 where the table says the call is not host, words 1-3 of every record
untouched; the counters grow by the host and the spared fragments.  The sizes are the smallest at which the kernel can go wrong:
nothing, one record, a wave less one / exactly / plus one, four waves less one / exactly / plus one, a workgroup (1024 threads)
less one / exactly / plus one, many workgroups with a partial last wave; in place and out of place, with and without counters, two
launches on one pair of counters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NH_EDEVICE = -4
NODES = 5000
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 100003]


@pytest.fixture(scope="module")
def eng(toy):
    from nohuman_amd import Engine
    e = Engine.from_images(toy[0], toy[1], toy[2])
    yield e
    e.close()


@pytest.fixture(scope="module")
def forged():
    """the table (about a third of the nodes host, node 0 never) and the largest array of results: calls over all nodes, a third of
    them 0, words 1-3 random"""
    rng = np.random.default_rng(128)
    table = (rng.random(NODES) < 0.35).astype(np.uint8)
    table[0] = 0
    res = rng.integers(0, 2 ** 32, size=(max(SIZES), 4), dtype=np.uint64).astype(np.uint32)
    calls = rng.integers(1, NODES, size=max(SIZES)).astype(np.uint32)
    calls[rng.random(max(SIZES)) < 0.33] = 0
    calls[:8] = [NODES - 1, 0, 1, NODES - 1, 1, 0, 2, 3]  # (the table's ends, in the first wave)
    res[:, 0] = calls
    return table, res


def model(res, table):
    """(the filtered records, host fragments, spared fragments)"""
    call = res[:, 0]
    host = table[call] != 0
    out = res.copy()
    out[~host, 0] = 0
    return out, int(host.sum()), int(((call != 0) & ~host).sum())


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(4, dtype=torch.int32, device="cuda")
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.uint8 if a.dtype == np.uint8 else np.int64)).cuda()


def launch(eng, res, table, in_place, d_counts=None, n_nodes=None):
    """one launch -> the output records (n, 4) uint32"""
    import torch
    n = len(res)
    d_in = dev(res.reshape(-1))
    d_out = d_in if in_place else torch.full((max(4 * n, 4) + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_t = dev(table)
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    eng.host_filter_device(d_in.data_ptr(), d_out.data_ptr(), n, d_t.data_ptr(), len(table) if n_nodes is None else n_nodes,
                           d_counts.data_ptr() if d_counts is not None else 0)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    if not in_place:
        assert (got[4 * n:] == 0x5A5A5A5A).all()  # nothing behind the last record is written
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32)[:4 * n], res.reshape(-1))  # the input is only read
    return got[:4 * n].reshape(n, 4)


def error_bit_is_clear(eng):
    """the sticky error word is read by the next blocking call: a clean word lets it pass"""
    eng.classify(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), np.array([0, 80], dtype=np.uint64))


@pytest.mark.parametrize("n", SIZES)
def test_sizes_in_place_and_out_of_place_with_and_without_counters(eng, forged, n):
    import torch
    table, res = forged
    res = res[:n]
    want, host, spared = model(res, table)
    assert n < 1000 or (host > n // 10 and spared > n // 10 and host + spared < n)
    for in_place in (False, True):
        got = launch(eng, res, table, in_place)  # no counters
        assert np.array_equal(got, want), (n, in_place, np.argwhere(got != want)[:8])
        d_c = torch.tensor([1000, 7], dtype=torch.int64, device="cuda")
        got = launch(eng, res, table, in_place, d_c)
        assert np.array_equal(got, want), (n, in_place)
        assert np.array_equal(got[:, 1:], res[:, 1:])  # words 1-3 of every record as they were
        assert d_c.cpu().tolist() == [1000 + host, 7 + spared], (n, in_place)
    error_bit_is_clear(eng)


def test_two_launches_accumulate(eng, forged):
    import torch
    table, res = forged
    d_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    a, b = res[:1025], res[1025:1025 + 257]
    launch(eng, a, table, False, d_c)
    launch(eng, b, table, True, d_c)
    _, ha, sa = model(a, table)
    _, hb, sb = model(b, table)
    assert d_c.cpu().tolist() == [ha + hb, sa + sb] and hb and sb
    error_bit_is_clear(eng)


@pytest.mark.parametrize("fill", [1, 0])
def test_a_table_of_all_host_and_of_all_zero(eng, forged, fill):
    import torch
    _, res = forged
    res = res[:1025]
    table = np.full(NODES, fill, dtype=np.uint8)
    table[0] = 0
    classified = int((res[:, 0] != 0).sum())
    d_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = launch(eng, res, table, False, d_c)
    if fill:
        assert np.array_equal(got, res)  # every classified fragment is host: the copy is the input
        assert d_c.cpu().tolist() == [classified, 0]
    else:
        assert (got[:, 0] == 0).all() and np.array_equal(got[:, 1:], res[:, 1:])
        assert d_c.cpu().tolist() == [0, classified]
    assert 0 < classified < 1025
    error_bit_is_clear(eng)


def test_a_call_outside_the_table_is_never_an_index(eng, forged):
    """three calls at n_nodes, n_nodes + 1 and 0xFFFFFFFF among 300 records: they come out as 0 and are counted nowhere, their
    neighbours are right, the engine's next blocking call fails with NH_EDEVICE and the message of the new error bit -- once"""
    import torch
    from nohuman_amd import EngineError
    table, res = forged
    res = res[:300].copy()
    res[10, 0], res[64, 0], res[299, 0] = NODES, NODES + 1, 0xFFFFFFFF
    inside = np.ones(300, dtype=bool)
    inside[[10, 64, 299]] = False
    want, host, spared = model(res[inside], table)
    for in_place in (False, True):
        d_c = torch.zeros(2, dtype=torch.int64, device="cuda")
        got = launch(eng, res, table, in_place, d_c)
        assert np.array_equal(got[inside], want)
        assert (got[~inside, 0] == 0).all() and np.array_equal(got[:, 1:], res[:, 1:])
        assert d_c.cpu().tolist() == [host, spared]
        with pytest.raises(EngineError) as ei:
            error_bit_is_clear(eng)
        assert ei.value.code == NH_EDEVICE and "host filter" in ei.value.message and "outside the taxonomy" in ei.value.message
        error_bit_is_clear(eng)  # cleared with the call that reported it: the engine is usable
    # a table said to be shorter than it is: the calls at and above n_nodes are the ones refused
    got = launch(eng, res[inside][:64], table, False, n_nodes=NODES - 1)
    sub = res[inside][:64].copy()
    assert (sub[:, 0] == NODES - 1).sum() >= 2
    sub[sub[:, 0] == NODES - 1, 0] = 0
    assert np.array_equal(got, model(sub, table)[0])
    with pytest.raises(EngineError):
        error_bit_is_clear(eng)
    error_bit_is_clear(eng)


def test_refusals(eng):
    import torch
    from nohuman_amd import EngineError
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    for args in ((0, d.data_ptr(), 4, d.data_ptr(), 4), (d.data_ptr(), 0, 4, d.data_ptr(), 4), (d.data_ptr(), d.data_ptr(), 4, 0, 4),
                 (d.data_ptr() + 4, d.data_ptr(), 4, d.data_ptr(), 4), (d.data_ptr(), d.data_ptr() + 8, 4, d.data_ptr(), 4)):
        with pytest.raises(EngineError) as ei:
            eng.host_filter_device(*args)
        assert ei.value.code == -1
    eng.host_filter_device(d.data_ptr(), d.data_ptr(), 0, d.data_ptr(), 0)  # n == 0: nothing is launched
    torch.cuda.synchronize()
    error_bit_is_clear(eng)
