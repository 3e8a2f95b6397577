"""The cut builder on the GPU (nh_host_cut_device; nohuman_amd/csrc/nh_cut.hip: the item list and the text) against
tests/hostcut_model.py on FORGED bitmaps: no database is asked, the coverage is whatever the test says.  The corpus is a text of a
few kilobytes; what it must contain is asserted on it before the GPU is used."""
import numpy as np
import pytest

from tests import builder_model as bmod
from tests import hostcut_model as hc
from tests import intervals_model as im

pytestmark = pytest.mark.gpu
CANARY = 0xEE
ERR_CUT, ERR_CAP, ERR_QLEN = 4096, 8192, 16384
START = (5, 6, 7, 8, 9, 10)  # the counters are added to: they start here
ITEM_BLOCK = 256             # items of one builder block (nh_cut.hip CB_ITEMS)
_CACHE = {}


def raw_of(h, s, q, fastq, shape="plain"):
    if not fastq:
        return b">" + h + b"\n" + s + b"\n"
    if shape == "crlf":
        return b"@" + h + b"\r\n" + s + b"\r\n+\r\n" + q + b"\r\n"
    if shape == "plusid":
        return b"@" + h + b"\n" + s + b"\n+" + h + b"\n" + q + b"\n"
    return b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n"


def forged_cover(rng, n, m):
    """covered runs of 1..60 bases and uncovered runs of m - 1, m, m + 1 or 1..120 bases in turn, starting with either"""
    cov = np.zeros(n, dtype=bool)
    p = 0 if rng.random() < 0.5 else int(rng.choice([m - 1, m, m + 1, int(rng.integers(1, 121))]))
    while p < n:
        c = int(rng.integers(1, 61))
        cov[p:p + c] = True
        p += c + int(rng.choice([m - 1, m, m + 1, int(rng.integers(1, 121)), int(rng.integers(1, 121))]))
    return cov


def corpus(m, fastq, seed=11):
    """-> dict(text, records, host, closed, bits): the records in order, which are host, the host records' closed coverage, and the
    bitmap of the text with stray bits outside the host sequences"""
    key = (m, fastq, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    items = []  # (header, length, host, coverage or None: forged, shape)
    comments = (b"", b" a comment", b"\ttab\tcomment")

    def add(name, ln, host, cov=None, shape="plain"):
        items.append((name + comments[len(items) % 3], ln, host, cov, shape))

    # 250 short records that are not host: one item each, so that the long read's pieces straddle the border of the first item block
    for i in range(250):
        add(b"n%d%s" % (i, b"x" * (i % 4)), int(rng.integers(0, 12)), False)
    add(b"long", 6000 + int(rng.integers(0, 200)), True)
    for i in range(60):
        shape = ("plain", "crlf", "plusid")[i % 3]
        add(b"h%d%s" % (i, b"y" * (i % 5)), int(rng.integers(36, 400)), True, shape=shape)
        if i % 4 == 0:
            add(b"u%d" % i, int(rng.integers(0, 90)), False, shape=shape)
    add(b"allcovered", 120, True, np.ones(120, dtype=bool))
    add(b"nothingcovered", 731, True, np.zeros(731, dtype=bool))  # (one piece of 1.5 kB: several spans under the small-span knob)
    for j, ln in enumerate((0, 1, 34, 35, 1, 1, 0, 35)):
        add(b"s%d" % j, ln, True, np.zeros(ln, dtype=bool) if j != 7 else np.ones(ln, dtype=bool))
    # exactly m - 1, m, m + 1 between covered runs, and at the two ends
    for j, ln in enumerate((m - 1, m, m + 1)):
        c = np.ones(40 + ln + 40, dtype=bool)
        c[40:40 + ln] = False
        add(b"mid%d" % j, len(c), True, c)
        c = np.ones(ln + 40, dtype=bool)
        c[:ln] = False
        add(b"start%d" % j, len(c), True, c)
        add(b"end%d" % j, len(c), True, c[::-1].copy())
    records, host, closed, raws = [], [], [], []
    for h, ln, is_host, cov, shape in items:
        s = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=ln).tobytes())
        q = bytes(rng.integers(35, 74, size=ln).astype(np.uint8).tobytes())
        raw = raw_of(h, s, q, fastq, shape)
        raws.append(raw)
        records.append(bmod.parse_record(raw, fastq))
        host.append(is_host)
        closed.append((forged_cover(rng, ln, m) if cov is None else cov) if is_host else None)
    text = b"".join(raws)
    bits = rng.random(len(text)) < 0.3  # stray bits everywhere ...
    at = 0
    for r, is_host, c in zip(records, host, closed):
        if is_host:
            bits[at + r.s:at + r.s + r.slen] = c  # ... but in the host sequences, whose bits are the coverage
        at += len(r.raw)
    _CACHE[key] = dict(text=text, records=records, host=host, closed=closed, bits=bits)
    return _CACHE[key]


def tables(records, host):
    """-> (the record table n x 4, the sequence starts, their lengths, the id lengths, the results n x 4)"""
    n = len(records)
    rec = np.zeros((n, 4), dtype=np.uint32)
    starts, lens, idl = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    res = np.zeros((n, 4), dtype=np.uint32)
    at = 0
    for i, r in enumerate(records):
        rec[i] = (at, r.hlen, at + r.q, r.qlen)
        starts[i], lens[i] = at + r.s, r.slen
        idl[i] = len(im.record_id(r.header, False))
        res[i, 0] = 7 if host[i] else 0
        at += len(r.raw)
    return rec, starts, lens, idl, res


def words_of(bits):
    pad = np.zeros((-len(bits)) % 32, dtype=bool)
    return np.packbits(np.concatenate((bits, pad)).astype(np.uint8), bitorder="little").view("<u4").copy()


def gpu_cut(eng, text, tabs, bits, fastq, m, cap, room=64):
    """-> (the out buffer: cap + room bytes, prefilled with the canary; the total; the counts the call added; the error word)"""
    import torch
    n = len(text)
    rec, starts, lens, idl, res = tabs

    def dev(a, t):
        return torch.from_numpy(np.ascontiguousarray(a).view(t).copy()).cuda()

    d_text = torch.frombuffer(bytearray(text) + bytearray(-n % 4), dtype=torch.uint8).cuda()
    d_rec, d_s, d_l, d_i, d_r = dev(rec, np.int32), dev(starts, np.int64), dev(lens, np.int32), dev(idl, np.int32), dev(res, np.int32)
    d_c = dev(np.concatenate((words_of(bits), np.zeros(1, np.uint32))), np.int32)
    d_out = torch.full((cap + room,), CANARY, dtype=torch.uint8, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_counts = torch.tensor(START, dtype=torch.int64, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.host_cut_device(d_text.data_ptr(), n, d_rec.data_ptr(), d_s.data_ptr(), d_l.data_ptr(), d_i.data_ptr(), d_r.data_ptr(), len(lens),
                        fastq, d_c.data_ptr(), m, d_out.data_ptr(), cap, d_total.data_ptr(), d_err.data_ptr(), d_counts.data_ptr())
    torch.cuda.synchronize()
    counts = tuple(int(x) - s for x, s in zip(d_counts.cpu().tolist(), START))
    return d_out.cpu().numpy().tobytes(), int(d_total.cpu()[0]), counts, int(d_err.cpu()[0])


def first_diff(a, b):
    n = min(len(a), len(b))
    return next((k for k in range(n) if a[k] != b[k]), n)


def check_corpus(c, m, want_text, cuts):
    """what the corpus promises, asserted on the model"""
    records, host, closed = c["records"], c["host"], c["closed"]
    starts, trans, combos, lens = set(), set(), set(), set()
    at = out = items = 0
    straddles = False
    for r, h, cl, ps in zip(records, host, closed, cuts):
        starts.add((at + r.s) % 4)
        if not h:
            out += r.out_len
            items += 1
        else:
            d = np.nonzero(np.diff(np.concatenate(([0], cl.astype(np.int8), [0]))))[0]
            trans |= {int(at + r.s + x) % 32 for x in d}
            straddles = straddles or (len(ps) >= 2 and items < ITEM_BLOCK < items + len(ps))
            for a, b in ps:
                head = 1 + len(im.record_id(r.header, False)) + len(b":%d-%d" % (a, b)) + (r.hlen - 1 - len(im.record_id(r.header, False))) + 1
                combos.add(((at + r.s + a) % 4, (out + head) % 4))
                assert want_text[out + head:out + head + (b - a)] == r.seq[a:b]
                out += head + (b - a) + 1 + ((3 + b - a) if r.fastq else 0)
                lens.add(b - a)
            items += len(ps)
        at += len(r.raw)
    assert out == len(want_text) and items > ITEM_BLOCK and straddles
    assert starts == set(range(4)) and trans == set(range(32)), (starts, sorted(trans))
    assert len(combos) == 16, sorted(combos)
    assert {m, m + 1} <= lens and (m - 1 not in lens or m == 1)
    runs = {b - a for cl in closed if cl is not None for a, b in im.runs(~cl)}
    assert {m, m + 1} <= runs and (m == 1 or m - 1 in runs)
    assert {r.slen for r, h in zip(records, host) if h} >= {0, 1, 34, 35}
    assert any(h and cl.all() and len(cl) for h, cl in zip(host, closed)) and any(h and len(cl) > 100 and not cl.any() for h, cl in zip(host, closed))
    long = next(i for i, r in enumerate(records) if r.header[1:5] == b"long")
    assert records[long].slen > 64 * 32 and len(im.runs(closed[long])) >= 20
    kinds = {(b" " in r.header, b"\t" in r.header) for r, h in zip(records, host) if h}
    assert kinds == {(False, False), (True, False), (False, True)}
    if records[0].fastq:
        assert any(b"\r\n" in r.raw for r, h in zip(records, host) if h) and any(b"\n+h" in r.raw for r, h in zip(records, host) if h)
    # two host sequences that share a bitmap word
    at, prev, shared = 0, None, False
    for r, h in zip(records, host):
        if h and r.slen:
            w0, w1 = (at + r.s) // 32, (at + r.s + r.slen - 1) // 32
            shared = shared or prev == w0
            prev = w1
        at += len(r.raw)
    assert shared


@pytest.mark.parametrize("span", [None, 256])
@pytest.mark.parametrize("fastq", [True, False])
@pytest.mark.parametrize("m", [1, 20, 35])
def test_against_the_model(toy_engine, monkeypatch, m, fastq, span):
    """span 256: NOHUMAN_CUT_SPAN, the bytes of an item that one wave writes -- the longest piece then takes six waves"""
    if span:
        monkeypatch.setenv("NOHUMAN_CUT_SPAN", str(span))
    c = corpus(m, fastq)
    want, six, cuts = hc.text_of(c["records"], c["host"], c["closed"], m)
    check_corpus(c, m, want, cuts)
    assert 5000 < len(c["text"]) < 64000
    assert max(b - a for ps in cuts if ps for a, b in ps) > 2 * 256  # (a piece longer than two of the small spans)
    tabs = tables(c["records"], c["host"])
    cap = len(want)  # exactly what is written
    out, total, counts, err = gpu_cut(toy_engine, c["text"], tabs, c["bits"], fastq, m, cap)
    assert err == 0 and total == len(want), (err, total, len(want))
    if out[:total] != want:
        i = first_diff(out[:total], want)
        raise AssertionError("differs from the model at byte %d: %r / %r" % (i, out[max(0, i - 60):i + 40], want[max(0, i - 60):i + 40]))
    assert out[total:] == bytes([CANARY]) * (len(out) - total)  # (bytes behind the total are untouched)
    assert counts == six, (counts, six)
    assert six[0] == six[2] + six[3] + six[4]
    # the coverage without the stray bits: the same text (a bit outside a host sequence changes nothing)
    clean = np.zeros(len(c["text"]), dtype=bool)
    at = 0
    for r, h, cl in zip(c["records"], c["host"], c["closed"]):
        if h:
            clean[at + r.s:at + r.s + r.slen] = cl
        at += len(r.raw)
    out2, total2, counts2, err2 = gpu_cut(toy_engine, c["text"], tabs, clean, fastq, m, cap + 100)
    assert (err2, total2, counts2) == (0, total, six) and out2[:total2] == want


@pytest.mark.parametrize("fastq", [True, False])
def test_a_cap_one_byte_short_writes_nothing(toy_engine, fastq):
    c = corpus(20, fastq)
    want, six, _cuts = hc.text_of(c["records"], c["host"], c["closed"], 20)
    out, total, counts, err = gpu_cut(toy_engine, c["text"], tables(c["records"], c["host"]), c["bits"], fastq, 20, len(want) - 1)
    assert err == ERR_CAP and total == 0
    assert out == bytes([CANARY]) * len(out)
    assert counts == six  # (the item list was made: the counts are the run's)


def test_a_sequence_outside_the_text_writes_nothing(toy_engine):
    c = corpus(20, True)
    n = len(c["text"])
    for victim, (start, ln) in ((260, (n - 10, 40)), (3, (n + 500, 8)), (270, (2 ** 40, 100))):
        rec, starts, lens, idl, res = tables(c["records"], c["host"])
        starts[victim], lens[victim] = start, ln
        keep = [i != victim for i in range(len(lens))]
        want, six, _ = hc.text_of([r for r, k in zip(c["records"], keep) if k], [h for h, k in zip(c["host"], keep) if k],
                                  [x for x, k in zip(c["closed"], keep) if k], 20)
        out, total, counts, err = gpu_cut(toy_engine, c["text"], (rec, starts, lens, idl, res), c["bits"], True, 20, len(want) + 50)
        assert err == ERR_CUT and total == len(want) and out[:total] == want, (victim, err, total, len(want))
        assert out[total:] == bytes([CANARY]) * (len(out) - total)
        assert counts == six


def test_fields_that_fail_their_checks_write_nothing(toy_engine):
    """a header outside the text, an id longer than its header, a quality line shorter than its host sequence: the record is not
    written, its bit is set, every other record is"""
    c = corpus(20, True)
    records, host, closed = c["records"], c["host"], c["closed"]
    first_host = next(i for i, (r, h, cl) in enumerate(zip(records, host, closed)) if h and i > 251 and hc.pieces(cl, 20))

    def without(victim):
        keep = [i != victim for i in range(len(records))]
        return hc.text_of([r for r, k in zip(records, keep) if k], [h for h, k in zip(host, keep) if k], [x for x, k in zip(closed, keep) if k], 20)[0]

    for what, bit in (("header", ERR_CUT), ("idlen", ERR_CUT), ("qlen", ERR_QLEN), ("qual", ERR_CUT)):
        rec, starts, lens, idl, res = tables(records, host)
        if what == "header":
            rec[first_host, 0] = len(c["text"]) - 3
        elif what == "idlen":
            idl[first_host] = rec[first_host, 1]  # 1 + idlen > hlen
        elif what == "qlen":
            rec[first_host, 3] -= 1
        else:
            rec[first_host, 2] = len(c["text"]) - 5
        want = without(first_host)
        out, total, _counts, err = gpu_cut(toy_engine, c["text"], (rec, starts, lens, idl, res), c["bits"], True, 20, len(want) + 50)
        assert err == bit and total == len(want) and out[:total] == want, (what, err, total, len(want))
        assert out[total:] == bytes([CANARY]) * (len(out) - total)
    # a record that is not host is written whole, as the masked run writes it, whatever its quality line's length
    victim = next(i for i, (r, h) in enumerate(zip(records, host)) if not h and r.slen > 4)
    rec, starts, lens, idl, res = tables(records, host)
    rec[victim, 3] -= 2
    out, total, _counts, err = gpu_cut(toy_engine, c["text"], (rec, starts, lens, idl, res), c["bits"], True, 20, len(c["text"]) * 2)
    want = hc.text_of(records, host, closed, 20)[0]
    assert err == 0 and total == len(want) - 2


def test_no_record_and_a_bad_min_piece(toy_engine):
    from nohuman_amd import EngineError
    c = corpus(20, True)
    out, total, counts, err = gpu_cut(toy_engine, c["text"], tuple(t[:0] for t in tables(c["records"], c["host"])), c["bits"], True, 20, 100)
    assert (total, counts, err) == (0, (0,) * 6, 0) and out == bytes([CANARY]) * len(out)
    for m in (0, 2 ** 31):
        with pytest.raises(EngineError) as ei:
            gpu_cut(toy_engine, c["text"], tables(c["records"], c["host"]), c["bits"], True, m, 100)
        assert ei.value.code == -1 and "min_piece" in ei.value.message
