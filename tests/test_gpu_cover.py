"""k_cover_mark and k_cover_ivl_* on the GPU (nh_host_cover_device, nh_cover_intervals_device; nohuman_amd/csrc/nh_cover.hip) on
the toy database: the bitmap, bit for bit, against tests/intervals_model.py AND against the classifier's own per-k-mer list
(nh_classify_records_device's d_kmer_taxa on the same buffers: an entry is host when it is not 0, not ambiguous, not the mate
border); the records against the model's.  The bitmap is prefilled with a pattern: a word the pass had no bit for must keep it."""
import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import intervals_model as im
from tests import synth

pytestmark = pytest.mark.gpu
K = 35
TQ = 124  # k-mers of a tile
AMBIG, BORDER = 0xFFFFFFFF, 0xFFFFFFFE
ERR_SEQ, ERR_CAP = 1024, 2048
_LIT = {}


def lit_db(toy):
    if "toy" not in _LIT:
        _LIT["toy"] = lit.DB.from_images(toy[0], toy[1], toy[2])
    return _LIT["toy"]


def layout(seqs, gaps=None, lead=b""):
    """the sequences in a row, gaps[i] in front of sequence i -> (text, [(start, length)])"""
    t, recs = bytearray(lead), []
    for i, s in enumerate(seqs):
        t += gaps[i] if gaps is not None else b"\n"
        recs.append((len(t), len(s)))
        t += s
    return bytes(t), recs


def dev_tables(recs):
    import torch
    a = np.array(recs, dtype=np.uint64).reshape(-1, 2)
    if not len(recs):
        return torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    return (torch.from_numpy(np.ascontiguousarray(a[:, 0]).view(np.int64)).cuda(),
            torch.from_numpy(a[:, 1].astype(np.uint32).view(np.int32)).cuda())


def gpu_cover(eng, text, recs, host_of=None, prefill=None):
    """-> the bitmap's words; the text buffer ends with the dword of its last byte"""
    import torch
    n = len(text)
    d_text = torch.frombuffer(bytearray(text) + bytearray(-n % 4), dtype=torch.uint8).cuda()
    d_s, d_l = dev_tables(recs)
    nw = (n + 31) // 32
    pre = np.zeros(max(nw, 1), dtype=np.uint32) if prefill is None else prefill
    d_c = torch.from_numpy(pre.view(np.int32).copy()).cuda()
    d_h = torch.from_numpy(np.asarray(host_of, dtype=np.uint8)).cuda() if host_of is not None else None
    torch.cuda.synchronize()
    eng.host_cover_device(d_text.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), len(recs), d_c.data_ptr(),
                          d_h.data_ptr() if d_h is not None else 0, len(host_of) if host_of is not None else 0)
    torch.cuda.synchronize()
    return d_c.cpu().numpy().view(np.uint32)[:nw]


def gpu_intervals(eng, words, text_len, recs, cap):
    """-> ([(seq, start, end)] as far as the total says, the total, the error bits, the whole record buffer)"""
    import torch
    d_c = torch.from_numpy(np.concatenate((words, np.zeros(1, np.uint32))).view(np.int32).copy()).cuda()
    d_s, d_l = dev_tables(recs)
    d_r = torch.full((3 * max(cap, 1) + 3,), -1, dtype=torch.int32, device="cuda")
    d_t = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    d_e = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.cover_intervals_device(d_c.data_ptr(), text_len, d_s.data_ptr(), d_l.data_ptr(), len(recs), d_r.data_ptr(), cap, d_t.data_ptr(), d_e.data_ptr())
    torch.cuda.synchronize()
    total, raw = int(d_t.cpu()[0]), d_r.cpu().numpy().view(np.uint32)
    return [tuple(int(x) for x in raw[3 * i:3 * i + 3]) for i in range(total)], total, int(d_e.cpu()[0]), raw


def gpu_taxa(eng, text, recs):
    """the classifier's per-k-mer taxa of every sequence, each a single-end fragment of its own"""
    import torch
    d_text = torch.frombuffer(bytearray(text) + bytearray(64), dtype=torch.uint8).cuda()
    d_s, d_l = dev_tables(recs)
    nk = [max(0, n - K + 1) for _s, n in recs]
    toff = np.concatenate(([0], np.cumsum(nk))).astype(np.int64)
    d_o = torch.from_numpy(toff).cuda()
    d_t = torch.zeros(int(toff[-1]) + 1, dtype=torch.int32, device="cuda")
    d_res = torch.zeros((len(recs), 4), dtype=torch.int32, device="cuda")
    eng.classify_records_device(d_text.data_ptr(), len(text), d_s.data_ptr(), d_l.data_ptr(), len(recs), False, 0.0, d_res.data_ptr(),
                                0, 0, d_t.data_ptr(), d_o.data_ptr())
    torch.cuda.synchronize()
    t = d_t.cpu().numpy().view(np.uint32)
    return [t[toff[i]:toff[i + 1]] for i in range(len(recs))]


def check(eng, db, text, recs, host_of=None, bad=(), classifier=True, cap=None):
    """bitmap == model (== the classifier's list) and records == model; -> (the model's per-sequence covers, the records)"""
    memo = {}
    covs = [np.zeros(0, dtype=bool) if i in bad else im.covered(db, text[s:s + n], host_of, memo) for i, (s, n) in enumerate(recs)]
    good = [(s, n) if i not in bad else (0, 0) for i, (s, n) in enumerate(recs)]
    want = im.cover_words(len(text), good, covs)
    rng = np.random.default_rng(len(text))
    pre = rng.integers(0, 1 << 32, size=max(want.size, 1), dtype=np.uint32) & np.uint32(0x11111111)
    got = gpu_cover(eng, text, recs, host_of, prefill=pre.copy())
    diff = np.nonzero(got != (want | pre[:want.size]))[0]
    assert diff.size == 0, "bitmap: %d words differ, first %d: got %08x, want %08x (prefilled %08x)" % (
        diff.size, diff[0], got[diff[0]], want[diff[0]] | pre[diff[0]], pre[diff[0]])
    if classifier and not bad:
        taxa = gpu_taxa(eng, text, recs)
        for i, (s, n) in enumerate(recs):
            host = [t not in (0, AMBIG, BORDER) and (host_of is None or bool(host_of[t])) for t in taxa[i].tolist()]
            assert np.array_equal(im.cover_of(host, K, n), covs[i]), "sequence %d: the model and the classifier's list disagree" % i
    want_recs = im.records_of(good, covs)
    cap = len(want_recs) + 3 if cap is None else cap
    got_recs, total, err, _raw = gpu_intervals(eng, want, len(text), recs, cap)
    assert (total, got_recs) == (len(want_recs), want_recs)
    assert err == (ERR_SEQ if bad else 0)
    return covs, want_recs


def error_bit_is_clear(eng):
    """the sticky error word is read by the next blocking call: a clean word lets it pass"""
    eng.classify(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), np.array([0, 80], dtype=np.uint64))


def host_read(toy, rng, n, taxon=9606):
    g = toy[3][taxon]
    at = int(rng.integers(0, len(g) - n + 1))
    return g[at:at + n]


def chimera(toy, rng, a, h, b):
    return synth.random_seq(rng, a) + host_read(toy, rng, h) + synth.random_seq(rng, b)


@pytest.mark.parametrize("piece", [None, TQ, 200])
def test_lengths_alignments_and_pieces(toy, toy_engine, monkeypatch, piece):
    """34 (no k-mer), 35, 36, 158, 159, 160 (the tile border at 124 k-mers) and a read of three pieces and a bit, host and random,
    upper and lower case, every start 0 .. 3 bytes into a dword"""
    if piece:
        monkeypatch.setenv("NOHUMAN_COVER_PIECE", str(piece))
    rng = np.random.default_rng(1)
    long_n = 3 * (piece or TQ) + 50 + K - 1
    seqs, gaps = [], []
    for i, n in enumerate((34, 35, 36, 158, 159, 160, long_n) * 2):
        for kind in range(3):
            s = host_read(toy, rng, n) if kind < 2 else synth.random_seq(rng, n)
            seqs.append(s.lower() if kind == 1 and i % 2 else s)
            gaps.append(b"\n" * (1 + (len(seqs) + i) % 4))
    text, recs = layout(seqs, gaps)
    assert {s % 4 for s, _n in recs} == {0, 1, 2, 3}
    covs, want = check(toy_engine, lit_db(toy), text, recs)
    assert sum(int(c.sum()) for c in covs) > 2000 and not any(c.any() for c, (_s, n) in zip(covs, recs) if n == 34)
    error_bit_is_clear(toy_engine)


def test_random_reads_set_no_bit(toy, toy_engine):
    rng = np.random.default_rng(2)
    text, recs = layout([synth.random_seq(rng, int(n)) for n in rng.integers(0, 400, size=40)])
    covs, want = check(toy_engine, lit_db(toy), text, recs)
    assert want == [] and not any(c.any() for c in covs)


def test_chimeras_at_tile_piece_and_word_borders(toy, toy_engine, monkeypatch):
    """random | host | random: the junctions at a tile border (k-mer 124 and the base behind its last k-mer), at a piece border
    (pieces of 300 k-mers) and at a 32-bit border of the bitmap"""
    monkeypatch.setenv("NOHUMAN_COVER_PIECE", "300")
    rng = np.random.default_rng(3)
    seqs, gaps = [], []
    for a in (TQ - 1, TQ, TQ + 1, TQ + K - 1, 2 * TQ, 299, 300, 301, 300 + K - 1, 600):
        for h in (40, 150, 330):
            seqs.append(chimera(toy, rng, a, h, int(rng.integers(60, 200))))
            gaps.append(b"\n")
    for want_mod in (0, 1, 31):  # the host stretch begins / ends at a word border of the bitmap
        pos = sum(len(s) + 1 for s in seqs) + 1
        a = 100 + (want_mod - (pos + 100)) % 32
        seqs.append(chimera(toy, rng, a, 96, 120))
        gaps.append(b"\n")
        assert (pos + a) % 32 == want_mod
    text, recs = layout(seqs, gaps)
    covs, want = check(toy_engine, lit_db(toy), text, recs)
    assert len(want) >= len(seqs)


def test_ambiguous_bases_inside_a_host_stretch(toy, toy_engine):
    """under rule 1 one N stays covered (the k-mer that begins with it is looked up), two in a row leave the first uncovered: two
    intervals one base apart; other bytes that are no bases count as N"""
    db = lit_db(toy)
    rng = np.random.default_rng(4)
    h = toy[3][21][450:750]  # (inside one segment of the genome: no N of its own)
    assert h.count(b"N") == 0
    one, two, dash = h[:150] + b"N" + h[151:], h[:150] + b"NN" + h[152:], h[:100] + b"-R" + h[102:200] + b"n" * 40 + h[240:]
    text, recs = layout([h, one, two, dash, two.lower()])
    covs, want = check(toy_engine, db, text, recs)
    per_seq = lambda i: [(s, e) for q, s, e in want if q == i]
    assert per_seq(0) == [(0, 300)] and per_seq(1) == [(0, 300)]
    assert per_seq(2) == [(0, 150), (151, 300)] == per_seq(4)
    assert per_seq(3)[0] == (0, 100) and per_seq(3)[1][0] == 101


def test_back_to_back_fastq_text_and_paired_layout(toy, toy_engine):
    rng = np.random.default_rng(5)
    # no byte between two host reads: two intervals, each clipped to its sequence
    a, b, c = host_read(toy, rng, 100), host_read(toy, rng, 77), host_read(toy, rng, 35)
    text, recs = layout([a, b, c, synth.random_seq(rng, 50), a], [b"", b"", b"", b"", b""], lead=b"#")
    covs, want = check(toy_engine, lit_db(toy), text, recs)
    assert want[:3] == [(0, 0, 100), (1, 0, 77), (2, 0, 35)] and want[3] == (4, 0, 100)
    # FASTQ text whose header and quality lines are host bases themselves; mate 2's text behind all of mate 1's
    g = toy[3][9606]
    t, recs1 = bytearray(), []
    for i in range(12):
        s = host_read(toy, rng, int(rng.integers(30, 200))) if i % 2 else synth.random_seq(rng, 120)
        t += b"@" + g[i * 50:i * 50 + 60] + b"\n"
        recs1.append((len(t), len(s)))
        t += s + b"\n+\n" + g[200:200 + len(s)] + b"\n"
    t2, recs2 = layout([chimera(toy, rng, 40, 80, 30) for _ in range(12)])
    recs = []
    for x, y in zip(recs1, recs2):
        recs += [x, (len(t) + y[0], y[1])]
    assert any(recs[i + 1][0] < recs[i][0] for i in range(len(recs) - 1))
    check(toy_engine, lit_db(toy), bytes(t) + t2, recs)
    error_bit_is_clear(toy_engine)


def test_host_table(toy, toy_engine):
    """host_of marks taxon 9606 alone: the minimizers its genome shares with its ancestors (values 20 and 1) and every other taxon's
    are not host"""
    db = lit_db(toy)
    host_of = [0] * len(db.external)
    host_of[db.external.index(9606)] = 1
    rng = np.random.default_rng(6)
    seqs = [toy[3][9606], toy[3][21], chimera(toy, rng, 100, 200, 100), host_read(toy, rng, 150, 111)]
    text, recs = layout(seqs)
    covs, want = check(toy_engine, db, text, recs, host_of=host_of)
    plain = [im.covered(db, s) for s in seqs]
    assert 0 < covs[0].sum() < plain[0].sum() and not covs[1].any() and plain[1].any() and not covs[3].any()


def test_minimum_hash_value(toy):
    """a database with minimum_acceptable_hash_value set: a minimizer below it is not looked up, here as in the classifier"""
    from nohuman_amd import Engine
    ob, tb, hb, genomes, _ = synth.toy_db(min_hash=1 << 62)
    db = lit.DB.from_images(ob, tb, hb)
    full = lit_db(toy)
    rng = np.random.default_rng(7)
    seqs = [genomes[9606][:700], genomes[21][300:520], synth.random_seq(rng, 200)]
    text, recs = layout(seqs)
    with Engine.from_images(ob, tb, hb) as eng:
        covs, _w = check(eng, db, text, recs)
    assert 0 < sum(int(c.sum()) for c in covs) < sum(int(im.covered(full, s).sum()) for s in seqs)


def test_a_geometry_the_pass_does_not_support_is_refused():
    import torch
    from nohuman_amd import Engine, EngineError
    ob, tb, hb, _g, _ = synth.toy_db(k=31, l=27)
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    with Engine.from_images(ob, tb, hb) as eng:
        with pytest.raises(EngineError) as ei:
            eng.host_cover_device(d.data_ptr(), 100, d.data_ptr(), d.data_ptr(), 1, d.data_ptr())
        assert ei.value.code == -1 and "k is 31" in ei.value.message


def test_sequence_that_leaves_the_text(toy, toy_engine):
    """a forged table: one sequence runs past the text, one begins behind it; they are skipped, the bit is set, the others are right"""
    from nohuman_amd import EngineError
    rng = np.random.default_rng(8)
    seqs = [host_read(toy, rng, 150) for _ in range(10)]
    text, recs = layout(seqs)
    recs[3] = (len(text) - 100, 150)
    recs[7] = (len(text) + 5000, 40)
    recs.append((2 ** 40, 2 ** 32 - 1))
    covs, want = check(toy_engine, lit_db(toy), text, recs, bad={3, 7, 10})
    assert len(want) >= 8
    with pytest.raises(EngineError) as ei:
        error_bit_is_clear(toy_engine)
    assert ei.value.code == -4 and "host intervals" in ei.value.message
    error_bit_is_clear(toy_engine)  # read once, the word is clean again


def test_capacity_one_below_the_total(toy, toy_engine):
    rng = np.random.default_rng(9)
    text, recs = layout([chimera(toy, rng, 50, 80, 50) for _ in range(300)])  # (more than one block of sequences)
    db = lit_db(toy)
    memo = {}
    covs = [im.covered(db, text[s:s + n], None, memo) for s, n in recs]
    words = im.cover_words(len(text), recs, covs)
    want = im.records_of(recs, covs)
    assert len(want) >= 300
    got, total, err, raw = gpu_intervals(toy_engine, words, len(text), recs, len(want))
    assert (got, total, err) == (want, len(want), 0)
    got, total, err, raw = gpu_intervals(toy_engine, words, len(text), recs, len(want) - 1)
    assert (got, total, err) == ([], 0, ERR_CAP) and (raw == 0xFFFFFFFF).all()  # nothing written


def test_no_sequence_launches_nothing(toy_engine):
    words = gpu_cover(toy_engine, b"ACGT" * 20, [], prefill=np.full(3, 0x5A5A5A5A, dtype=np.uint32))
    assert (words == 0x5A5A5A5A).all()
    got, total, err, raw = gpu_intervals(toy_engine, np.full(3, 0xFFFFFFFF, dtype=np.uint32), 80, [], 4)
    assert (got, total, err) == ([], 0, 0) and (raw == 0xFFFFFFFF).all()
    error_bit_is_clear(toy_engine)
