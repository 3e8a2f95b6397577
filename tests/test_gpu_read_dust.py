"""k_rdust on the GPU (nh_dust_reads_device, nohuman_amd/csrc/nh_dust.hip): the masked copy of a batch's sequences and the
count of masked bases against tests/dust_model.py's mask of every sequence ON ITS OWN, on texts built here.  The output buffer
is a copy of the text and the WHOLE buffer is compared: a byte touched outside a masked base fails, and so does the count.
Window 64, level 20; a tile of the kernel owns 900 positions of the virtual text (the sequences in table order, one separator
behind each), so the shapes put tile borders at many offsets inside reads, inside stretches and between reads."""
import numpy as np
import pytest

from tests import dust_model as dm

pytestmark = pytest.mark.gpu
TILE = 900  # DUST_TILE_BASES


def launch(eng, text, recs, out=None):
    """-> (the output buffer, the masked count); recs: (start, length); out: what the output holds before (default: the text)"""
    import torch
    n = len(text)
    d_text = torch.frombuffer(bytearray(text) + bytearray(8), dtype=torch.uint8).cuda()
    d_out = torch.frombuffer(bytearray(out if out is not None else text) + bytearray(8), dtype=torch.uint8).cuda()
    a = np.array(recs, dtype=np.uint64).reshape(-1, 2)
    d_s = torch.from_numpy(np.ascontiguousarray(a[:, 0]).view(np.int64)).cuda() if len(recs) else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_l = torch.from_numpy(a[:, 1].astype(np.uint32).view(np.int32)).cuda() if len(recs) else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_m = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.dust_reads_device(d_text.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), len(recs), d_out.data_ptr(), d_masked=d_m.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:n], int(d_m.cpu()[0])


def reference(text, recs, out=None, bad=()):
    want = np.frombuffer(bytes(out if out is not None else text), dtype=np.uint8).copy()
    masked = 0
    for i, (s, n) in enumerate(recs):
        if i in bad or n == 0:
            continue
        m = dm.mask_bool(bytes(text[s:s + n]))
        want[s:s + n][m] = ord("N")
        masked += int(m.sum())
    return want, masked


def error_bit_is_clear(eng):
    """the sticky error word is read by the next blocking call: a clean word lets it pass"""
    eng.classify(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), np.array([0, 80], dtype=np.uint64))


def check(eng, text, recs, out=None, bad=()):
    want, want_n = reference(text, recs, out, bad)
    got, got_n = launch(eng, text, recs, out)
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, "%d bytes differ, first at %d (got %r, want %r)" % (
        diff.size, diff[0], bytes(got[max(0, diff[0] - 8):diff[0] + 8]), bytes(want[max(0, diff[0] - 8):diff[0] + 8]))
    assert got_n == want_n
    return want_n


def lines(seqs, sep=b"\n"):
    """the sequences in a row, `sep` between them -> (text, records)"""
    t, recs = bytearray(b"#"), []
    for s in seqs:
        recs.append((len(t), len(s)))
        t += s + sep
    return bytes(t), recs


def test_short_lengths(toy_engine):
    """0, 1, 2, 3 (no triplet interval), 6 and 7 (the shortest masked homopolymer is 7), 63, 64, 65 (the window), 150, 151"""
    rng = np.random.default_rng(1)
    seqs = []
    for n in (0, 1, 2, 3, 6, 7, 63, 64, 65, 150, 151):
        seqs += [b"A" * n, dm.periodic(rng, n, 2), dm.mixed(rng, n, flank=8, longest=40), dm.iid(rng, n)]
    text, recs = lines(seqs)
    assert dm.mask(b"A" * 6) == b"A" * 6 and dm.mask(b"A" * 7) == b"N" * 7
    assert check(toy_engine, text, recs) > 0
    error_bit_is_clear(toy_engine)


def test_forty_reads_of_151_bases(toy_engine):
    """152 positions a read: the borders of the 900-position tiles fall at 7 different offsets inside reads"""
    rng = np.random.default_rng(2)
    seqs = [dm.mixed(rng, 151, flank=25, longest=70, n_share=0.01, lower_share=0.3) for _ in range(40)]
    text, recs = lines(seqs)
    assert len({(TILE * t) % 152 for t in range(1, 40 * 152 // TILE + 1)}) >= 6
    assert check(toy_engine, text, recs) > 40
    error_bit_is_clear(toy_engine)


def test_stretch_across_a_tile_border_and_a_long_read(toy_engine):
    """a 2 000-base read with an (AC)n stretch across virtual position 900 and another across 1 800; one read of 20 000 bases"""
    rng = np.random.default_rng(3)
    s = bytearray(dm.iid(rng, 2000))
    s[860:950] = b"AC" * 45
    s[1790:1815] = b"CAG" * 8 + b"C"
    long_read = dm.mixed(rng, 20_000, flank=60, longest=200, n_share=0.002, lower_share=0.2)
    text, recs = lines([bytes(s), long_read, dm.iid(rng, 150)])
    assert recs[0][0] == 1  # (the virtual text begins with this read: its base 900 is virtual position 900)
    want, _ = reference(text, recs)
    assert bytes(want[1 + 860:1 + 950]) == b"N" * 90
    assert check(toy_engine, text, recs) > 1000
    error_bit_is_clear(toy_engine)


def test_neighbours_do_not_reach_into_each_other(toy_engine):
    """a read ending in A x 6 followed by a read beginning with A x 6: each alone is clear, joined they would be masked"""
    rng = np.random.default_rng(4)
    a = dm.iid(rng, 100) + b"C" + b"A" * 6
    b = b"A" * 6 + b"G" + dm.iid(rng, 100)
    for x in (a, b):  # (the random flanks carry no stretch of their own)
        assert dm.mask(x) == x
    joined = dm.mask_bool(a + b)
    assert joined[101:113].all()
    # with a line end between them as in a file, and with nothing at all between them in the text
    for sep in (b"\n", b""):
        text, recs = lines([a, b] * 10, sep)
        assert check(toy_engine, text, recs) == 0
    # ... and at a tile border: a's last base is the last position of tile 0, the separator between the two the first of tile 1
    pad = dm.iid(rng, TILE - len(a) - 1 - 200)
    text, recs = lines([dm.iid(rng, 199), pad, a, b], b"")
    assert sum(n + 1 for _s, n in recs[:3]) == TILE + 1
    assert check(toy_engine, text, recs) == sum(dm.masked_count(text[s:s + n]) for s, n in recs)
    error_bit_is_clear(toy_engine)


def test_n_and_lowercase_inside_stretches(toy_engine):
    seqs = [b"a" * 20 + b"A" * 20, b"A" * 6 + b"N" + b"A" * 6, b"A" * 7 + b"N" + b"a" * 7, b"acACacACacACacACacAC" * 3,
            b"AC" * 10 + b"n" + b"AC" * 10, b"T" * 30 + b"R" + b"T" * 3, b"ACGT" * 2 + b"-" * 20 + b"G" * 9]
    text, recs = lines(seqs)
    want, n = reference(text, recs)
    s1 = recs[1][0]
    assert bytes(want[s1:s1 + 13]) == seqs[1] and bytes(want[recs[2][0]:recs[2][0] + 15]) == b"N" * 15  # (the N stays, and stays uncounted)
    assert n == check(toy_engine, text, recs) > 0
    error_bit_is_clear(toy_engine)


def fastq_text(rng, seqs):
    """records whose header and quality lines are themselves low-complexity bases"""
    t, recs = bytearray(), []
    for i, s in enumerate(seqs):
        t += b"@" + (b"A" * 40 if i % 2 else b"ACACACACACACACACACAC") + b"\n"
        recs.append((len(t), len(s)))
        t += s + b"\n+\n" + (b"AC" * len(s))[:len(s)] + b"\n"
    return bytes(t), recs


def test_sequences_in_place_inside_fastq_text(toy_engine):
    """header and quality lines of AAAAAAAA... and ACACAC...: the lines around a sequence are never read as bases or written"""
    rng = np.random.default_rng(6)
    seqs = [dm.mixed(rng, int(n), flank=30, longest=60) for n in rng.integers(30, 300, size=60)]
    text, recs = fastq_text(rng, seqs)
    assert check(toy_engine, text, recs) > 0
    # the output prefilled as the quality mask leaves it: nothing but the sequences, some bases N already
    pre = bytearray(b"\xEE" * len(text))
    for s, n in recs:
        pre[s:s + n] = text[s:s + n]
        pre[s + n // 2:s + n // 2 + 3] = b"NNN"[:max(0, min(3, n - n // 2))]
    check(toy_engine, text, recs, out=bytes(pre))
    error_bit_is_clear(toy_engine)


def test_paired_layout(toy_engine):
    """the table of a paired batch: mate 1, mate 2, mate 1, ... with mate 2's text behind all of mate 1's: starts not ascending"""
    rng = np.random.default_rng(7)
    t1, r1 = fastq_text(rng, [dm.mixed(rng, 151, flank=20, longest=50) for _ in range(30)])
    t2, r2 = fastq_text(rng, [dm.mixed(rng, int(n), flank=20, longest=50) for n in rng.integers(0, 200, size=30)])
    recs = []
    for a, b in zip(r1, r2):
        recs += [a, (len(t1) + b[0], b[1])]
    assert any(recs[i + 1][0] < recs[i][0] for i in range(len(recs) - 1))
    assert check(toy_engine, t1 + t2, recs) > 0
    error_bit_is_clear(toy_engine)


def test_no_sequence_launches_nothing(toy_engine):
    text = b"@r\n" + b"A" * 50 + b"\n"
    got, n = launch(toy_engine, text, [])
    assert bytes(got) == text and n == 0
    error_bit_is_clear(toy_engine)


def test_sequence_that_leaves_the_text(toy_engine):
    """a forged table: one sequence runs past the text, one begins behind it; they are skipped -- nothing of them is read or
    written --, the error value is set, every other sequence is masked"""
    from nohuman_amd import EngineError
    rng = np.random.default_rng(9)
    seqs = [dm.mixed(rng, 150, flank=20, longest=50) for _ in range(12)] + [b"A" * 120]
    text, recs = lines(seqs)
    recs[3] = (len(text) - 100, 150)
    recs[7] = (len(text) + 5000, 40)
    recs.append((2 ** 40, 2 ** 32 - 1))
    assert check(toy_engine, text, recs, bad={3, 7, 13}) >= 120
    with pytest.raises(EngineError) as ei:
        error_bit_is_clear(toy_engine)
    assert ei.value.code == -4 and "read DUST" in ei.value.message
    error_bit_is_clear(toy_engine)  # read once, the word is clean again
