"""k_qmask on the GPU (nh_quality_mask_device, nohuman_amd/csrc/nh_qmask.hip): the masked copy of a batch's sequences and
the count of masked bases against numpy, on texts built here -- every pair of residues mod 4 of the bases and the qualities,
lengths around the kernel's chunk (16 bytes), team (512 bytes) and workgroup steps (4096 bytes), sequences one byte apart,
records without qualities, and quality lines that are not as long as their sequence.  The output is prefilled with 0xEE:
no byte outside the sequence ranges may change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FILL = 0xEE
NONE = 2 ** 64 - 1


class Text:
    """a batch text under construction: records of (sequence start, length, quality start)"""

    def __init__(self, rng):
        self.rng, self.t, self.recs = rng, bytearray(), []

    def pad_to(self, residue):
        """filler (no line ends: they must not look like a quality line's end) up to an offset of the residue mod 4"""
        while len(self.t) % 4 != residue:
            self.t += b"#"

    def put(self, data, residue=None):
        if residue is not None:
            self.pad_to(residue)
        at = len(self.t)
        self.t += data
        return at

    def bases(self, n):
        return bytes(self.rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=n).tobytes())

    def quals(self, n, lo=33, hi=126):
        return bytes(self.rng.integers(lo, hi + 1, size=n).astype(np.uint8).tobytes())

    def fastq(self, n, rs=None, rq=None, lo=33, hi=126):
        """a four-line record with n bases, the sequence at residue rs and the qualities at residue rq"""
        self.put(b"@r%d" % len(self.recs))
        if rs is not None:
            self.pad_to((rs - 1) % 4)
        self.t += b"\n"
        s = self.put(self.bases(n))
        self.t += b"\n+"
        if rq is not None:
            self.pad_to((rq - 1) % 4)
        self.t += b"\n"
        q = self.put(self.quals(n, lo, hi))
        self.t += b"\n"
        self.recs.append((s, n, q))

    def fasta(self, n, rs=None):
        self.put(b">r%d" % len(self.recs))
        if rs is not None:
            self.pad_to((rs - 1) % 4)
        self.t += b"\n"
        s = self.put(self.bases(n))
        self.t += b"\n"
        self.recs.append((s, n, NONE))


def reference(text, recs, q, bad=()):
    """numpy: the output buffer and the masked count; the records in `bad` are not written"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    out = np.full(len(t) + 8, FILL, dtype=np.uint8)
    masked = 0
    for i, (s, n, qs) in enumerate(recs):
        if i in bad or n == 0:
            continue
        b = t[s:s + n].copy()
        if qs != NONE:
            low = t[qs:qs + n].astype(np.int64) - 33 < q
            b[low] = ord("N")
            masked += int(low.sum())
        out[s:s + n] = b
    return out, masked


def launch(eng, text, recs, q):
    import torch
    n = len(text)
    t = torch.zeros(n + 8, dtype=torch.uint8)
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    d_text = t.cuda()
    d_out = torch.full((n + 8,), FILL, dtype=torch.uint8, device="cuda")
    a = np.array(recs, dtype=np.uint64).reshape(-1, 3)
    d_s = torch.from_numpy(a[:, 0].copy().view(np.int64)).cuda()
    d_l = torch.from_numpy(a[:, 1].astype(np.uint32).view(np.int32)).cuda()
    d_q = torch.from_numpy(a[:, 2].copy().view(np.int64)).cuda()
    d_m = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert d_text.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    eng.quality_mask_device(d_text.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), d_q.data_ptr(), len(recs), q, d_out.data_ptr(),
                            d_masked=d_m.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), int(d_m.cpu()[0])


def error_bit_is_clear(eng):
    """the sticky error word is read by the next blocking call: a clean word lets it pass"""
    eng.classify(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), np.array([0, 80], dtype=np.uint64))


def check(eng, tx, q, bad=()):
    want, want_n = reference(tx.t, tx.recs, q, bad)
    got, got_n = launch(eng, tx.t, tx.recs, q)
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, "Q %d: %d bytes differ, first at %d (got %r, want %r); records %r" % (
        q, diff.size, diff[0], bytes(got[diff[0]:diff[0] + 8]), bytes(want[diff[0]:diff[0] + 8]), tx.recs[:4])
    assert got_n == want_n
    return want_n


@pytest.mark.parametrize("q", [1, 20, 93])
def test_lengths_0_to_9_at_every_pair_of_residues(toy_engine, q):
    tx = Text(np.random.default_rng(q))
    for n in range(10):
        for rs in range(4):
            for rq in range(4):
                tx.fastq(n, rs, rq)
    assert {(s % 4, qs % 4) for s, n, qs in tx.recs if n == 9} == {(a, b) for a in range(4) for b in range(4)}
    assert check(toy_engine, tx, q) > 0
    error_bit_is_clear(toy_engine)


@pytest.mark.parametrize("q", [1, 20, 93])
def test_lengths_around_every_step(toy_engine, q):
    """63 .. 257 (chunks of a team's first and second step), 500 .. 530 (where the workgroup takes over from the team), 4600
    and 8705 (more than one step of the workgroup), 70 000 (many steps of one record); residues in turn"""
    tx = Text(np.random.default_rng(100 + q))
    lens = [63, 64, 65, 255, 256, 257, 500, 509, 511, 512, 513, 516, 530, 4600, 8705, 70_000, 15, 16, 17, 31, 32, 33]
    for i, n in enumerate(lens):
        tx.fastq(n, i % 4, (i // 4 + i) % 4)
    assert len(tx.recs) > 16  # more than one workgroup
    assert check(toy_engine, tx, q) > 0
    error_bit_is_clear(toy_engine)


def test_sequences_one_byte_apart(toy_engine):
    """the sequences in a row with one byte between them, the qualities in a row behind: neighbours share their first and last
    dwords, whatever the lengths"""
    rng = np.random.default_rng(7)
    tx = Text(rng)
    lens = [1, 2, 3, 4, 5, 7, 8, 9, 3, 1, 1, 16, 17, 2, 33, 6, 150, 151, 149, 3, 600, 1, 2]
    starts = []
    for n in lens:
        starts.append(tx.put(tx.bases(n)))
        tx.t += b"\n"
    tx.t += b"##"
    for s, n in zip(starts, lens):
        qs = tx.put(tx.quals(n, 33, 80))
        tx.t += b"\n"
        tx.recs.append((s, n, qs))
    assert check(toy_engine, tx, 20) > 0
    error_bit_is_clear(toy_engine)


def test_fasta_record_between_fastq_records(toy_engine):
    tx = Text(np.random.default_rng(8))
    for i in range(40):
        if i % 3 == 1:
            tx.fasta([0, 5, 150, 700, 5000][i % 5], i % 4)
        else:
            tx.fastq([151, 3, 76, 2000][i % 4], i % 4, (i + 1) % 4, 33, 70)
    masked = check(toy_engine, tx, 20)
    assert masked > 0
    want, _ = reference(tx.t, tx.recs, 20)
    t = np.frombuffer(bytes(tx.t), dtype=np.uint8)
    for s, n, qs in tx.recs:
        if qs == NONE:
            assert np.array_equal(want[s:s + n], t[s:s + n])
    error_bit_is_clear(toy_engine)


@pytest.mark.parametrize("q", [1, 20, 93])
def test_nothing_masked_and_everything_masked(toy_engine, q):
    hi = Text(np.random.default_rng(9))
    lo = Text(np.random.default_rng(10))
    for i, n in enumerate([150, 151, 9, 1000, 64, 0, 5000]):
        hi.fastq(n, i % 4, (i + 2) % 4, 33 + q, 126)   # every quality at the threshold or above: nothing
        lo.fastq(n, i % 4, (i + 3) % 4, 33, 33 + q - 1)  # every quality below
    assert check(toy_engine, hi, q) == 0
    assert check(toy_engine, lo, q) == sum(n for _s, n, _q in lo.recs)
    got, _ = launch(toy_engine, lo.t, lo.recs, q)
    for s, n, _qs in lo.recs:
        assert bytes(got[s:s + n]) == b"N" * n


def test_quality_line_of_another_length(toy_engine):
    """a well-formed text; the quality starts of four records point at the quality line of a neighbour that is shorter or
    longer (among them a long record, whose line the whole workgroup reads first), and one record lies outside the text:
    the error bit is set, nothing is written for these, every other record is as it should be"""
    from nohuman_amd import EngineError
    tx = Text(np.random.default_rng(11))
    lens = [150, 120, 150, 9, 12, 150, 6000, 5000, 150, 33, 150, 150, 150, 77, 150, 150, 150, 150, 40]
    for i, n in enumerate(lens):
        tx.fastq(n, i % 4, (i + 1) % 4, 33, 80)
    r = list(tx.recs)  # (a copy: the quality starts are swapped between records below)
    bad = {0: 1, 3: 4, 4: 3, 6: 7, 7: 6}  # record -> the record whose quality line it is given
    assert all(lens[a] != lens[b] for a, b in bad.items())
    for a, b in bad.items():
        tx.recs[a] = (r[a][0], r[a][1], r[b][2])
    assert all(tx.recs[a][2] == r[b][2] != r[a][2] for a, b in bad.items())
    tx.recs[12] = (len(tx.t) - 100, 150, r[12][2])  # the sequence runs past the text
    tx.recs[14] = (r[14][0], r[14][1], len(tx.t) - 10)  # the qualities do
    check(toy_engine, tx, 20, bad=set(bad) | {12, 14})
    with pytest.raises(EngineError) as ei:
        error_bit_is_clear(toy_engine)
    assert "quality" in ei.value.message
    error_bit_is_clear(toy_engine)  # read once, the word is clean again
    for q in (94, 200):
        with pytest.raises(EngineError) as ei:
            launch(toy_engine, tx.t, tx.recs, q)
        assert ei.value.code == -1
