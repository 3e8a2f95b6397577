"""k_rstats on the GPU (nh_read_stats_device, nohuman_amd/csrc/nh_rstats.hip): the four accumulators -- all 4 x 102 words --
against the numpy model of tests/rstats_model.py, on texts built here: every pair of residues mod 4 of the bases and the
qualities, lengths around the kernel's chunk (16 bytes), team (512 bytes) and workgroup steps (4096 bytes), sequences one byte
apart, records without qualities, both classes inside one group of 16 and a group all of one class, paired launches, binned and
uniform qualities, quality bytes outside the printable range, a capped grid, two launches into one accumulator, and quality
lines that are not as long as their sequence.  Every record lies inside its text.  (A byte 10 inside a quality line is, for this
entry, the end of the line: the model's own tests cover its bin.)"""
import numpy as np
import pytest

from tests import rstats_model as rm

pytestmark = pytest.mark.gpu
NONE = rm.NONE
BASES = b"ACGTacgtNnR-"
BINNED = bytes([33 + 2, 33 + 12, 33 + 23, 33 + 37])  # Illumina's four quality values


class Text:
    """a batch text under construction: records of (sequence start, length, quality start)"""

    def __init__(self, rng):
        self.rng, self.t, self.recs = rng, bytearray(), []

    def pad_to(self, residue):
        """filler (no line ends: they must not look like a quality line's end) up to an offset of the residue mod 4"""
        while len(self.t) % 4 != residue:
            self.t += b"#"

    def put(self, data):
        at = len(self.t)
        self.t += data
        return at

    def bases(self, n):
        return self.rng.choice(np.frombuffer(BASES, dtype=np.uint8), size=n).tobytes()

    def quals(self, n, lo=33, hi=126, alphabet=None):
        if alphabet is not None:  # runs of 1 .. 40 equal bytes, as binned qualities come
            out = bytearray()
            while len(out) < n:
                out += bytes([alphabet[int(self.rng.integers(0, len(alphabet)))]]) * int(self.rng.integers(1, 41))
            return bytes(out[:n])
        return self.rng.integers(lo, hi + 1, size=n).astype(np.uint8).tobytes()

    def fastq(self, n, rs=None, rq=None, **kw):
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
        q = self.put(self.quals(n, **kw))
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


def new_acc():
    import torch
    a = rm.empty()
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def launch(eng, text, recs, calls, mates=1, max_workgroups=0, d_acc=None):
    """one launch -> the accumulators as a (2, 2, 102) uint64 array (d_acc: added to, returned as well)"""
    import torch
    n = len(text)
    t = torch.zeros(n + 8, dtype=torch.uint8)
    t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    d_text = t.cuda()
    a = np.array(recs, dtype=np.uint64).reshape(-1, 3)
    assert len(recs) == len(calls) * mates and all(s + ln <= n and (q == NONE or q + ln <= n) for s, ln, q in recs)
    d_s = torch.from_numpy(a[:, 0].copy().view(np.int64)).cuda()
    d_l = torch.from_numpy(a[:, 1].astype(np.uint32).view(np.int32)).cuda()
    d_q = torch.from_numpy(a[:, 2].copy().view(np.int64)).cuda()
    res = np.zeros((len(calls), 4), dtype=np.uint32)
    res[:, 0] = np.asarray(calls, dtype=np.uint32)
    res[:, 1:] = 0xABCD  # (only `call` is read)
    d_r = torch.from_numpy(res.view(np.int32)).cuda()
    if d_acc is None:
        d_acc = new_acc()
    assert d_text.data_ptr() % 4 == 0 and d_acc.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    eng.read_stats_device(d_text.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), d_q.data_ptr(), d_r.data_ptr(), len(calls),
                          d_acc.data_ptr(), paired=mates == 2, max_workgroups=max_workgroups)
    torch.cuda.synchronize()
    return d_acc.cpu().numpy().view(np.uint64).reshape(2, 2, rm.WORDS), d_acc


def error_bit_is_clear(eng):
    """the sticky error word is read by the next blocking call: a clean word lets it pass"""
    eng.classify(np.frombuffer(b"ACGT" * 20, dtype=np.uint8), np.array([0, 80], dtype=np.uint64))


def same(got, want):
    diff = np.argwhere(got != want)
    assert diff.size == 0, "%d words differ: %s" % (len(diff), [(tuple(int(x) for x in d), int(got[tuple(d)]), int(want[tuple(d)])) for d in diff[:8]])


def check(eng, tx, calls, mates=1, bad=(), **kw):
    want = rm.accumulate(rm.reads_of_text(tx.t, tx.recs, calls, mates, bad))
    got, _ = launch(eng, tx.t, tx.recs, calls, mates, **kw)
    same(got, want)
    return want


def alternate(n, period=3):
    """calls with both classes inside every group of 16"""
    return [(7 if i % period == 0 else 0) for i in range(n)]


def test_lengths_0_to_9_at_every_pair_of_residues(toy_engine):
    tx = Text(np.random.default_rng(1))
    for n in range(10):
        for rs in range(4):
            for rq in range(4):
                tx.fastq(n, rs, rq)
    assert {(s % 4, qs % 4) for s, n, qs in tx.recs if n == 9} == {(a, b) for a in range(4) for b in range(4)}
    want = check(toy_engine, tx, alternate(len(tx.recs)))
    assert int(want[0, 0, rm.READS]) > 0 and int(want[1, 0, rm.READS]) > 0 and int(want[:, 0, rm.MIN_LEN].max()) == 0
    assert int(want[:, 0, rm.OTHER].sum()) > 0
    error_bit_is_clear(toy_engine)


@pytest.mark.parametrize("kind", ["uniform", "binned"])
def test_lengths_around_every_step(toy_engine, kind):
    """chunk, team and workgroup steps, and one record of many steps; residues in turn; qualities 33 .. 126 or four values"""
    tx = Text(np.random.default_rng(2))
    lens = [0, 1, 3, 4, 5, 15, 16, 17, 511, 512, 513, 4095, 4096, 4097, 70_001, 63, 64, 65, 255, 256, 257, 500, 509, 516, 530, 8705]
    kw = dict(alphabet=BINNED) if kind == "binned" else {}
    for i, n in enumerate(lens):
        tx.fastq(n, i % 4, (i // 4 + i) % 4, **kw)
    assert len(tx.recs) > 16  # more than one group
    want = check(toy_engine, tx, alternate(len(tx.recs), 2))
    hist = want[:, 0, 8:].sum(axis=0)
    assert int((hist > 0).sum()) == (4 if kind == "binned" else 94)
    assert int(want[:, 0, rm.MAX_LEN].max()) == 70_001
    error_bit_is_clear(toy_engine)


def test_sequences_one_byte_apart(toy_engine):
    """the sequences in a row with one byte between them, the qualities in a row behind: neighbours share their first and last
    dwords, whatever the lengths"""
    tx = Text(np.random.default_rng(3))
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
    check(toy_engine, tx, alternate(len(lens)))
    error_bit_is_clear(toy_engine)


def test_fasta_records_among_fastq_records(toy_engine):
    tx = Text(np.random.default_rng(4))
    for i in range(40):
        if i % 3 == 1:
            tx.fasta([0, 5, 150, 700, 5000][i % 5], i % 4)
        else:
            tx.fastq([151, 3, 76, 2000][i % 4], i % 4, (i + 1) % 4, lo=33, hi=70)
    want = check(toy_engine, tx, alternate(40, 2))
    assert 0 < int(want[:, 0, rm.QUAL_READS].sum()) < int(want[:, 0, rm.READS].sum()) == 40
    assert int(want[:, 0, rm.QUAL_BASES].sum()) == int(want[:, 0, 8:].sum()) < int(want[:, 0, rm.BASES].sum())
    error_bit_is_clear(toy_engine)


def test_a_group_all_of_one_class_and_groups_of_both(toy_engine):
    """48 reads: the first group of 16 all non-human, the second all human, the third mixed; then no human read at all: the
    human accumulators stay as the caller left them (min_len all-ones)"""
    tx = Text(np.random.default_rng(5))
    for i in range(48):
        tx.fastq([150, 151, 149, 37, 600][i % 5], i % 4, (i + 2) % 4, alphabet=BINNED)
    calls = [0] * 16 + [5] * 16 + alternate(16, 2)
    want = check(toy_engine, tx, calls)
    assert int(want[1, 0, rm.READS]) == 24 and int(want[0, 0, rm.READS]) == 24
    want = check(toy_engine, tx, [0] * 48)
    assert int(want[1, 0, rm.MIN_LEN]) == NONE and int(want[1, 0].sum()) == NONE


def test_paired_class_by_fragment_mate_by_parity(toy_engine):
    """sequences 2f and 2f + 1 are the mates of fragment f: both take its class; mate 2 is shorter, and FASTA in the second text"""
    rng = np.random.default_rng(6)
    for fasta2 in (False, True):
        tx = Text(rng)
        for f in range(37):
            tx.fastq([150, 100, 250, 5][f % 4], f % 4, (f + 1) % 4, lo=33, hi=74)
            if fasta2:
                tx.fasta([60, 0, 700][f % 3], (f + 2) % 4)
            else:
                tx.fastq([60, 0, 700][f % 3], (f + 2) % 4, (f + 3) % 4, lo=50, hi=60)
        calls = alternate(37)
        want = check(toy_engine, tx, calls, mates=2)
        n_h = sum(1 for c in calls if c)
        assert [int(want[c, m, rm.READS]) for c in range(2) for m in range(2)] == [37 - n_h, 37 - n_h, n_h, n_h]
        assert int(want[:, 0, rm.MAX_LEN].max()) == 250 and int(want[:, 1, rm.MAX_LEN].max()) == 700
        assert (int(want[:, 1, rm.QUAL_READS].sum()) == 0) == fasta2
    error_bit_is_clear(toy_engine)


def test_quality_bytes_outside_the_printable_range(toy_engine):
    """32, 127 and 255 inside a quality line (a byte up to ' ' behind the line ends it; inside it is a quality): bins 0 and 93"""
    tx = Text(np.random.default_rng(7))
    odd = bytes([32, 127, 255, 33, 126, 128, 1, 31])
    for i, n in enumerate([150, 9, 16, 33, 700, 4100]):
        tx.fastq(n, i % 4, (i + 3) % 4, alphabet=odd)
    want = check(toy_engine, tx, alternate(len(tx.recs), 2))
    hist = want[:, 0, 8:].sum(axis=0)
    assert int(hist[0]) > 0 and int(hist[93]) > 0 and int(hist[1:93].sum()) == 0
    error_bit_is_clear(toy_engine)


def test_capped_grid_loops_and_flushes_once(toy_engine):
    """100 sequences (7 groups of 16) on 2, 1 and 3 workgroups and on the default grid: the same words"""
    tx = Text(np.random.default_rng(8))
    for i in range(100):
        tx.fastq([150, 151, 76, 1000, 0, 5000][i % 6], i % 4, (i + 1) % 4, alphabet=BINNED)
    calls = alternate(100)
    want = check(toy_engine, tx, calls, max_workgroups=2)
    for cap in (1, 3, 0, 1000):
        got, _ = launch(toy_engine, tx.t, tx.recs, calls, max_workgroups=cap)
        same(got, want)
    error_bit_is_clear(toy_engine)


def test_two_launches_into_one_accumulator(toy_engine):
    rng = np.random.default_rng(9)
    a, b = Text(rng), Text(rng)
    for i in range(20):
        a.fastq([150, 40, 600][i % 3], i % 4, (i + 1) % 4)
        b.fastq([90, 3, 5000][i % 3], (i + 2) % 4, i % 4, alphabet=BINNED)
    ca, cb = alternate(20, 2), alternate(20, 5)
    first = rm.accumulate(rm.reads_of_text(a.t, a.recs, ca))
    want = rm.accumulate(rm.reads_of_text(b.t, b.recs, cb), first)
    got, d_acc = launch(toy_engine, a.t, a.recs, ca)
    same(got, first)
    got, _ = launch(toy_engine, b.t, b.recs, cb, d_acc=d_acc)
    same(got, want)
    assert int(want[0, 0, rm.MIN_LEN]) == 3 and int(want[:, 0, rm.MAX_LEN].max()) == 5000


def test_quality_line_of_another_length(toy_engine):
    """a well-formed text; the quality starts of five records point at the quality line of a neighbour that is shorter or
    longer (among them two long records, whose line the whole workgroup reads first), and one quality line holds a line end:
    these records are not counted at all, every other record is, the error bit fails the next blocking call once"""
    from nohuman_amd import EngineError
    tx = Text(np.random.default_rng(11))
    lens = [150, 120, 150, 9, 12, 150, 6000, 5000, 150, 33, 150, 150, 150, 77, 150, 150, 150, 150, 40]
    for i, n in enumerate(lens):
        tx.fastq(n, i % 4, (i + 1) % 4, lo=33, hi=80)
    r = list(tx.recs)  # (a copy: the quality starts are swapped between records below)
    bad = {0: 1, 3: 4, 4: 3, 6: 7, 7: 6}  # record -> the record whose quality line it is given
    assert all(lens[a] != lens[b] for a, b in bad.items())
    for a, b in bad.items():
        tx.recs[a] = (r[a][0], r[a][1], r[b][2])
    tx.t[r[13][2] + 40] = 10  # a line end inside record 13's quality line: the line is shorter than its sequence
    n = len(tx.t)
    assert all(s + ln <= n and q + ln <= n for s, ln, q in tx.recs)  # no record leaves the text
    calls = alternate(len(lens), 2)
    want = check(toy_engine, tx, calls, bad=set(bad) | {13})
    assert int(want[:, 0, rm.READS].sum()) == len(lens) - 6
    with pytest.raises(EngineError) as ei:
        error_bit_is_clear(toy_engine)
    assert "quality" in ei.value.message
    error_bit_is_clear(toy_engine)  # read once, the word is clean again


def test_arguments(toy_engine):
    from nohuman_amd import EngineError
    with pytest.raises(EngineError) as ei:
        toy_engine.read_stats_device(0, 0, 0, 0, 0, 0, 0, 0)
    assert ei.value.code == -1
