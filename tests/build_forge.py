"""Forged inputs for the tests of nh_build_db: minimizers made to order, and the order-free specification of a table.

fmix64 is a bijection of the 64-bit words, so the cell a minimizer starts its probe at (fmix64(m) % capacity) and the key it leaves
there (fmix64(m) >> 34) can be chosen: pick the hash, invert it, keep the preimages that are legal minimizers (below 2^62, no bit
outside the default spaced mask: about 2^-16 of all words) and wrap each in a 35-base record whose only k-mer has that minimizer.
That reaches what random genomes of test size never do: two distinct minimizers with one compacted key on one probe path, probe
paths that wrap round the table's end, tables with one empty cell, the last slot of the counting set.

Where keys are shared the table depends on the order of insertion, so build_db_util.same_table no longer says what a correct
table is; valid_table does, for any order.  CPU only: numpy, oracle/ and build_db_util."""
from __future__ import annotations

import math

import numpy as np

from oracle import k2_literal as lit
from oracle import minidb
from tests import build_db_util as u

M64 = (1 << 64) - 1
SPACED = minidb.default_spaced_mask()
KEY_SHIFT = 32 + u.VALUE_BITS
KEY_MAX = (1 << (64 - KEY_SHIFT)) - 1  # 2^30 - 1
MAX_TARGET_CAPACITY = 4099
_C1, _C2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
_I1, _I2 = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)
_CHUNK = 1 << 20
_BASES = b"ACGT"
# the seven bases of an l-mer that the spaced mask drops, counted from the l-mer's first base
_MASKED = [i for i in range(minidb.DEFAULT_L) if not (SPACED >> (2 * (minidb.DEFAULT_L - 1 - i))) & 3]
assert len(_MASKED) == 7


def inv_fmix64(h: int) -> int:
    """the word whose fmix64 is h (x ^= x >> 33 undoes itself: the shift is more than half the word)"""
    h ^= h >> 33
    h = (h * _I2) & M64
    h ^= h >> 33
    h = (h * _I1) & M64
    h ^= h >> 33
    return h


def inv_fmix64_np(h):
    h = np.asarray(h).astype(np.uint64).copy()
    s = np.uint64(33)
    h ^= h >> s
    h *= np.uint64(_I2)
    h ^= h >> s
    h *= np.uint64(_I1)
    h ^= h >> s
    return h


def _progression(capacity, home, low_ones):
    """(a, L): the hashes with h % capacity == home and the low `low_ones` bits set are h = a + L t"""
    P = 1 << low_ones
    ones = P - 1
    g = math.gcd(P, capacity)
    if (home - ones) % g:
        raise ValueError("no hash has home %d of %d and %d low ones" % (home, capacity, low_ones))
    c = capacity // g
    t0 = ((home - ones) // g * pow(P // g, -1, c)) % c if c > 1 else 0
    return ones + P * t0, P * c


def _hash_chunks(capacity, home, key, low_ones):
    """the hashes asked for, as uint64 arrays, every one exactly once.  With a key: the 2^34 / L of them under that key, in
    rising order.  Without: all 2^64 / L, in passes whose neighbours lie 2^44 apart, so that a pass runs through all keys."""
    a, L = _progression(capacity, home, low_ones)
    if key is not None:
        lo, hi = key << KEY_SHIFT, (key + 1) << KEY_SHIFT
        first = lo + (a - lo) % L
        total = max(0, -(-(hi - first) // L))
        for t in range(0, total, _CHUNK):
            n = min(_CHUNK, total - t)
            yield np.uint64(first + L * t) + np.uint64(L) * np.arange(n, dtype=np.uint64)
        return
    Q = max(1, (1 << 44) // L)
    for j in range(Q):
        first = a + L * j
        total = -(-((1 << 64) - first) // (L * Q))
        for t in range(0, total, _CHUNK):
            n = min(_CHUNK, total - t)
            yield np.uint64(first + L * Q * t) + np.uint64(L * Q) * np.arange(n, dtype=np.uint64)


def iter_minimizers(capacity, home, key=None, low_ones=0):
    """forge_minimizers without an end: every legal minimizer of the target, in the order of _hash_chunks"""
    assert 0 <= home < capacity and 0 <= low_ones < 64 and (key is None or 0 <= key <= KEY_MAX)
    assert key is None or capacity <= MAX_TARGET_CAPACITY, "a (key, home) target has about 2^18 / capacity preimages"
    illegal = np.uint64(~SPACED & M64)
    for hs in _hash_chunks(capacity, home, key, low_ones):
        ms = inv_fmix64_np(hs)
        for m in ms[(ms & illegal) == 0]:
            yield int(m)


def forge_minimizers(capacity, home, key=None, n=1, low_ones=0):
    """n distinct minimizers m with fmix64(m) % capacity == home; fmix64(m) >> 34 == key where a key is given; the low
    `low_ones` bits of fmix64(m) all ones (then the probe for m starts at the last slot of every power-of-two set of up to
    2^low_ones slots).  Every m is below 2^62 and has no bit outside the default spaced mask, which about 2^-16 of all preimages
    do; a (key, home) pair has only 2^34 / capacity hashes, so about 2^18 / capacity legal preimages: targets with a key are for
    capacities of at most 4099 (64 preimages to choose from).  The arithmetic progression of the hashes is enumerated, not
    sampled: the same call gives the same list.  ValueError where the target has fewer than n."""
    out = []
    for m in iter_minimizers(capacity, home, key, low_ones):
        if len(out) == n:
            break
        out.append(m)
    if len(out) < n:
        raise ValueError("only %d of %d minimizers for home %d of %d, key %r, %d low ones" % (len(out), n, home, capacity, key, low_ones))
    return out


def _lmer_bytes(x):
    return bytes(_BASES[(x >> (2 * (minidb.DEFAULT_L - 1 - i))) & 3] for i in range(minidb.DEFAULT_L))


def record_for(m, rng, tries=48):
    """a 35-base record whose one k-mer has the minimizer m, or None.  The seven bases that the spaced mask drops are filled so
    that the l-mer is not above its reverse complement (then it is the canonical one and m is what the mask leaves of it); no
    fill does that where m's first base exceeds the complement of its last.  Zero to four random bases go in front and the rest
    of four behind; the record is accepted when k2_literal.kmer_minimizers gives exactly [(False, m)], i.e. when none of the
    other four l-mers of the k-mer beats m."""
    L = minidb.DEFAULT_L
    assert 0 <= m < 1 << 62 and not m & ~SPACED
    if (m >> (2 * (L - 1))) & 3 > 3 - (m & 3):
        return None
    shim = u._shim()
    for _ in range(tries):
        x = m
        for i, b in zip(_MASKED, rng.integers(0, 4, size=len(_MASKED))):
            x |= int(b) << (2 * (L - 1 - i))
        if x > lit.reverse_complement(x, L):
            continue
        front = int(rng.integers(0, 5))
        flank = bytes(_BASES[int(b)] for b in rng.integers(0, 4, size=4))
        seq = flank[:front] + _lmer_bytes(x) + flank[front:]
        if lit.kmer_minimizers(shim, seq) == [(False, m)]:
            return seq
    return None


def forge(capacity, targets, rng, low_ones=0, distinct_keys=False, exclude=()):
    """one (minimizer, 35-base record) per target, in the targets' order.  A target is (home, key) with key None for any key.
    All minimizers are distinct (and none is in `exclude`); with distinct_keys no two have one compacted key either.  A candidate
    that admits no record is passed over for the next of its target; a target that runs out of candidates raises.  Never fewer
    records than targets."""
    sources, used, used_keys, out = {}, set(exclude), set(), []
    for home, key in targets:
        src = sources.get((home, key))
        if src is None:
            src = sources[(home, key)] = iter_minimizers(capacity, home, key, low_ones)
        for m in src:
            k = lit.fmix64(m) >> KEY_SHIFT
            if m in used or (distinct_keys and k in used_keys):
                continue
            rec = record_for(m, rng)
            if rec is not None:
                used.add(m)
                used_keys.add(k)
                out.append((m, rec))
                break
        else:
            raise ValueError("no record for home %d of %d, key %r" % (home, capacity, key))
    assert len(out) == len(targets)
    return out


def _walk(cells, mins, capacity):
    """every minimizer's probe: (minimizers, keys, homes, cells walked until the key was found or 0 where an empty cell or the
    whole table came first)"""
    cells = np.asarray(cells).astype(np.int64)
    assert cells.size == capacity
    ms = np.array(sorted(int(m) for m in mins), dtype=np.uint64)
    hc = u.fmix64_np(ms)
    keys = (hc >> np.uint64(KEY_SHIFT)).astype(np.int64)
    homes = (hc % np.uint64(capacity)).astype(np.int64)
    length = np.zeros(ms.size, dtype=np.int64)
    live = np.arange(ms.size)
    for d in range(capacity):
        if live.size == 0:
            break
        c = cells[(homes[live] + d) % capacity]
        hit = (c != 0) & ((c >> u.VALUE_BITS) == keys[live])
        length[live[hit]] = d + 1
        live = live[~hit & (c != 0)]
    return ms, keys, homes, length


def probe_lengths(cells, mins, capacity):
    """cells walked from its home until each minimizer's key is found (home itself: 1), in the order of sorted(mins)"""
    ms, _, _, length = _walk(cells, mins, capacity)
    bad = np.flatnonzero(length == 0)
    assert bad.size == 0, "minimizer %#x is not found" % int(ms[bad[0]])
    return length


def valid_table(hdr, cells, mins, capacity, value=2):
    """what a one-taxon table built from the set `mins` is, in whatever order they went in:
    1. the header is (capacity, non-zero cells, 30, 2); every non-zero cell has the taxon's value and a key of some member of mins;
    2. every m in mins is found: walking from home(m), a cell with key(m) comes before any empty cell;
    3. every occupied cell p with key c is justified: some m in mins has key c, and every cell from home(m) up to but excluding p,
       cyclically, is occupied and none of them holds c (so the insertion of m could have claimed p) -- p is then the cell that
       the walk of point 2 ends at for that m;
    4. distinct keys <= size <= len(mins).
    Asserts each with the cell or minimizer at fault."""
    cells = np.asarray(cells)
    mins = set(int(m) for m in mins)
    occupied = np.flatnonzero(cells != 0)
    assert tuple(int(x) for x in hdr) == (capacity, occupied.size, 32 - u.VALUE_BITS, u.VALUE_BITS), \
        "header %r, but %d of %d cells are occupied" % (tuple(hdr), occupied.size, capacity)
    ms, keys, homes, length = _walk(cells, mins, capacity)
    vmask = (1 << u.VALUE_BITS) - 1
    wanted = set(keys.tolist())
    for p in occupied:
        c = int(cells[p])
        assert c & vmask == value, "cell %d holds value %d" % (p, c & vmask)
        assert c >> u.VALUE_BITS in wanted, "cell %d holds key %#x, which no minimizer has" % (p, c >> u.VALUE_BITS)
    bad = np.flatnonzero(length == 0)
    assert bad.size == 0, "minimizer %#x (home %d, key %#x) is not found before an empty cell" % (
        int(ms[bad[0]]), int(homes[bad[0]]), int(keys[bad[0]]))
    justified = set(((homes + length - 1) % capacity).tolist())
    for p in occupied:
        assert int(p) in justified, "cell %d (key %#x): no minimizer's probe ends there" % (p, int(cells[p]) >> u.VALUE_BITS)
    size = int(hdr[1])
    assert len(wanted) <= size <= len(mins), "%d keys, size %d, %d minimizers" % (len(wanted), size, len(mins))


def shared_key_records(capacity, rng, filler=21):
    """the input of the sequential-insertion tests, forged for `capacity` (56 cells or more, so that the homes below
    lie apart): (records, minimizers), in file order, every record 35 bases with one k-mer and a minimizer of its own.
      same3   three minimizers with one key and one home: one cell in any order
      zero    a foreign key, then key 0, both at one home: key 0 is no empty cell, and no match for a cell that was empty a moment ago
      acb     A and B with one key at homes h and h + 1, C with another key at home h, in the order A C B: B walks past C's cell and
              claims a third; reversed, B sits at h + 1 when A arrives there behind C and A adds no cell
      acb0    the same with key 0 for A and B and key 2^30 - 1 for C;  acbmax: the keys exchanged
      wrap    W1 W2 W3 with one key at homes capacity - 2, capacity - 1 and 0, X and Y with keys of their own at capacity - 2
              and capacity - 1, in the order W1 X W2 Y W3: W2 and Y wrap round the table's end
      fill    random 35-mers"""
    q = capacity // 8
    assert q >= 7
    k1, k2, k3, k4, k5, k6, k7 = 0x2AAAAAAA, 0x15555555, 0x0F0F0F0F, 0x33333333, 0x1C71C71C, 0x00000001, 0x3FFFFFFE
    groups = [
        ("same3", [(q, k1)] * 3),
        ("zero", [(5 * q, k7), (5 * q, 0)]),
        ("acb", [(2 * q, k2), (2 * q, k3), (2 * q + 1, k2)]),
        ("acb0", [(3 * q, 0), (3 * q, KEY_MAX), (3 * q + 1, 0)]),
        ("acbmax", [(4 * q, KEY_MAX), (4 * q, 0), (4 * q + 1, KEY_MAX)]),
        ("wrap", [(capacity - 2, k4), (capacity - 2, k5), (capacity - 1, k4), (capacity - 1, k6), (0, k4)]),
    ]
    targets = [t for _, ts in groups for t in ts]
    names = [b"%s_%d" % (g.encode(), i) for g, ts in groups for i in range(len(ts))]
    made = forge(capacity, targets, rng)
    recs = [(n, r) for n, (_, r) in zip(names, made)]
    mins = [m for m, _ in made]
    shim = u._shim()
    while len(recs) < len(targets) + filler:
        seq = bytes(_BASES[int(b)] for b in rng.integers(0, 4, size=35))
        (amb, m), = lit.kmer_minimizers(shim, seq)
        if not amb and m not in mins:
            recs.append((b"fill_%d" % len(recs), seq))
            mins.append(m)
    return recs, mins


def batches_of(seqs, batch_bytes):
    """how the builder lays sequences into batches of batch_bytes (nh_build.hip add_sequence, no masking): a sequence takes what
    room is left, down to 35 bases, and goes on in the next batch with the k-mer after its last -> a list of batches, each a list
    of (index of the sequence, its bases in that batch)"""
    out, used = [[]], 0
    for i, s in enumerate(seqs):
        pos = 0
        while pos < len(s) - 34:
            room = batch_bytes - used
            if room < 35:
                out.append([])
                used = 0
                continue
            take = min(len(s) - pos, room)
            out[-1].append((i, s[pos:pos + take]))
            used += take
            pos += take - 34
    return [b for b in out if b]


def counting_set_slots(seqs, batch_bytes):
    """the slots of the counting set while each batch of batches_of is counted: 65536 at first, doubled before a batch until
    slots >= 2 x (distinct minimizers so far + k-mers of the batch) + 64 -> (batches, slots per batch)"""
    batches = batches_of(seqs, batch_bytes)
    slots, cur, seen = [], 0, np.zeros(0, np.uint64)
    for b in batches:
        need = 2 * (seen.size + sum(len(c) - 34 for _, c in b)) + 64
        if need > cur:
            cur = cur or 1 << 16
            while cur < need:
                cur *= 2
        slots.append(cur)
        seen = np.union1d(seen, u.fast_minimizers([c for _, c in b]))
    return batches, slots


def last_slot_records(rng):
    """the input of the counting set's test: 60 forged records in three groups of 20 whose probes all start at the last slot of a
    set of 65536, 131072 or 262144 slots, and 180 kb of random sequence: group 1, 60 kb, group 2, 120 kb, group 3 (random
    sequence has a distinct minimizer every third base, and the second doubling comes at 45 000 of them plus a full batch).  Behind group 2
    comes group 1 once more, and behind group 3 groups 1 and 2: a key that was carried into a larger set is looked up there
    again, so one that the re-insertion left where a look-up does not pass shows as a minimizer counted twice.
    -> (records, forged minimizers, for each group the indices of its records, first copies first)"""
    from tests import synth
    made = forge(1, [(0, None)] * 60, rng, low_ones=18)
    g = [[(b"g%d_%d" % (j + 1, i), r) for i, (_, r) in enumerate(made[20 * j:20 * j + 20])] for j in range(3)]
    again = lambda recs, t: [(n + b"_again%d" % t, r) for n, r in recs]  # noqa: E731
    recs = g[0] + [(b"random_1", synth.random_seq(rng, 60_000))] + g[1] + again(g[0], 1) \
        + [(b"random_2", synth.random_seq(rng, 120_000))] + g[2] + again(g[0], 2) + again(g[1], 2)
    where = [[i for i, (n, _) in enumerate(recs) if n.startswith(b"g%d_" % (j + 1))] for j in range(3)]
    return recs, [m for m, _ in made], where
