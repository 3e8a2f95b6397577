"""Symmetric DUST (Morgulis et al. 2006) at dustmasker's defaults -- window 64 bases, score threshold 2.0 -- as DESIGN.md 6.10
defines it: the model that nh_dust_mask and the masking builder are compared with, bit for bit.

  runs        maximal stretches of ACGTacgt; every other byte ends a run, is never masked and never counted
  triplets    t_i = the code (0..63) of bases i, i+1, i+2 of a run
  score       of the triplet interval [i, i+d]: r / d with r = sum over the 64 codes of n_c (n_c - 1) / 2
  perfect     d <= 61, 10 r > 20 d, and no sub-interval with a higher score (a tie does not disqualify)
  masked      the union of the bases of all perfect intervals

mask_brute reads that literally (every interval, every sub-interval); mask is the data-parallel recurrence the kernel runs,
vectorised over the starts of a run.  All arithmetic is in integers; scores are compared by cross-multiplication."""
from __future__ import annotations

import numpy as np

MAX_D = 61  # 62 triplets = 64 bases

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i


def runs(seq: bytes):
    """(start, end) of every maximal run of ACGTacgt"""
    c = _CODE[np.frombuffer(seq, np.uint8)] < 4
    edges = np.flatnonzero(np.diff(np.concatenate([[0], c.astype(np.int8), [0]])))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def _triplets(codes):
    c = codes.astype(np.int64)
    return c[:-2] * 16 + c[1:-1] * 4 + c[2:]


def _run_mask(codes) -> np.ndarray:
    """the recurrence over one run (2-bit codes) -> bool per base"""
    L = codes.size
    out = np.zeros(L, bool)
    nt = L - 2
    if nt < 2:
        return out
    t = _triplets(codes)
    r1 = np.zeros(nt, np.int64)  # r_{d-1}
    r2 = np.zeros(nt, np.int64)  # r_{d-2}
    mn = np.zeros(nt, np.int64)  # M_{d-1} = mn / md
    md = np.ones(nt, np.int64)
    reach = np.zeros(nt, np.int64)
    for d in range(1, min(MAX_D, nt - 1) + 1):
        m = nt - d  # starts 0 .. m-1 have their triplet i + d inside the run
        r = r1[:m] + r1[1:m + 1] - r2[1:m + 1] + (t[:m] == t[d:d + m])
        an, ad, bn, bd = mn[:m], md[:m], mn[1:m + 1], md[1:m + 1]
        nb = bn * ad > an * bd
        Bn, Bd = np.where(nb, bn, an), np.where(nb, bd, ad)
        ge = r * Bd >= Bn * d
        perfect = ge & (10 * r > 20 * d)
        reach[:m][perfect] = d + 3
        new_n, new_d = np.where(ge, r, Bn), np.where(ge, d, Bd)
        r2[:] = r1
        r1[:m] = r
        mn[:m] = new_n
        md[:m] = new_d
    end = np.where(reach > 0, np.arange(nt) + reach, 0)
    pm = np.maximum.accumulate(end)
    b = np.arange(L)
    out[:] = pm[np.minimum(b, nt - 1)] > b
    return out


def mask_bool(seq: bytes) -> np.ndarray:
    """bool per byte of one sequence: masked or not"""
    codes = _CODE[np.frombuffer(seq, np.uint8)]
    out = np.zeros(len(seq), bool)
    for a, b in runs(seq):
        out[a:b] = _run_mask(codes[a:b])
    return out


def apply(seq: bytes, m: np.ndarray) -> bytes:
    s = np.frombuffer(seq, np.uint8).copy()
    s[m] = ord("N")
    return s.tobytes()


def mask(seq: bytes) -> bytes:
    """the sequence with every masked base as N"""
    return apply(seq, mask_bool(seq))


def masked_count(seq: bytes) -> int:
    return int(mask_bool(seq).sum())


def _run_brute(codes) -> np.ndarray:
    L = codes.size
    out = np.zeros(L, bool)
    nt = L - 2
    if nt < 2:
        return out
    t = _triplets(codes)
    D = MAX_D + 1
    R = np.zeros((nt, D), np.int64)       # R[i, d] = r of [i, i + d]
    there = np.zeros((nt, D), bool)       # the interval lies in the run
    tl = t.tolist()
    for i in range(nt):
        n, r = [0] * 64, 0  # n_c of [i, i + d]; one more occurrence of code c adds n_c pairs to sum n_c (n_c - 1) / 2
        for d in range(0, min(MAX_D, nt - 1 - i) + 1):
            c = tl[i + d]
            r += n[c]
            n[c] += 1
            R[i, d] = r
            there[i, d] = True
    dd = np.arange(D)[None, :]
    for i in range(nt):
        for d in range(1, D):
            if not there[i, d] or not 10 * R[i, d] > 20 * d:
                continue
            # sub-intervals [i', i' + d'] with i <= i', i' + d' <= i + d, d' >= 1: a higher score r'/d' > r/d disqualifies
            sub = R[i:i + d + 1, :d + 1]
            ii = np.arange(sub.shape[0])[:, None]
            inside = (ii + dd[:, :d + 1] <= d) & (dd[:, :d + 1] >= 1)
            if np.any(inside & (sub * d > R[i, d] * dd[:, :d + 1])):
                continue
            out[i:i + d + 3] = True
    return out


def mask_brute_bool(seq: bytes) -> np.ndarray:
    codes = _CODE[np.frombuffer(seq, np.uint8)]
    out = np.zeros(len(seq), bool)
    for a, b in runs(seq):
        out[a:b] = _run_brute(codes[a:b])
    return out


def mask_brute(seq: bytes) -> bytes:
    """the definition read literally: all intervals, all sub-intervals"""
    return apply(seq, mask_brute_bool(seq))


# ---- generators of low-complexity sequence ---------------------------------------------------------------------------------
def iid(rng, n, weights=None) -> bytes:
    p = None if weights is None else np.asarray(weights, float) / sum(weights)
    return np.frombuffer(b"ACGT", np.uint8)[rng.choice(4, size=n, p=p)].tobytes()


def homopolymer(rng, n) -> bytes:
    return bytes([b"ACGT"[int(rng.integers(0, 4))]]) * n


def periodic(rng, n, period) -> bytes:
    unit = iid(rng, period)
    return (unit * (n // period + 1))[:n]


def biased(rng, n) -> bytes:
    w = [10, 10, 10, 10]
    w[int(rng.integers(0, 4))] = 70
    return iid(rng, n, w)


def stretch(rng, n) -> bytes:
    """one low-complexity stretch of n bases: a homopolymer, a repeat of period 2..7 or a 70/10/10/10 stretch"""
    k = int(rng.integers(0, 8))
    if k == 0:
        return homopolymer(rng, n)
    if k <= 6:
        return periodic(rng, n, k + 1)
    return biased(rng, n)


def mixed(rng, n, flank=20, longest=90, n_share=0.0, lower_share=0.0) -> bytes:
    """n bases: stretches of 3..longest bases between iid flanks of 0..flank bases; a share of the positions turned into N,
    a share of the stretches in lowercase"""
    out = bytearray()
    while len(out) < n:
        s = stretch(rng, int(rng.integers(3, longest + 1)))
        if lower_share and rng.random() < lower_share:
            s = s.lower()
        out += s
        out += iid(rng, int(rng.integers(0, flank + 1)))
    out = out[:n]
    if n_share:
        for p in np.flatnonzero(rng.random(n) < n_share):
            out[int(p)] = ord("N")
    return bytes(out)


def plant(rng, seq: bytes, lengths, gap=37) -> tuple[bytes, list]:
    """stretches of the given lengths planted into seq at positions that are no multiple of anything (a prime-ish gap that
    grows with the index) -> (sequence, [(position, length)])"""
    s = bytearray(seq)
    pos, where = 11, []
    for j, n in enumerate(lengths):
        if pos + n > len(s):
            break
        s[pos:pos + n] = stretch(rng, n)
        where.append((pos, n))
        pos += n + gap + 2 * (j % 29) + 1
    return bytes(s), where


# ---- a masked FASTA against this mask (PINDAY.md 2b): python -m tests.dust_model genome.fa genome.masked.fa ----------------
def read_fasta(path):
    name, parts, out = None, [], []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(parts)))
                name, parts = line[1:].split()[0] if line[1:].split() else b"", []
            elif name is not None:
                parts.append(line)
    if name is not None:
        out.append((name, b"".join(parts)))
    return out


def compare(plain_path, masked_path) -> int:
    """prints, per record, how this mask of plain_path differs from masked_path (masked there: x, X, n, N or lowercase where
    the plain file has an uppercase base) -> the number of bases that differ"""
    plain, other = read_fasta(plain_path), dict(read_fasta(masked_path))
    bad = 0
    for name, s in plain:
        o = np.frombuffer(other.get(name, b""), np.uint8)
        if o.size != len(s):
            print("%s: %d bases here, %d there" % (name.decode(errors="replace"), len(s), o.size))
            bad += abs(len(s) - o.size) or 1
            continue
        p = np.frombuffer(s, np.uint8)
        theirs = (o != p) & (np.isin(o, np.frombuffer(b"xXnN", np.uint8)) | (o >= 97))
        diff = np.flatnonzero(mask_bool(s) != theirs)
        if diff.size:
            print("%s: %d of %d bases differ, the first at %d" % (name.decode(errors="replace"), diff.size, len(s), diff[0]))
        bad += int(diff.size)
    print("IDENTICAL" if not bad else "%d bases differ" % bad)
    return bad


if __name__ == "__main__":
    import sys
    sys.exit(1 if compare(sys.argv[1], sys.argv[2]) else 0)
