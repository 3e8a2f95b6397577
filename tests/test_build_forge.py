"""tests/build_forge.py on the CPU: the inverse of fmix64, forged records under both scanners, the order-dependent A/B/C scenario
through the model, and valid_table on the model's tables and on spoiled ones."""
import itertools
import struct

import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import build_db_util as u
from tests import build_forge as bf

CAP = 1009


def test_inv_fmix64():
    rng = np.random.default_rng(1)
    words = np.concatenate([rng.integers(0, 1 << 64, size=2000, dtype=np.uint64), np.array([0, bf.M64, 1, 1 << 63], dtype=np.uint64)])
    assert np.array_equal(u.fmix64_np(bf.inv_fmix64_np(words)), words)
    assert np.array_equal(bf.inv_fmix64_np(u.fmix64_np(words)), words)
    for w in [int(x) for x in words[:200]] + [0, bf.M64]:
        assert lit.fmix64(bf.inv_fmix64(w)) == w and bf.inv_fmix64(lit.fmix64(w)) == w
        assert bf.inv_fmix64(w) == int(bf.inv_fmix64_np(np.array([w], dtype=np.uint64))[0])
    assert bf.inv_fmix64(0) == 0


TARGETS = [(0, 0), (CAP - 1, 0), (0, bf.KEY_MAX), (CAP - 1, bf.KEY_MAX), (10, 0x12345), (10, 0x12345), (11, 0x12345), (500, None)]


@pytest.fixture(scope="module")
def forged():
    return bf.forge(CAP, TARGETS, np.random.default_rng(2))


def test_forged_records(forged):
    assert len(forged) == len(TARGETS) and len({m for m, _ in forged}) == len(TARGETS)
    for (home, key), (m, rec) in zip(TARGETS, forged):
        assert len(rec) == 35 and set(rec) <= set(b"ACGT")
        assert m < 1 << 62 and not m & ~bf.SPACED
        hc = lit.fmix64(m)
        assert hc % CAP == home and (key is None or hc >> 34 == key)
        assert u.minimizers([rec]) == ({m}, 1, 0)
        assert u.fast_minimizers([rec]).tolist() == [m]


def test_forge_minimizers():
    ms = bf.forge_minimizers(CAP, 7, key=3, n=5)
    assert len(set(ms)) == 5 and ms == bf.forge_minimizers(CAP, 7, key=3, n=5)
    assert all(lit.fmix64(m) % CAP == 7 and lit.fmix64(m) >> 34 == 3 and not m & ~bf.SPACED for m in ms)
    ms = bf.forge_minimizers(1, 0, n=12, low_ones=18)
    assert len(set(ms)) == 12 and all(lit.fmix64(m) & 0x3FFFF == 0x3FFFF and not m & ~bf.SPACED for m in ms)
    assert len({lit.fmix64(m) >> 34 for m in ms}) == 12  # without a key the enumeration runs through the keys
    ms = bf.forge_minimizers(48, 15, n=3, low_ones=4)  # (gcd(16, 48) = 16 divides 15 - 15)
    assert all(lit.fmix64(m) % 48 == 15 and lit.fmix64(m) & 15 == 15 for m in ms)
    with pytest.raises(ValueError):
        bf.forge_minimizers(48, 14, low_ones=4)  # a hash that ends in four ones is 15 modulo 16
    with pytest.raises(ValueError):
        bf.forge_minimizers(CAP, 7, key=3, n=100000)  # more than the pair has: an error, not a shorter list
    with pytest.raises(AssertionError):
        bf.forge_minimizers(1 << 20, 7, key=3)


def test_unfillable_minimizer_is_refused():
    rng = np.random.default_rng(3)
    m = (3 << 60) | 3  # first base T, last base T: the reverse complement starts with A and is the smaller one
    assert bf.record_for(m, rng) is None
    with pytest.raises(ValueError):
        bf.forge(1, [(0, None)], rng, low_ones=63)  # two hashes, neither a legal minimizer's: an error, not an empty list


@pytest.fixture(scope="module")
def abc(forged):
    """A and B share a key at homes 10 and 11, C has another key at home 10: the six orders and their model tables"""
    a, b = forged[4], forged[6]
    (c,) = bf.forge(CAP, [(10, 0x54321)], np.random.default_rng(4))
    recs = {"A": a, "B": b, "C": c}
    tables = {}
    for order in itertools.permutations("ABC"):
        blob, size = u.model_hash([recs[x][1] for x in order], CAP)
        tables["".join(order)] = (u.cells_of(blob), size)
    return [m for m, _ in (a, b, c)], tables


def test_order_dependence(abc):
    """B adds a cell of its own unless it finds A's key on its path, and A unless it finds B's: A sits at 10 and is off B's path
    (which starts at 11) when A goes in before C; otherwise C holds 10, A moves to 11 or finds B there, and the two share a cell"""
    mins, tables = abc
    sizes = {o: s for o, (_, s) in tables.items()}
    assert sizes == {"ABC": 3, "ACB": 3, "BAC": 3, "CAB": 2, "BCA": 2, "CBA": 2}
    for o, ((hdr, cells), size) in tables.items():
        assert hdr[1] == size == int((cells != 0).sum())
    assert len(set(mins)) == 3  # what the counting pass reports, whatever the order


def test_valid_table_accepts(abc):
    mins, tables = abc
    for o, ((hdr, cells), _) in tables.items():
        bf.valid_table(hdr, cells, mins, CAP)
        assert bf.probe_lengths(cells, mins, CAP).max() == (3 if o in ("ABC", "BAC") else 2), o


def _spoiled(abc):
    mins, tables = abc
    (hdr, cells), _ = tables["ACB"]  # A at 10, C at 11, B at 12
    assert np.flatnonzero(cells).tolist() == [10, 11, 12] and cells[10] == cells[12]
    out = {}
    c = cells.copy()
    c[12] = 0  # B is lost
    out["zeroed"] = ((hdr[0], 2, 30, 2), c)
    out["zeroed, old header"] = (hdr, c)
    c = cells.copy()
    c[11] = (0x77777 << 2) | 2
    out["foreign key"] = (hdr, c)
    c = cells.copy()
    c[12], c[13] = 0, cells[12]
    out["behind an empty cell"] = (hdr, c)
    out["wrong size"] = ((hdr[0], 2, 30, 2), cells)
    out["wrong key bits"] = ((hdr[0], 3, 29, 3), cells)
    c = cells.copy()
    c[11] = (c[11] & ~np.uint32(3)) | np.uint32(1)
    out["value 1"] = (hdr, c)
    c = cells.copy()
    c[13] = cells[12]  # B's key twice on B's path: no insertion claims the second
    out["key twice"] = ((hdr[0], 4, 30, 2), c)
    (hdr2, cells2), _ = tables["CAB"]
    c = cells2.copy()
    c[12] = cells2[11]  # the same where A and B share cell 11
    out["key twice, shared"] = ((hdr2[0], 3, 30, 2), c)
    return mins, out


@pytest.mark.parametrize("what", ["zeroed", "zeroed, old header", "foreign key", "behind an empty cell", "wrong size", "wrong key bits",
                                  "value 1", "key twice", "key twice, shared"])
def test_valid_table_rejects(abc, what):
    mins, spoiled = _spoiled(abc)
    hdr, cells = spoiled[what]
    with pytest.raises(AssertionError):
        bf.valid_table(hdr, cells, mins, CAP)


def test_valid_table_rejects_a_missing_minimizer(abc):
    """a table of A and C alone is no table of A, B and C ... unless B's key is on B's path, which it is not"""
    mins, _ = abc
    (a,) = [m for m in mins if lit.fmix64(m) % CAP == 10 and lit.fmix64(m) >> 34 == 0x12345]
    blob = struct.pack("<4Q", CAP, 1, 30, 2) + struct.pack("<%dI" % CAP, *[((0x12345 << 2) | 2) if i == 10 else 0 for i in range(CAP)])
    hdr, cells = u.cells_of(blob)
    bf.valid_table(hdr, cells, [a], CAP)
    with pytest.raises(AssertionError, match="not found"):
        bf.valid_table(hdr, cells, mins, CAP)
    with pytest.raises(AssertionError, match="not found"):
        bf.probe_lengths(cells, mins, CAP)


def test_shared_key_records():
    """the input of the GPU tests does what it is for: forward and reversed give tables of different sizes, both valid, and
    the wrap group wraps"""
    recs, mins = bf.shared_key_records(CAP, np.random.default_rng(7))
    assert len(recs) == 40 and len(set(mins)) == 40
    seqs = [s for _, s in recs]
    assert u.minimizers(seqs)[0] == set(mins)
    fwd, size_f = u.model_hash(seqs, CAP)
    rev, size_r = u.model_hash(seqs[::-1], CAP)
    assert size_r < size_f < len(mins)
    for blob in (fwd, rev):
        hdr, cells = u.cells_of(blob)
        bf.valid_table(hdr, cells, mins, CAP)
    cells = u.cells_of(fwd)[1]
    assert cells[CAP - 2] and cells[CAP - 1] and cells[0] >> 2 == 0x33333333 and cells[1] >> 2 == 1  # W2 and Y, past the end
