"""Engine.add_sequences (nh_synthetic_add_sequences, k_insert_sequences) at its borders, against the Python minimizer model the
build-db tests use (tests/build_db_util.py minimizers): sequences packed back to back, so that their starts fall on every
alignment mod 4; lengths around the first k-mer (34 / 35) and around one, two tiles of 124 k-mers (158 / 159, 282 / 283) and
one of many tiles; an N, lower case; and the last sequence ending where the bases the call is given end (the 8 readable bytes
behind them hold letters that are no part of any sequence).

Which key sits in which cell of a probe run depends on the order in which the waves arrive, so the table is held to what no
order changes: every model minimizer is found with the value by a linear probe from its home before any empty cell, every
occupied cell holds the key of a model minimizer, and the occupied cells are as many as the call counted."""
import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import build_db_util as u
from tests import synth

pytestmark = pytest.mark.gpu
CAPACITY = 30011
VALUE = 30
LENGTHS = (34, 35, 158, 159, 282, 283, 5003, 301, 202, 161)  # [7] gets an N in its middle, [8] is lower case


def sequences():
    rng = np.random.default_rng(20)
    seqs = [bytearray(synth.random_seq(rng, n)) for n in LENGTHS]
    seqs[7][150] = ord("N")
    seqs[8] = bytearray(bytes(seqs[8]).lower())
    return [bytes(s) for s in seqs]


def probe(cells, vbits, mz):
    """the value under minimizer mz by a linear probe from its home, None where an empty cell (or every cell) comes first"""
    hc = lit.fmix64(mz)
    key, idx = hc >> (32 + vbits), hc % cells.size
    for _ in range(cells.size):
        c = int(cells[idx])
        if c == 0:
            return None
        if c >> vbits == key:
            return c & ((1 << vbits) - 1)
        idx = (idx + 1) % cells.size
    return None


def test_borders():
    import torch
    from nohuman_amd import Engine
    seqs = sequences()
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    assert set(int(o) % 4 for o in offs[:-1]) == {0, 1, 2, 3}
    mins, kmers, amb = u.minimizers(seqs)
    assert kmers == sum(max(0, n - 34) for n in LENGTHS) and 30 <= amb <= 40 and len(mins) > 1000  # (the N's k-mers)
    text = b"".join(seqs) + b"ACGTACGT"  # readable for 8 bytes behind the last base, as the entry asks; no sequence holds them
    d_bases = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    d_offs = torch.from_numpy(offs).to("cuda:0")
    with Engine.synthetic(CAPACITY, 0, depth=30, seed=1) as eng:
        assert eng.ambiguity_rule() == u.rule() and eng.options().linear_probing == 1
        vbits = int(eng.info.value_bits)
        assert eng.info.size == 0 and eng.info.capacity == CAPACITY
        eng.add_sequences(d_bases.data_ptr(), d_offs.data_ptr(), len(seqs), VALUE)
        cells = eng.download_table()
        counted = int(eng.info.size)
        # once more: every key is there already
        eng.add_sequences(d_bases.data_ptr(), d_offs.data_ptr(), len(seqs), VALUE)
        assert int(eng.info.size) == counted and np.array_equal(eng.download_table(), cells)
    missing = [m for m in sorted(mins) if probe(cells, vbits, m) != VALUE]
    assert not missing, "%d of %d model minimizers are not found with value %d, the first %#x" % (len(missing), len(mins), VALUE, missing[0])
    keys = {lit.fmix64(m) >> (32 + vbits) for m in mins}
    occupied = cells[cells != 0]
    strangers = set(int(c) >> vbits for c in occupied) - keys
    assert not strangers, "%d occupied cells hold keys of no model minimizer" % len(strangers)
    assert (occupied & ((1 << vbits) - 1) == VALUE).all()
    assert occupied.size == counted
    assert len(keys) <= occupied.size <= len(mins)  # (minimizers that share a compacted key may share a cell)
