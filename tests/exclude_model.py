"""The specification of a build with an exclusion list (nh_build_db_exclude), in pure Python on oracle/k2_literal.py and
tests/build_db_util.py.

H is the set of minimizers of the non-ambiguous k-mers of the host sequences (of the sequences as tests/dust_model.py masks
them where the build masks), X the same set of the exclusion sequences, which are never masked; both under the ambiguity rule in
force, exactly as build_db_util.minimizers computes them.  The database is the one a build makes of a host whose minimizer set is
H \\ X: the host is scanned as ever and a minimizer in X is passed over, whichever taxon's sequence it came from.

Exclusion works on the 62-bit minimizers, the table keeps compacted keys: an excluded minimizer is still "found" where a kept
minimizer with its key lies on its probe path.  shared_keys and still_found count that for a given input."""
from __future__ import annotations

import struct

import numpy as np

from oracle import k2_literal as lit
from oracle import minidb
from tests import build_db_util as u
from tests import build_forge as bf
from tests import synth


def sets(host_seqs, exclude_seqs, mask=False):
    """(H, X, k-mers of the host, its ambiguous k-mers, k-mers of the exclusion input, its ambiguous k-mers)"""
    if mask:
        from tests import dust_model as dm
        host_seqs = [dm.mask(s) for s in host_seqs]
    H, kmers, amb = u.minimizers(host_seqs)
    X, x_kmers, x_amb = u.minimizers(exclude_seqs)
    return H, X, kmers, amb, x_kmers, x_amb


def run_starts(seqs) -> int:
    """look-ups of the exclusion pass: a non-ambiguous k-mer whose minimizer is not that of the k-mer before it in its sequence
    (an ambiguous k-mer ends a run), as the classifier counts table look-ups"""
    db, n = u._shim(), 0
    for s in seqs:
        last = None
        for a, m in lit.kmer_minimizers(db, s):
            if a:
                last = None
            elif m != last:
                n += 1
                last = m
    return n


def build_hash(tax, pairs, X, capacity):
    """oracle/minidb.py build_hash of (external taxid, sequence) pairs with every minimizer in X passed over -> (hash.k2d
    bytes, size).  A minimizer two taxa share becomes their lowest common ancestor, as there."""
    vb = minidb.value_bits_for(tax.node_count)
    vmask = (1 << vb) - 1
    cells, size = [0] * capacity, 0
    shim = lit.DB(minidb.DEFAULT_K, minidb.DEFAULT_L, minidb.default_spaced_mask(), minidb.DEFAULT_TOGGLE, 1, 0, 1, capacity, 0,
                  32 - vb, vb, cells, tax.parent, tax.external, ambiguity_rule=u.rule())
    for ext, seq in pairs:
        taxon = tax.internal[ext]
        for ambiguous, m in lit.kmer_minimizers(shim, seq):
            if ambiguous or m in X:
                continue
            hc = lit.fmix64(m)
            key, idx = hc >> (32 + vb), hc % capacity
            for _ in range(capacity):
                cell = cells[idx]
                if cell & vmask == 0:
                    cells[idx] = key << vb | taxon
                    size += 1
                    break
                if cell >> vb == key:
                    cells[idx] = key << vb | tax.lca(cell & vmask, taxon)
                    break
                idx = (idx + 1) % capacity
            else:
                raise AssertionError("the model's table of %d cells is full" % capacity)
    return struct.pack("<4Q", capacity, size, 32 - vb, vb) + struct.pack("<%dI" % capacity, *cells), size


def model(host_seqs, exclude_seqs, load_factor=0.7, capacity=0, mask=False, taxid=9606):
    """a one-taxon build with an exclusion list -> dict: H, X, kept (H \\ X), excluded (H & X), capacity, the table (hash.k2d
    bytes) and its size, and the totals of both inputs as the library reports them"""
    H, X, kmers, amb, x_kmers, x_amb = sets(host_seqs, exclude_seqs, mask)
    kept, excluded = H - X, H & X
    cap = capacity or u.default_capacity(len(kept), load_factor)
    if mask:
        from tests import dust_model as dm
        host_seqs = [dm.mask(s) for s in host_seqs]
    blob, size = (None, 0) if not kept else build_hash(u.taxonomy(taxid), [(taxid, s) for s in host_seqs], X, cap)
    return dict(H=H, X=X, kept=kept, excluded=excluded, capacity=cap, table=blob, size=size, kmers=kmers, ambiguous=amb,
                x_kmers=x_kmers, x_ambiguous=x_amb, x_sequences=len(exclude_seqs), x_bases=sum(len(s) for s in exclude_seqs),
                x_lookups=run_starts(exclude_seqs))


def _scan(seqs):
    """(distinct minimizers of the non-ambiguous k-mers, k-mers, ambiguous k-mers, run starts) by the C oracle's scanner"""
    from oracle import oracle as orc
    ob, tb, hb, _, _ = synth.toy_db()  # (any database of the default geometry: only the scanner is used)
    odb = orc.OracleDB(ob, tb, hb)
    odb.set(ambiguity_rule=u.rule())
    parts, kmers, amb_n, runs = [], 0, 0, 0
    for s in seqs:
        mins, amb = odb.scan(s)
        if mins.size == 0:
            continue
        ok = amb == 0
        kmers += mins.size
        amb_n += int((~ok).sum())
        prev_ok = np.concatenate([[False], ok[:-1]])
        prev_same = np.concatenate([[False], mins[1:] == mins[:-1]])
        runs += int((ok & ~(prev_ok & prev_same)).sum())
        parts.append(mins[ok])
    return set(np.unique(np.concatenate(parts)).tolist()) if parts else set(), kmers, amb_n, runs


def model_fast(host_seqs, exclude_seqs, load_factor=0.7, capacity=0):
    """model() for inputs too long for pure Python, without masking: the sets by the C oracle's scanner (oracle/k2_oracle.c),
    the table by inserting the kept minimizers in ascending order -- any order gives the same occupied positions and sorted
    cells while no two of them share a compacted key, which is asserted.  tests/test_exclude_model.py holds it to model()."""
    H, kmers, amb, _ = _scan(host_seqs)
    X, x_kmers, x_amb, x_runs = _scan(exclude_seqs)
    kept, excluded = H - X, H & X
    cap = capacity or u.default_capacity(len(kept), load_factor)
    assert len({lit.fmix64(m) >> bf.KEY_SHIFT for m in kept}) == len(kept), "two kept minimizers share a compacted key: choose another seed"
    cells = [0] * cap
    for m in sorted(kept):
        hc = lit.fmix64(m)
        idx = hc % cap
        while cells[idx]:
            idx = (idx + 1) % cap
        cells[idx] = hc >> bf.KEY_SHIFT << u.VALUE_BITS | 2
    blob = struct.pack("<4Q", cap, len(kept), 32 - u.VALUE_BITS, u.VALUE_BITS) + struct.pack("<%dI" % cap, *cells)
    return dict(H=H, X=X, kept=kept, excluded=excluded, capacity=cap, table=blob if kept else None, size=len(kept), kmers=kmers,
                ambiguous=amb, x_kmers=x_kmers, x_ambiguous=x_amb, x_sequences=len(exclude_seqs),
                x_bases=sum(len(s) for s in exclude_seqs), x_lookups=x_runs)


def build_hash_fast(tax, pairs, X, capacity):
    """build_hash for inputs too long for pure Python: every taxon's minimizers by the C oracle's scanner, a minimizer's value the
    lowest common ancestor of the taxa that carry it, the kept ones inserted in ascending order -- the occupied positions and
    sorted cells of any order while no two of them share a compacted key, which is asserted -> (hash.k2d bytes, size)"""
    vb = minidb.value_bits_for(tax.node_count)
    value = {}
    for ext in dict.fromkeys(t for t, _ in pairs):
        node = tax.internal[ext]
        for m in _scan([s for t, s in pairs if t == ext])[0]:
            value[m] = tax.lca(value[m], node) if m in value else node
    kept = sorted(m for m in value if m not in X)
    assert len({lit.fmix64(m) >> (32 + vb) for m in kept}) == len(kept), "two kept minimizers share a compacted key: choose another seed"
    cells = [0] * capacity
    for m in kept:
        hc = lit.fmix64(m)
        idx = hc % capacity
        while cells[idx]:
            idx = (idx + 1) % capacity
        cells[idx] = hc >> (32 + vb) << vb | value[m]
    return struct.pack("<4Q", capacity, len(kept), 32 - vb, vb) + struct.pack("<%dI" % capacity, *cells), len(kept)


def order_free(m):
    """the condition under which same_table is the whole truth about the model's table: no two KEPT minimizers share a compacted
    key (build_db_util.order_free's condition, on H \\ X) -> the model"""
    keys = {lit.fmix64(x) >> bf.KEY_SHIFT for x in m["kept"]}
    assert len(keys) == len(m["kept"]) == m["size"], "two kept minimizers share a compacted key: choose another seed"
    return m


def shared_keys(kept, excluded, value_bits=u.VALUE_BITS):
    """the excluded minimizers whose compacted key a kept minimizer has too: the only ones a table of the kept set can still
    answer for, and it does where the kept one lies on the excluded one's probe path -> sorted list"""
    keys = {lit.fmix64(m) >> (32 + value_bits) for m in kept}
    return sorted(m for m in excluded if lit.fmix64(m) >> (32 + value_bits) in keys)


def still_found(cells, excluded, capacity):
    """the excluded minimizers that a look-up in this table finds all the same (a cell with their key before any empty cell on
    their probe path) -> sorted list.  Every one of them is in shared_keys for the set the table was built from."""
    if not excluded:
        return []
    ms, _, _, length = bf._walk(cells, excluded, capacity)
    return [int(m) for m in ms[np.flatnonzero(length)]]


def brute_minimizers(seq: bytes, rule=None):
    """the definition read k-mer by k-mer, for tiny inputs: the set of minimizers of the non-ambiguous k-mers of one sequence.
    A k-mer is ambiguous when a byte that is no base lies in its last 31 bases (rule 0) or its last 34 (rule 1); otherwise its
    minimizer is the least candidate among its l-mers that hold no such byte -- all five of them unless the byte is among the
    k-mer's first bases -- a candidate being the canonical l-mer under the spaced mask, compared after the toggle.  No sliding
    window and no bookkeeping across k-mers: independent of k2_literal.kmer_minimizers in everything but reverse_complement."""
    L, K = minidb.DEFAULT_L, minidb.DEFAULT_K
    span = L if (u.rule() if rule is None else rule) == 0 else K - 1
    spaced, toggle = minidb.default_spaced_mask(), minidb.DEFAULT_TOGGLE & ((1 << 2 * L) - 1)
    code = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
    out = set()
    for i in range(len(seq) - K + 1):
        kmer = seq[i:i + K]
        if any(b not in code for b in kmer[K - span:]):
            continue
        best = None
        for j in range(K - L + 1):
            lmer = kmer[j:j + L]
            if any(b not in code for b in lmer):
                continue
            x = 0
            for b in lmer:
                x = x << 2 | code[b]
            c = (min(x, lit.reverse_complement(x, L)) & spaced) ^ toggle
            best = c if best is None or c < best else best
        out.add(best ^ toggle)
    return out
