"""A numpy model of nh_extend_db: a base hash.k2d + taxo.k2d, a manifest of additions and their sequences in,
the extended table and taxonomy out.  The steps are the library's: merge and renumber the tree, re-key every cell for the wider
value field, send its value through the renumbering, give the cells of one probe run that now share a key the LCA of their values
(shadowed cells), then insert the new (taxon, minimizer) pairs by linear probing with LCA.  CPU only: numpy, oracle/ and the test
helpers."""
from __future__ import annotations

import functools
import struct

import numpy as np

from oracle import k2_literal as lit
from oracle import minidb
from tests import build_db_util as u


def read_taxo(tb):
    """taxo.k2d -> (parent, external id, name, rank) lists by internal id"""
    assert tb[:8] == b"K2TAXDAT"
    n, name_len, rank_len = struct.unpack_from("<3Q", tb, 8)
    names = tb[32 + 56 * n:32 + 56 * n + name_len]
    ranks = tb[32 + 56 * n + name_len:32 + 56 * n + name_len + rank_len]
    parent, ext, name, rank = [], [], [], []
    for i in range(n):
        p, _, _, name_off, rank_off, e, _ = struct.unpack_from("<7Q", tb, 32 + 56 * i)
        parent.append(p)
        ext.append(e)
        name.append(names[name_off:names.index(b"\0", name_off)].decode())
        rank.append(ranks[rank_off:ranks.index(b"\0", rank_off)].decode())
    return parent, ext, name, rank


def merge(base_taxo, lines):
    """the base's tree with the manifest lines (taxid, parent taxid, name, ...) on top -> (minidb.Taxonomy of the merged tree with
    the names it keeps, remap: internal id of the base -> internal id of the merged tree).  A line whose taxid the base holds must
    name the base's parent and keeps the base's name."""
    parent, ext, name, _ = read_taxo(base_taxo)
    assert ext[1] == 1 and len(set(ext[1:])) == len(ext) - 1
    edges, names = {1: 0}, {1: name[1]}
    for i in range(2, len(ext)):
        edges[ext[i]] = ext[parent[i]]
        names[ext[i]] = name[i]
    for taxid, par, nm, *_ in lines:
        if taxid in edges:
            assert edges[taxid] == par, "taxid %d is in the base under %d, not %d" % (taxid, edges[taxid], par)
        else:
            edges[taxid] = par
            names[taxid] = nm
    for taxid, par in edges.items():
        assert par == 0 or par in edges, "the parent %d of %d is nowhere" % (par, taxid)
    tax = minidb.Taxonomy(edges, names)
    assert tax.node_count == len(edges) + 1, "a cycle"
    return tax, [0] + [tax.internal[e] for e in ext[1:]]


def runs_of(cells):
    """the probe runs (maximal cyclic stretches of non-empty cells) -> an int64 array with a run number per cell, -1 where empty"""
    occ = cells != 0
    run = np.cumsum(~occ).astype(np.int64)
    if occ[0] and occ[-1] and not occ.all():
        run[run == 0] = run[-1]  # the run that wraps round the table's end
    run[~occ] = -1
    return run


def rekey(cells, old_vb, new_vb, remap, tax):
    """every cell re-keyed and renumbered, then the shadow rule -> (cells, shadowed cells).  A cell is shadowed when a cell before
    it in its run has its key; every cell of such a group gets the LCA of the group's values."""
    remap = np.asarray(remap, dtype=np.uint32)
    occ = cells != 0
    values = cells & np.uint32((1 << old_vb) - 1)
    assert occ.sum() == 0 or (values[occ].min() >= 1 and values[occ].max() < len(remap)), "a value that is no node of the base"
    keys = (cells >> np.uint32(old_vb)) >> np.uint32(new_vb - old_vb)
    out = np.where(occ, (keys << np.uint32(new_vb)) | remap[np.minimum(values, len(remap) - 1)], np.uint32(0)).astype(np.uint32)
    shadowed = 0
    if new_vb > old_vb:
        run = runs_of(out)
        where = np.flatnonzero(occ)
        group = (run[where] << 32) | keys[where].astype(np.int64)
        _, inverse, counts = np.unique(group, return_inverse=True, return_counts=True)
        vmask = (1 << new_vb) - 1
        for g in np.flatnonzero(counts > 1):
            members = where[inverse == g]
            v = 0
            for p in members:
                v = tax.lca(v, int(out[p]) & vmask)
            out[members] = np.uint32((int(out[members[0]]) & ~vmask) | v)
            shadowed += len(members) - 1
    return out, shadowed


def insert(cells, vb, tax, pairs):
    """(internal id, minimizer) pairs into the table as minidb.build_hash inserts them (a cell is empty when it is 0, as the
    library has it) -> cells claimed"""
    cap = len(cells)
    vmask = (1 << vb) - 1
    claimed = 0
    for taxon, m in pairs:
        hc = lit.fmix64(int(m))
        key = hc >> (32 + vb)
        idx = hc % cap
        for _ in range(cap):
            c = int(cells[idx])
            if c == 0:
                cells[idx] = (key << vb) | taxon
                claimed += 1
                break
            if c >> vb == key:
                cells[idx] = (key << vb) | tax.lca(c & vmask, taxon)
                break
            idx = (idx + 1) % cap
        else:
            raise AssertionError("the table is full")
    return claimed


@functools.lru_cache(maxsize=None)
def _scanner():
    from oracle import oracle as orc
    from tests import synth
    ob, tb, hb, _, _ = synth.toy_db()  # (any database of the default geometry: only the scanner is used)
    return orc.OracleDB(ob, tb, hb)


def minimizer_pairs(tax, pairs):
    """(external taxid, sequence) pairs -> (internal id, minimizer) pairs, every distinct minimizer of a sequence once (the C
    oracle's scanner under the ambiguity rule in force, as build_db_util.fast_minimizers has it)"""
    odb = _scanner()
    odb.set(ambiguity_rule=u.rule())
    out = []
    for t, s in pairs:
        mins, amb = odb.scan(s)
        out += [(tax.internal[t], int(m)) for m in np.unique(mins[amb == 0])]
    return out


def extend(base_hash, base_taxo, lines, pairs=(), forged=()):
    """the whole extension.  pairs: (external taxid, sequence) of the addition; forged: (external taxid, minimizer), inserted behind
    them -> dict(hash: hash.k2d bytes, size, tax, remap, old_vb, new_vb, shadowed, cells_added, base_cells, cells: per-node
    counts before / after the insertion, by internal id of the merged tree)"""
    from tests import build_taxa_util as t
    (cap, size, kb, old_vb), cells = u.cells_of(base_hash)
    assert kb + old_vb == 32 and int((cells != 0).sum()) == size
    tax, remap = merge(base_taxo, lines)
    new_vb = max(old_vb, minidb.value_bits_for(tax.node_count))
    out, shadowed = rekey(cells, old_vb, new_vb, remap, tax)
    base_cells = t.value_counts(out, new_vb, tax.node_count)
    added = insert(out, new_vb, tax, minimizer_pairs(tax, pairs) + [(tax.internal[x], int(m)) for x, m in forged])
    blob = struct.pack("<4Q", cap, size + added, 32 - new_vb, new_vb) + out.astype("<u4").tobytes()
    return dict(hash=blob, size=size + added, tax=tax, remap=remap, old_vb=old_vb, new_vb=new_vb, shadowed=shadowed, cells_added=added,
                base_cells=base_cells, cells=t.value_counts(out, new_vb, tax.node_count))
