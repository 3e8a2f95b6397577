"""The cases that the tests of nh_extend_db share (model and GPU): a base and an addition, as manifest lines and records per taxon,
with the union that a build in one go would be given.  Made once a process and never changed."""
from __future__ import annotations

import functools
import math
import struct

import numpy as np

from oracle import k2_literal as lit
from oracle import minidb
from tests import build_db_util as u
from tests import build_forge as bf
from tests import build_taxa_util as t
from tests import extend_model as xm

BASE_LOAD = 0.4
BETWEEN_SEEDS = {10: 611, 20: 612, 30: 613, "more": 614}
WIDE_BASE_SEED = 621
SHADOW_CAP = 1021


def _case(base_lines, base_records, add_lines, add_records, cap=None):
    """union: every line once (the base's name where both have one), a taxon's records the base's then the addition's"""
    union_lines = list(base_lines) + [ln for ln in add_lines if ln[0] not in {b[0] for b in base_lines}]
    union_records = {k: list(v) for k, v in base_records.items()}
    for k, v in add_records.items():
        union_records[k] = union_records.get(k, []) + list(v)
    base_tax, union_tax = t.taxonomy_of(base_lines), t.taxonomy_of(union_lines)
    base_pairs, union_pairs = t.pairs_of(base_tax, base_records), t.pairs_of(union_tax, union_records)
    add_pairs = t.pairs_of(union_tax, add_records)
    base_mins = u.fast_minimizers([s for _, s in base_pairs])
    if cap is None:
        cap = int(math.ceil(len(base_mins) / BASE_LOAD))
    return dict(base_lines=tuple(base_lines), base_records=base_records, add_lines=tuple(add_lines), add_records=add_records,
                union_lines=tuple(union_lines), union_records=union_records, base_tax=base_tax, union_tax=union_tax,
                base_pairs=base_pairs, add_pairs=add_pairs, union_pairs=union_pairs, cap=cap)


@functools.lru_cache(maxsize=None)
def case(name, n_seq=8):
    """n_seq: records (2.5 kb each) of every base genome that is not the tree's; the splits of the tree have the tree's own capacity, so
    that their union is build_taxa_util.tree_case as it stands, every other base is at BASE_LOAD"""
    tc = t.tree_case()
    genome = lambda seed: u.genome(seed, n_seq=n_seq)  # noqa: E731
    added = lambda seed: u.genome(seed, n_seq=max(1, n_seq // 2))  # noqa: E731  (half a base genome: two of them fit a base at 0.4)
    rec = tc["records"]
    line = {ln[0]: ln for ln in t.TREE_LINES}
    if name == "leaf":  # a leaf under an inner node of the base
        return _case([line[t.G], line[t.A], line[t.C_]], {k: rec[k] for k in (t.G, t.A, t.C_)}, [line[t.B]], {t.B: rec[t.B]}, cap=tc["cap"])
    if name == "inner":  # an inner node with sequences of its own, and its leaves
        return _case([line[t.C_]], {t.C_: rec[t.C_]}, [line[t.G], line[t.A], line[t.B]], {k: rec[k] for k in (t.G, t.A, t.B)}, cap=tc["cap"])
    if name == "existing":  # sequences for a taxon the base has
        base = dict(rec)
        base[t.A] = rec[t.A][:4]
        return _case(list(t.TREE_LINES), base, [line[t.A]], {t.A: rec[t.A][4:]}, cap=tc["cap"])
    if name == "one":  # one taxon onto a base of one taxon: four nodes, the value field keeps its two bits
        return _case([(10, 1, "ten")], {10: genome(BETWEEN_SEEDS[10])}, [(30, 1, "thirty")], {30: added(BETWEEN_SEEDS[30])})
    if name == "two":  # two taxa added: five nodes, one bit more
        return _case([(10, 1, "ten")], {10: genome(BETWEEN_SEEDS[10])}, [(20, 1, "twenty"), (30, 1, "thirty")],
                     {20: added(BETWEEN_SEEDS[20]), 30: added(BETWEEN_SEEDS[30])})
    if name == "between":  # a sibling between two children of the base (30 moves from 3 to 4), and more sequences for 30
        return _case([(10, 1, "ten"), (30, 1, "thirty")], {10: genome(BETWEEN_SEEDS[10]), 30: genome(BETWEEN_SEEDS[30])},
                     [(20, 1, "twenty"), (30, 1, "thirty")], {20: added(BETWEEN_SEEDS[20]), 30: u.genome(BETWEEN_SEEDS["more"], n_seq=1)})
    w = t.wide_case(300)
    if name == "wide3":  # 300 leaves onto three nodes: two value bits become nine
        return _case([(5, 1, "five")], {5: u.genome(WIDE_BASE_SEED)}, list(w["lines"]), w["records"])
    if name == "tree_wide":  # the tree of the multi-taxon tests plus the 300 leaves: three value bits become nine
        return _case(list(t.TREE_LINES), rec, list(w["lines"]), w["records"])
    raise KeyError(name)


def taxo_bytes(tax):
    """the taxo.k2d that the library writes for the model's taxonomy (the sentinel shares the root's name)"""
    n = tax.node_count
    first, count = [0] * n, [0] * n
    for i in range(2, n):
        p = tax.parent[i]
        if count[p] == 0:
            first[p] = i
        count[p] += 1
    names, nodes = bytearray(b"root\0"), bytearray()
    for i in range(n):
        off = 0
        if i >= 2:
            off = len(names)
            names += tax.names[tax.external[i]].encode() + b"\0"
        nodes += struct.pack("<7Q", tax.parent[i], first[i], count[i], off, 0, tax.external[i] if i else 0, 0)
    return b"K2TAXDAT" + struct.pack("<3Q", n, len(names), 8) + bytes(nodes) + bytes(names) + b"no rank\0"


def base_hash(tax, pairs, cap, forged=()):
    """a base table made by the model's own inserter on an empty table (test_extend_model.py holds it to minidb.build_hash)"""
    vb = minidb.value_bits_for(tax.node_count)
    cells = np.zeros(cap, dtype=np.uint32)
    size = xm.insert(cells, vb, tax, xm.minimizer_pairs(tax, pairs) + [(tax.internal[x], int(m)) for x, m in forged])
    return struct.pack("<4Q", cap, size, 32 - vb, vb) + cells.astype("<u4").tobytes()


def write_base(d, tax, hash_bytes, opts=None):
    minidb.write_db(str(d), minidb.opts_bytes() if opts is None else opts, taxo_bytes(tax), hash_bytes)
    return str(d)


def colliding_keys_apart(mins, cap, vb, cells):
    """the condition under which a table does not depend on the order of insertion, and an extension has no shadowed cell: two
    minimizers with one compacted key at `vb` value bits have homes further apart than the longest run of the table"""
    hc = u.fmix64_np(np.asarray(mins, dtype=np.uint64))
    ck = hc >> np.uint64(32 + vb)
    home = (hc % np.uint64(cap)).astype(np.int64)
    order = np.argsort(ck, kind="stable")
    ck, home = ck[order], home[order]
    apart = u.longest_run(cells) + 1
    for i in np.nonzero(ck[1:] == ck[:-1])[0]:
        d = abs(int(home[i + 1]) - int(home[i]))
        assert min(d, cap - d) > apart, "two minimizers share a key at %d value bits and lie in reach of each other: choose another seed" % vb


X_ID, Y_ID, Z_ID = 7, 8, 9


@functools.lru_cache(maxsize=None)
def shadow_case():
    """X and Y under the root (two value bits).  m1 with the key 2K under X and m2 with 2K + 1 under Y, both at home capacity - 1,
    so that m2 lies in cell 0 and their run wraps; m3 with a key of its own between them in neither's way (home 1); fillers with
    keys of their own.  One taxon more (Z) makes three value bits, and both cells hold the key K.  m4: a third minimizer of the key
    K (2K again, at the value bits of the forge) and the same home, for Z."""
    cap = SHADOW_CAP
    rng = np.random.default_rng(77)
    K = 0x0ABCDEF1
    made = bf.forge(cap, [(cap - 1, 2 * K), (cap - 1, 2 * K + 1), (cap - 1, 2 * K)], rng)
    (m1, r1), (m2, r2), (m4, r4) = made
    fill = bf.forge(cap, [(h, None) for h in (1, 1, 200, 201, 500, cap - 3)], rng, distinct_keys=True, exclude=(m1, m2, m4))
    assert all((lit.fmix64(m) >> 35) != K for m, _ in fill)
    lines = ((X_ID, 1, "taxon X"), (Y_ID, 1, "taxon Y"))
    tax = t.taxonomy_of(lines)
    owners = [X_ID, Y_ID, X_ID, Y_ID, X_ID, Y_ID]
    records = {X_ID: [(b"m1", r1)] + [(b"fx%d" % i, r) for i, ((_, r), o) in enumerate(zip(fill, owners)) if o == X_ID],
               Y_ID: [(b"m2", r2)] + [(b"fy%d" % i, r) for i, ((_, r), o) in enumerate(zip(fill, owners)) if o == Y_ID]}
    forged = [(X_ID, m1), (Y_ID, m2)] + [(o, m) for (m, _), o in zip(fill, owners)]
    return dict(cap=cap, K=K, lines=lines, tax=tax, records=records, forged=forged, m1=m1, m2=m2, m4=m4, r2=r2, r4=r4,
                z_line=(Z_ID, 1, "taxon Z"), z_filler=bf.forge(cap, [(700, None)], rng, distinct_keys=True, exclude=(m1, m2, m4))[0])
