"""Model of the minimizer data (nh_run_mdata, nohuman_amd/csrc/nh_mdata.hip; include/nohuman_engine.h has the definitions): on
oracle/k2_literal.py, the loop of classify_fragment once more, recording for every hit group the taxon found and the CELL where the
key matched.  Pure Python, CPU only.

A hit group: a run start (a minimizer that differs from the fragment's previous non-ambiguous one; the previous one survives
ambiguous k-mers and is reset at mate 2 exactly when db.reset_per_mate is set) whose look-up finds a cell with a non-zero value.
Per node t:  minimizers_own[t] hit groups with value t;  distinct_own[t] distinct cells among them;  db_cells_own[t] cells of the
table with value t;  *_clade the sums over the subtree (db.parent);  reads_* as the report has them."""
from __future__ import annotations

import struct

import numpy as np

from oracle import k2_literal as lit

HEADER = "taxid\tname\treads_clade\treads_own\tminimizers_clade\tminimizers_own\tdistinct_clade\tdistinct_own\tdb_cells_clade\t" \
         "db_cells_own\tcoverage_pct\n"
FIELDS = ("reads_clade", "reads_own", "minimizers_clade", "minimizers_own", "distinct_clade", "distinct_own", "db_cells_clade",
          "db_cells_own")


def find(db: lit.DB, minimizer: int):
    """compact_hash.cc Get with the place: (value, index of the cell where the key matched), (0, -1) for a miss"""
    assert db.linear_probing
    hc = lit.fmix64(minimizer)
    vmask = (1 << db.value_bits) - 1
    compacted = hc >> (32 + db.value_bits)
    idx = first = hc % db.capacity
    while True:
        cell = db.cells[idx]
        if cell & vmask == 0:
            return 0, -1
        if cell >> db.value_bits == compacted:
            return cell & vmask, idx
        idx = (idx + 1) % db.capacity
        if idx == first:
            return 0, -1


def hit_groups(db: lit.DB, mates, scanner=None, found=None):
    """the hit groups of one fragment, in order: [(taxon, cell)].  scanner: what gives a sequence's (ambiguous, minimizer) per k-mer
    in place of lit.kmer_minimizers (c_scanner below, for inputs of thousands of reads); found: a dict that keeps the look-ups"""
    assert not db.min_hash
    out = []
    last_min = None
    for seq in mates:
        if db.reset_per_mate:
            last_min = None
        for ambiguous, minimizer in (scanner(seq) if scanner else lit.kmer_minimizers(db, seq)):
            if ambiguous or minimizer == last_min:
                continue
            last_min = minimizer
            if found is None:
                taxon, cell = find(db, minimizer)
            else:
                if minimizer not in found:
                    found[minimizer] = find(db, minimizer)
                taxon, cell = found[minimizer]
            if taxon:
                out.append((taxon, cell))
    return out


def c_scanner(odb):
    """the scanner of the C oracle (oracle.OracleDB.scan) in the form hit_groups takes: the same k-mers, a hundred times faster;
    tests/test_mdata_model.py holds it to lit.kmer_minimizers.  The ambiguity rule is odb's."""
    def scanner(seq):
        mins, amb = odb.scan(seq)
        return zip(amb.tolist(), mins.tolist())
    return scanner


def scan(db: lit.DB, fragments, scanner=None):
    """fragments: tuples of mates (bytes).  -> (hit groups per node, the set of marked cells, hit groups per fragment)"""
    n = len(db.parent)
    groups = np.zeros(n, dtype=np.uint64)
    marked = set()
    per_fragment = []
    found = {}
    for mates in fragments:
        hg = hit_groups(db, mates, scanner, found)
        per_fragment.append(len(hg))
        for taxon, cell in hg:
            groups[taxon] += np.uint64(1)
            marked.add(cell)
    return groups, marked, per_fragment


def bitmap(db: lit.DB, marked) -> np.ndarray:
    """the bitmap k_mdata_mark leaves: bit c & 31 of word c >> 5, ceil(capacity / 32) words"""
    words = np.zeros((db.capacity + 31) // 32, dtype=np.uint32)
    for c in marked:
        words[c >> 5] |= np.uint32(1 << (c & 31))
    return words


def cells_by_value(db: lit.DB, only=None) -> np.ndarray:
    """cells of the table per value (`only`: among these cells), by internal id"""
    vmask = (1 << db.value_bits) - 1
    out = np.zeros(len(db.parent), dtype=np.uint64)
    for c in (range(db.capacity) if only is None else only):
        v = db.cells[c] & vmask
        if v:
            out[v] += np.uint64(1)
    return out


def clade(db: lit.DB, own) -> np.ndarray:
    out = np.array(own, dtype=np.uint64)
    for i in range(len(db.parent) - 1, 1, -1):  # children have larger ids than their parents
        out[db.parent[i]] += out[i]
    return out


def numbers(db: lit.DB, fragments, calls, scanner=None):
    """the eight columns of a run as a dict of arrays by internal id; calls: the internal taxon of every fragment's call"""
    groups, marked, per_fragment = scan(db, fragments, scanner)
    reads = np.zeros(len(db.parent), dtype=np.uint64)
    for c in calls:
        if c:
            reads[c] += np.uint64(1)
    own = {"reads": reads, "minimizers": groups, "distinct": cells_by_value(db, marked), "db_cells": cells_by_value(db)}
    out = {}
    for q, a in own.items():
        out[q + "_own"] = a
        out[q + "_clade"] = clade(db, a)
    out["per_fragment"] = per_fragment
    out["marked"] = marked
    return out


def names_of(taxo: bytes):
    """taxo.k2d -> the nodes' names, by internal id"""
    n, name_len, _ = struct.unpack_from("<3Q", taxo, 8)
    blob = taxo[32 + 56 * n:32 + 56 * n + name_len]
    out = []
    for i in range(n):
        off = struct.unpack_from("<Q", taxo, 32 + 56 * i + 24)[0]
        out.append(blob[off:blob.index(b"\0", off)].decode())
    return out


def table(db: lit.DB, names, num) -> str:
    rows = [HEADER]
    for i in range(1, len(db.parent)):
        if not num["reads_clade"][i] and not num["minimizers_clade"][i]:
            continue
        cov = "%.4f" % (100.0 * int(num["distinct_clade"][i]) / int(num["db_cells_clade"][i])) if num["db_cells_clade"][i] else "NA"
        rows.append("\t".join([str(db.external[i]), names[i]] + [str(int(num[f][i])) for f in FIELDS] + [cov]) + "\n")
    return "".join(rows)


def taxa_list(db: lit.DB, num):
    """what run(minimizer_data=[]) receives: a dict per node from the root on"""
    return [dict([("taxid", db.external[i])] + [(f, int(num[f][i])) for f in FIELDS]) for i in range(1, len(db.parent))]


def report(db: lit.DB, names, num, total, minimizer_data=True) -> str:
    """the report of a database whose every rank is "no rank" (every database the tests build): with minimizer_data the 8-column
    form -- pct, reads_clade, reads_own, minimizers_clade, distinct_clade, rank, taxid, name"""
    n = len(db.parent)
    reads_clade, reads_own = num["reads_clade"], num["reads_own"]
    kids = {i: [j for j in range(2, n) if db.parent[j] == i] for i in range(n)}
    uncl = total - int(reads_clade[1]) if n > 1 else total
    lines = []
    if uncl:
        lines.append("%6.2f\t%d\t%d\t%sU\t0\tunclassified\n" % (100.0 * uncl / total, uncl, uncl, "0\t0\t" if minimizer_data else ""))

    def dfs(i, depth):
        if not reads_clade[i]:
            return
        extra = "%d\t%d\t" % (num["minimizers_clade"][i], num["distinct_clade"][i]) if minimizer_data else ""
        lines.append("%6.2f\t%d\t%d\t%s%s\t%d\t%s%s\n" % (100.0 * int(reads_clade[i]) / total, reads_clade[i], reads_own[i], extra,
                                                         "R" + (str(depth) if depth else ""), db.external[i], "  " * depth, names[i]))
        for j in sorted(kids[i], key=lambda j: -int(reads_clade[j])):
            dfs(j, depth + 1)

    if n > 1 and total:
        dfs(1, 0)
    return "".join(lines)


def drop_minimizer_columns(text: str) -> str:
    """an 8-column report without its columns 4 and 5"""
    out = []
    for line in text.splitlines(keepends=True):
        f = line.split("\t")
        out.append("\t".join(f[:3] + f[5:]))
    return "".join(out)
