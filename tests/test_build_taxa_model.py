"""The inputs of tests/test_gpu_build_db_taxa.py under the Python model (oracle/minidb.py), on the CPU: each is order free -- the
model gives the same occupied positions and sorted cells with the (taxon, record) pairs forward, reversed and interleaved, and no
two distinct minimizers share a compacted key at the database's key_bits -- so the GPU's table, whatever order its waves arrive
in, is compared with the model's as it is and nothing is left out.  The seeds in build_taxa_util.py were chosen for that.  And the
library's internal ids of a manifest are minidb.Taxonomy's."""
import numpy as np
import pytest

from oracle import minidb
from tests import build_db_util as u
from tests import build_taxa_util as t


@pytest.mark.parametrize("case", ["tree", "border", "wide"])
def test_the_inputs_are_order_free(case):
    c = {"tree": t.tree_case, "border": t.border_case, "wide": t.wide_case}[case]()
    blob, size = t.assert_order_free(c["tax"], c["pairs"], c["cap"], forward=(c["model"], c["size"]))
    assert blob == c["model"] and size == c["size"] == len(c["mins"])
    vb = minidb.value_bits_for(c["tax"].node_count)
    assert vb == {"tree": 3, "border": 3, "wide": 9}[case]
    counts = t.value_counts(u.cells_of(blob)[1], vb, c["tax"].node_count)
    assert counts[0] == 0 and sum(counts) == size
    if case == "wide":
        assert c["tax"].node_count == 302 and counts[1] > 0 and min(counts[2:]) > 0
    else:
        # every node holds cells: the leaves their own, G what A and B (or A and G) share, the root what C shares with them
        assert min(counts[1:]) > 0, counts


def test_the_tree_case_reaches_every_merge():
    c = t.tree_case()
    tax, st = c["tax"], c["stretches"]
    per = {tx: u.fast_minimizers([s for x, s in c["pairs"] if x == tx]) for tx in (t.A, t.B, t.C_, t.G)}
    ab, abc, ag = (u.fast_minimizers([st[k]]) for k in ("ab", "abc", "ag"))
    assert np.isin(ab, per[t.A]).all() and np.isin(ab, per[t.B]).all() and not np.isin(ab, per[t.C_]).any()
    assert all(np.isin(abc, per[x]).all() for x in (t.A, t.B, t.C_)) and np.isin(ag, per[t.A]).all() and np.isin(ag, per[t.G]).all()
    cells = u.cells_of(c["model"])[1]
    counts = t.value_counts(cells, 3, 6)
    # (the root holds what A, B and C share; G its own sequences and what A shares with B or with G)
    assert len(abc) <= counts[1] < len(abc) + 200
    assert len(ab) + len(ag) <= counts[tax.internal[t.G]] <= len(per[t.G]) + len(ab)
    assert [tax.lca(tax.internal[a], tax.internal[b]) for a, b in ((t.A, t.B), (t.A, t.G), (t.A, t.C_), (t.G, t.C_))] == [3, 3, 1, 1]


def test_the_race_genome_has_distinct_keys():
    seqs = [s for _, s in t.race_records()]
    mins = u.fast_minimizers(seqs)
    assert len(np.unique(u.fmix64_np(mins) >> np.uint64(35))) == len(mins) > 6000


def test_internal_ids_are_the_models(tmp_path):
    """nh_build_check gives the taxids in internal-id order: 0 the sentinel (not listed), 1 the root, then breadth first with the
    children of a node in ascending external id -- minidb.Taxonomy's order, whatever the order of the manifest's lines"""
    (tmp_path / "a.fa").write_bytes(b">s\nACGT\n")
    rng = np.random.default_rng(3)
    cases = [list(t.TREE_LINES), list(t.wide_case()["lines"])]
    # a random tree of 60 nodes with ids that do not sort like their depth
    ids = [int(x) for x in rng.choice(np.arange(2, 100000), size=60, replace=False)]
    cases.append([(x, 1 if i == 0 else ids[int(rng.integers(0, i))], "n%d" % x) for i, x in enumerate(ids)])
    for lines in cases:
        tax = t.taxonomy_of(lines)
        for order in (lines, lines[::-1], [lines[i] for i in rng.permutation(len(lines))]):
            rows = [tuple(ln) + (("a.fa",) if i == 0 else ()) for i, ln in enumerate(order)]
            m = t.write_manifest(tmp_path / "taxa.tsv", rows)
            rc, msg, st, per = t.raw_call("nh_build_check", m, str(tmp_path / "db"))
            assert rc == 0, msg
            assert st.taxa == tax.node_count - 1
            assert [per[i].taxid for i in range(st.taxa)] == tax.external[1:]
