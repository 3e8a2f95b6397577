"""nh_build_db with a taxa manifest on trees that are deep, wide or at the top of the range (tests/taxo_forge.py): the parent walk and
the compare-and-swap loop of the LCA merge (k_build_pieces<false, true>) on a chain of 60, up to 32 taxa meeting in one cell,
external ids that say nothing about the tree, and 4094 against 4095 taxa.  Every table is compared with the Python model's
(minidb.build_hash), as in test_gpu_build_db_taxa.py, and every occupied cell with lca_by_sets of the taxa whose sequences hold
its minimizer, which compares no ids.  tests/test_taxo_forge.py asserts on the CPU what the inputs promise."""
import numpy as np
import pytest

from oracle import minidb
from oracle import oracle as orc
from tests import build_db_util as u
from tests import build_taxa_util as t
from tests import taxo_forge as tf
from tests.test_gpu_build_db_taxa import assert_is_the_model, build

pytestmark = pytest.mark.gpu


def built(tmp, c, **kw):
    """the case built into tmp / db and held to the model and to lca_by_sets -> (stats, cells)"""
    m = t.write_case(tmp, c["lines"], c["records"])
    st = build(m, tmp / "db", **kw)
    assert_is_the_model(st, tmp / "db", c)
    cells = u.read_db(str(tmp / "db"))[1]
    tf.assert_cells_are_the_lcas(cells, c)
    return st, cells


@pytest.mark.parametrize("kw", [dict(), dict(batch=997, piece_kmers=64)], ids=["default", "batch997_piece64"])
def test_deep_tree(tmp_path, kw):
    """caterpillar(60): walks of up to 60 parents; stretches shared by two leaves, by a leaf and its ancestor, by a leaf and a
    chain node below its own, by three taxa"""
    c = tf.deep_case()
    st, cells = built(tmp_path, c, **kw)
    assert u.read_db(str(tmp_path / "db"))[0][2:] == (25, 7)
    counts = t.value_counts(cells, 7, 122)
    assert counts[c["tax"].internal[tf.C(1)]] > 0 and sum(1 for x in counts if x) >= 90


def test_many_way_races(tmp_path):
    """caterpillar(16): 40 records of 125 bases, each under 2 to 32 taxa, in pieces of 64 k-mers and one batch: more than a
    thousand waves, up to 32 of them at one cell.  Every cell of record j ends at lca_by_sets(S_j)"""
    c = tf.race_case()
    st, cells = built(tmp_path, c, piece_kmers=64)
    tax = c["tax"]
    by_key = {int(k): int(v) for k, v in zip(cells[cells != 0] >> np.uint32(6), cells[cells != 0] & np.uint32(63))}
    assert len(by_key) == st["size"]
    for j, mins in enumerate(c["by_record"]):
        want = tax.internal[tf.lca_by_sets(c["parent"], c["subsets"][j])]
        keys = u.fmix64_np(np.array(sorted(mins), dtype=np.uint64)) >> np.uint64(32 + 6)
        assert {by_key[int(k)] for k in keys} == {want}, j


def test_shuffled_external_ids(tmp_path):
    """random_tree(1000): a child's external id may be smaller than its parent's; the internal ids follow the BFS rule alone"""
    c = tf.shuffled_case()
    built(tmp_path, c)
    hdr, _, _, tb = u.read_db(str(tmp_path / "db"))
    assert hdr[2:] == (22, 10) and t.parse_taxo(tb) == t.model_nodes(c["tax"])


@pytest.mark.parametrize("n,bits", [(4094, (20, 12)), (4095, (19, 13))])
def test_top_of_the_range(tmp_path, n, bits):
    """heap(4094) and heap(4095): value_bits 12 against 13, the parent table of 2^value_bits entries, the last bin of
    k_value_cells, a walk of 11 parents from the largest id; then the database opened and the last taxon's reads classified"""
    from nohuman_amd import Engine
    c = tf.top_case(n)
    st, cells = built(tmp_path, c)
    tax = c["tax"]
    hdr, _, ob, tb = u.read_db(str(tmp_path / "db"))
    assert hdr[2:] == bits
    ts = st["taxon_stats"]
    counts = t.value_counts(u.cells_of(c["model"])[1], bits[1], tax.node_count)
    assert len(ts) == n + 1 and (ts[-1]["taxid"], ts[-1]["cells"]) == (c["last"], counts[-1]) and counts[-1] > 0
    assert ts[1]["taxid"] == 10 and ts[1]["cells"] == counts[2] > 0
    # the last taxon's reads on the built database against the oracle on the same files
    reads = [s for name, s in c["records"][c["last"]] if name.startswith(b"own")]
    reads += [reads[0][:50], reads[0][7:]]
    bases, offs = orc.pack_reads(reads, False)
    odb = orc.OracleDB(directory=str(tmp_path / "db"))
    odb.set(ambiguity_rule=u.rule(), minimum_hit_groups=1)
    exp, lookups, etaxa, _ = odb.classify(bases, offs, False, 0.0, want_taxa=True)
    assert [int(odb.external_ids[int(x)]) for x in exp["call"]] == [c["last"]] * len(reads)
    with Engine.open(str(tmp_path / "db")) as eng:
        chk = eng.db_check()
        assert chk.non_empty_cells == st["size"] and chk.max_value == tax.node_count - 1
        eng.set_options(minimum_hit_groups=1)
        eng.reset_stats()
        got, taxa, _ = eng.classify(bases, offs, False, 0.0, want_taxa=True)
        for f in ("call", "total_kmers", "clade_hits", "hit_groups"):
            assert np.array_equal(got[f], exp[f]), f
        assert np.array_equal(taxa, etaxa)
        assert [eng.external_id(int(x)) for x in got["call"]] == [c["last"]] * len(reads)
        assert eng.stats().table_lookups == int(lookups.sum())
    assert minidb.value_bits_for(tax.node_count) == bits[1]
