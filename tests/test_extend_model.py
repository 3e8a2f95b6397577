"""tests/extend_model.py against oracle/minidb.py: a base extended by the model is the table that minidb.build_hash makes of the
union in one go (build_db_util.same_table), for every way of splitting a tree into base and addition; and the shadow rule on
forged cells.  CPU only."""
import struct

import numpy as np
import pytest

from oracle import k2_literal as lit
from oracle import minidb
from tests import build_db_util as u
from tests import build_taxa_util as t
from tests import extend_cases as xc
from tests import extend_model as xm


def _extended(c):
    base = xc.base_hash(c["base_tax"], c["base_pairs"], c["cap"])
    return base, xm.extend(base, xc.taxo_bytes(c["base_tax"]), c["add_lines"], c["add_pairs"])


def test_the_fast_base_builder_is_build_hash():
    c = xc.case("between", 2)
    want, size = t.model(c["base_tax"], c["base_pairs"], c["cap"])
    got = xc.base_hash(c["base_tax"], c["base_pairs"], c["cap"])
    assert u.cells_of(got)[0] == u.cells_of(want)[0] == (c["cap"], size, 30, 2)
    u.same_table(u.cells_of(got), u.cells_of(want))


@pytest.mark.parametrize("name", ["leaf", "inner", "existing", "one", "two", "between", "wide3"])
def test_extension_is_the_one_shot_table(name):
    c = xc.case(name, 2)
    base, x = _extended(c)
    tree = name in ("leaf", "inner", "existing")  # (their union is the tree of the multi-taxon tests, whose model is made once)
    want, size = (t.tree_case()["model"], t.tree_case()["size"]) if tree else t.model(c["union_tax"], c["union_pairs"], c["cap"])
    assert not tree or (sorted(c["union_pairs"]) == sorted(t.tree_case()["pairs"]) and c["union_tax"].external == t.tree_case()["tax"].external)
    hdr, cells = u.cells_of(x["hash"])
    vb = minidb.value_bits_for(c["union_tax"].node_count)
    assert hdr == (c["cap"], size, 32 - vb, vb) and x["shadowed"] == 0
    xc.colliding_keys_apart(u.fast_minimizers([s for _, s in c["union_pairs"]]), c["cap"], vb, cells)
    u.same_table((hdr, cells), u.cells_of(want))
    assert x["tax"].external == c["union_tax"].external and x["tax"].parent == c["union_tax"].parent
    # per node: what the base held, renumbered, and what the union holds
    old = t.value_counts(u.cells_of(base)[1], x["old_vb"], c["base_tax"].node_count)
    assert sum(x["base_cells"]) == sum(old) and all(x["base_cells"][x["remap"][i]] == n for i, n in enumerate(old))
    assert x["cells"] == t.value_counts(u.cells_of(want)[1], vb, c["union_tax"].node_count)


def test_the_cases_cover_what_they_are_for():
    d = {n: _extended(xc.case(n, 2))[1] for n in ("one", "two", "between", "wide3", "existing")}
    assert (d["one"]["old_vb"], d["one"]["new_vb"]) == (2, 2) and d["one"]["remap"] == [0, 1, 2]
    assert (d["two"]["old_vb"], d["two"]["new_vb"]) == (2, 3) and d["two"]["remap"] == [0, 1, 2]
    assert d["between"]["remap"] == [0, 1, 2, 4] and d["between"]["new_vb"] == 3  # 30 moves behind the new 20
    assert (d["wide3"]["old_vb"], d["wide3"]["new_vb"]) == (2, 9)  # delta 7
    assert d["existing"]["remap"] == list(range(6)) and d["existing"]["new_vb"] == d["existing"]["old_vb"] == 3
    assert xm.extend(*_tree_wide_base())["new_vb"] == 9


def _tree_wide_base():
    c = xc.case("tree_wide")
    return xc.base_hash(c["base_tax"], c["base_pairs"], c["cap"]), xc.taxo_bytes(c["base_tax"]), c["add_lines"], c["add_pairs"]


def test_merge_refuses_what_the_library_refuses():
    tb = xc.taxo_bytes(t.taxonomy_of(t.TREE_LINES))
    with pytest.raises(AssertionError, match="nowhere"):
        xm.merge(tb, [(55, 54, "orphan")])
    with pytest.raises(AssertionError, match="under 100"):
        xm.merge(tb, [(t.A, 1, "taxon A")])
    tax, remap = xm.merge(tb, [(15, t.G, "between A and B"), (t.B, t.G, "another name")])
    assert tax.external == [0, 1, t.C_, t.G, t.A, 15, t.B] and remap == [0, 1, 2, 3, 4, 6] and tax.names[t.B] == "taxon B"


def test_shadowed_cells_get_the_lca_and_stay():
    s = xc.shadow_case()
    cap, K = s["cap"], s["K"]
    base = xc.base_hash(s["tax"], [], cap, forged=s["forged"])
    (_, size, _, vb), cells = u.cells_of(base)
    assert vb == 2 and size == 8 and cells[cap - 1] == (2 * K) << 2 | s["tax"].internal[xc.X_ID] and cells[0] == (2 * K + 1) << 2 | s["tax"].internal[xc.Y_ID]
    assert (xm.runs_of(cells)[[cap - 1, 0, 1, 2]] == xm.runs_of(cells)[0]).all() and cells[cap - 2] == 0 and cells[3] == 0  # the run wraps
    tb = xc.taxo_bytes(s["tax"])
    x = xm.extend(base, tb, [s["z_line"]], forged=[(xc.Z_ID, s["z_filler"][0])])
    (_, size_x, kb, vb_x), out = u.cells_of(x["hash"])
    assert (kb, vb_x) == (29, 3) and x["shadowed"] == 1 and size_x == size + 1
    assert out[cap - 1] == out[0] == K << 3 | 1  # both cells: the key K and the root
    assert np.array_equal(out != 0, np.where(np.arange(cap) == lit.fmix64(s["z_filler"][0]) % cap, True, cells != 0))
    # a third minimizer of the key, for Z: the first cell of the key on its path stays the root, and no cell is claimed for it
    y = xm.extend(base, tb, [s["z_line"]], forged=[(xc.Z_ID, s["z_filler"][0]), (xc.Z_ID, s["m4"])])
    assert y["size"] == x["size"] and y["hash"] == x["hash"]


def test_a_run_that_is_the_whole_table_but_one_cell():
    """capacity 8, cells 1..7 occupied, the keys of cells 6 and 2 equal after the re-key: one run (it does not wrap, the next case
    does), and the order of the group follows the run, not the cell index"""
    tax = t.taxonomy_of(((7, 1, "x"), (8, 1, "y")))
    tb = xc.taxo_bytes(tax)
    for shift in (0, 3):  # shift 3: the empty cell is cell 3 and the run wraps
        cells = np.zeros(8, dtype=np.uint32)
        for i in range(1, 8):
            cells[(i + shift) % 8] = (100 + 2 * i) << 2 | 2
        cells[(2 + shift) % 8] = (50 << 2) | 2
        cells[(6 + shift) % 8] = (51 << 2) | 3
        base = struct.pack("<4Q", 8, 7, 30, 2) + cells.tobytes()
        x = xm.extend(base, tb, [(9, 1, "z")])
        _, out = u.cells_of(x["hash"])
        assert x["shadowed"] == 1 and out[(2 + shift) % 8] == out[(6 + shift) % 8] == (25 << 3) | 1
        assert x["size"] == 7 and (out != 0).sum() == 7
