"""The model of the host selection (tests/host_model.py) itself: hand cases on the toy taxonomy
1 -> {10 -> {11 -> {111, 112}, 12}, 20 -> {21, 9606}}, and agreement with the per-taxon outputs' rule (tests/taxout_model.py
bin_of: the deepest selected ancestor-or-self) for every host / keep split of every subset of up to three taxids.  No GPU needed."""
import itertools

import pytest

from tests import host_model as hm
from tests import synth
from tests import taxout_model as tm

PARENT = dict(synth.TOY_EDGES)
ALL = sorted(PARENT)


def _hosts(host, keep=()):
    m = hm.host_of(PARENT, host, keep)
    assert sorted(m) == ALL
    return {t for t in ALL if m[t]}


def test_the_root_is_every_classified_fragment():
    assert _hosts([1]) == set(ALL)


def test_one_leaf():
    assert _hosts([9606]) == {9606}


def test_keep_inside_host():
    assert _hosts([10], [11]) == {10, 12}


def test_host_inside_keep_inside_host():
    assert _hosts([1, 111], [10]) == {1, 20, 21, 9606, 111}
    assert _hosts([111, 1], [10]) == {1, 20, 21, 9606, 111}  # (the order of a list carries no meaning)


def test_keep_nested_in_keep():
    assert _hosts([1], [10, 11]) == {1, 20, 21, 9606}
    assert _hosts([1], [11, 10]) == {1, 20, 21, 9606}


def test_unclassified_is_never_host_and_the_table_has_a_zero_first():
    m = hm.host_of(PARENT, [1])
    assert not hm.is_host(0, m) and hm.is_host(1, m) and hm.is_host(9606, m)
    ext = [0] + ALL
    assert hm.table(ext, m) == bytes([0] + [1] * len(ALL))
    assert hm.table(ext, hm.host_of(PARENT, [20], [21])) == bytes([0] + [int(t in (20, 9606)) for t in ALL])


def test_what_the_model_refuses():
    for host, keep in (([10, 10], []), ([10], [10]), ([0], []), ([], [10]), ([4242], []), ([1], [4242])):
        with pytest.raises(AssertionError):
            hm.host_of(PARENT, host, keep)


def test_agrees_with_the_per_taxon_rule_on_every_split_of_up_to_three_taxids():
    n = 0
    for size in (1, 2, 3):
        for sel in itertools.combinations(ALL, size):
            bins = tm.bin_of(PARENT, list(sel))
            for roles in itertools.product((True, False), repeat=size):  # True: a host taxid
                host = [t for t, r in zip(sel, roles) if r]
                keep = [t for t, r in zip(sel, roles) if not r]
                if not host:
                    continue  # (keep taxids alone are refused)
                m = hm.host_of(PARENT, host, keep)
                for node in ALL:
                    k = bins[node]
                    assert m[node] == (k is not None and sel[k] in host), (sel, roles, node)
                n += 1
    assert n == 9 * 1 + 36 * 3 + 84 * 7


def test_filtering_a_keep_human_output_and_an_input():
    recs = [(b"@a x", b"ACGT", b"IIII"), (b"@b", b"GG", b"##"), (b"@c", b"TTT", b"FFF"), (b"@d", b"CA", b"AB")]
    calls = [111, 0, 12, 9606]
    m = hm.host_of(PARENT, [10], [11])
    assert hm.kept(recs, calls, m, True) == b"@a x\nACGT\n+\nIIII\n@b\nGG\n+\n##\n@d\nCA\n+\nAB\n"
    assert hm.removed(recs, calls, m, True) == b"@c kraken:taxid|12\nTTT\n+\nFFF\n"
    assert hm.masked(recs, calls, m, True) == b"@a x\nACGT\n+\nIIII\n@b\nGG\n+\n##\n@c\nNNN\n+\nFFF\n@d\nCA\n+\nAB\n"
    assert hm.ids([b"a", b"b", b"c", b"d"], calls, m) == b"c\n"
    keep_human = b"".join(hm.normalised(r, True, c) for r, c in zip(recs, calls) if c)
    assert hm.filter_keep_human(keep_human, True, m) == hm.removed(recs, calls, m, True)
    assert hm.filter_keep_human(keep_human, True, hm.host_of(PARENT, [1])) == keep_human
    fa = [(b">s", b"ACGTAC", b"")]
    assert hm.kept(fa, [21], hm.host_of(PARENT, [9606]), False) == b">s\nACGTAC\n"
    assert hm.removed(fa, [21], hm.host_of(PARENT, [20]), False) == b">s kraken:taxid|21\nACGTAC\n"
