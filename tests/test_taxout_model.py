"""The routing rule of the per-taxon outputs (tests/taxout_model.py) on the golden calls of the toy database at confidence 0.0:
taxonomy 1 -> {10 -> {11 -> {111, 112}, 12}, 20 -> {21, 9606}}.  No GPU needed."""
import json
import os

import pytest

from tests import taxout_model as tm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEL = [10, 11, 9606, tm.OTHER]


def _golden(name):
    exp = json.load(open(os.path.join(GOLD, name)))
    ext = exp["meta"]["external_ids"]
    return tm.parent_map(ext, exp["meta"]["parent"]), [ext[r["by_conf"]["0.0"][0]] for r in exp["records"]]


@pytest.mark.parametrize("name", ["expected_se.json", "expected_pe.json"])
def test_every_classified_fragment_lands_in_exactly_one_bin(name):
    parent, calls = _golden(name)
    got = tm.route_calls(calls, parent, SEL)
    flat = sorted(i for b in got for i in b)
    assert flat == [i for i, c in enumerate(calls) if c]  # each once, no unclassified one
    assert all(b == sorted(b) for b in got)  # input order inside a bin
    assert all(got), "an empty bin"


def test_nested_selector_takes_its_clade_away_from_the_outer_one():
    parent, calls = _golden("expected_se.json")
    got = tm.route_calls(calls, parent, SEL)
    assert {calls[i] for i in got[1]} == {11, 111, 112}
    assert {calls[i] for i in got[0]} == {10, 12}
    assert {calls[i] for i in got[2]} == {9606}
    assert {calls[i] for i in got[3]} == {1, 20, 21}
    assert [len(b) for b in got] == [78, 51, 10, 112]


def test_pe_goldens_have_calls_at_every_node():
    parent, calls = _golden("expected_pe.json")
    for node in parent:
        assert sum(c == node for c in calls) >= 13, node


def test_without_other_the_rest_lands_nowhere():
    parent, calls = _golden("expected_se.json")
    got = tm.route_calls(calls, parent, SEL[:3])
    assert [len(b) for b in got] == [78, 51, 10]
    taken = {i for b in got for i in b}
    assert {calls[i] for i in range(len(calls)) if calls[i] and i not in taken} == {1, 20, 21}


def test_root_as_a_selector_equals_other():
    parent, calls = _golden("expected_se.json")
    assert tm.route_calls(calls, parent, [10, 11, 9606, 1]) == tm.route_calls(calls, parent, SEL)
    # ... but not once both are given: the root then takes everything `other` would
    got = tm.route_calls(calls, parent, [1, tm.OTHER])
    assert len(got[0]) == sum(1 for c in calls if c) and got[1] == []


def test_partition_cuts_a_classified_out_text():
    parent, _ = _golden("expected_se.json")
    fq = b"@a kraken:taxid|111\nAC\n+\nII\n@b x kraken:taxid|20\nG\n+\nI\n@c kraken:taxid|12\n\n+\n\n"
    files, counts = tm.partition(fq, True, parent, SEL)
    assert counts == [1, 1, 0, 1]
    assert files[0] == b"@c kraken:taxid|12\n\n+\n\n" and files[1].startswith(b"@a ") and files[3].startswith(b"@b x ")
    assert b"".join(sorted(files)) == b"".join(sorted(tm.records(fq, True)))
    fa = b">a kraken:taxid|9606\nACGT\n>b kraken:taxid|1\nAC\n"
    files, counts = tm.partition(fa, False, parent, [9606])
    assert counts == [1] and files[0] == b">a kraken:taxid|9606\nACGT\n"
    with pytest.raises(AssertionError):
        tm.bin_of(parent, [4242])
    with pytest.raises(AssertionError):
        tm.bin_of(parent, [10, 10])
