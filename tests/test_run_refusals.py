"""Every refusal of the whole-run entries, byte for byte: the table of bad calls in tests/run_refusals.py goes through each
standalone nh_run_* entry and through its nh_run_engine_* twin, and code and full message are those recorded in
tests/golden/run_refusals.json (tools/record_run_refusals.py, from the commit before the entries were last changed).  After every
case the directory holds no new file.  The first test needs no GPU: every case of it returns before a device is touched."""
import json
import os

import pytest

from tests import run_refusals as rr


@pytest.fixture(scope="module")
def golden():
    with open(rr.GOLDEN) as f:
        return json.load(f)


def _drive(cases, want, engine, tmp_path):
    from nohuman_amd import _lib
    L = _lib.lib()
    assert sorted(want) == sorted(c["id"] for c in cases)  # the table and the recording hold the same cases
    for c in cases:
        d = tmp_path / c["id"]
        d.mkdir()
        before = rr.make_files(str(d))
        got = [rr.call(L, c, str(d), False), rr.call(L, c, str(d), engine)]
        print(c["id"], got)
        assert got == want[c["id"]], c["id"]
        if c.get("same", True):  # an argument error: the two entries say the same
            assert got[0] == got[1], c["id"]
        assert got[0][0] != 0 and got[1][0] != 0, c["id"]
        assert sorted(os.listdir(str(d))) == before, c["id"]  # no file created


def test_refusals_before_any_device(golden, tmp_path):
    _drive(rr.CPU_CASES, golden["cpu"], None, tmp_path)


@pytest.mark.gpu
def test_refusals_of_the_run_itself(golden, tmp_path):
    """the database open, before the first kernel: paired input without out2, a confidence and a codec out of range, a missing
    input, an output hard-linked to the input, a selector's and a host taxid that the taxonomy does not hold"""
    from nohuman_amd import Engine
    with Engine.open(rr.DB) as eng:
        _drive(rr.GPU_CASES, golden["gpu"], eng.handle, tmp_path)
