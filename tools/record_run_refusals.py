#!/usr/bin/env python3
"""Record tests/golden/run_refusals.json: the (code, message) of every bad call in tests/run_refusals.py, through the standalone
entry and through its engine twin.  Run it against a build of the commit BEFORE a change to the run entries, never against the
code under test.

    python tools/record_run_refusals.py          # the cases refused before any device is touched (needs no GPU)
    python tools/record_run_refusals.py --gpu    # also the cases refused by the run itself, the database open (needs a GPU)

Without --gpu the "gpu" part of an existing file is kept as it is."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import run_refusals as rr  # noqa: E402


def record(L, cases, engine):
    out = {}
    for c in cases:
        with tempfile.TemporaryDirectory() as d:
            before = rr.make_files(d)
            out[c["id"]] = [rr.call(L, c, d, False), rr.call(L, c, d, engine)]
            assert sorted(os.listdir(d)) == before, (c["id"], sorted(os.listdir(d)))
        assert out[c["id"]][0][0] != 0 and out[c["id"]][1][0] != 0, (c["id"], out[c["id"]])
    return out


def main():
    from nohuman_amd import Engine, _lib
    L = _lib.lib()
    old = json.load(open(rr.GOLDEN)) if os.path.exists(rr.GOLDEN) else {}
    doc = {"cpu": record(L, rr.CPU_CASES, None), "gpu": old.get("gpu", {})}
    if "--gpu" in sys.argv[1:]:
        with Engine.open(rr.DB) as eng:
            doc["gpu"] = record(L, rr.GPU_CASES, eng.handle)
    path = sys.argv[sys.argv.index("-o") + 1] if "-o" in sys.argv else rr.GOLDEN
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d + %d cases" % (path, len(doc["cpu"]), len(doc["gpu"])))


if __name__ == "__main__":
    main()
