"""Every call of tests/fold_dispatch_cases.py's grid still reaches the kernel, or the refusal, that
tests/golden/fold_dispatch.json records (tools/fold_dispatch_table.py wrote it).  Right bits do not show routing:
a fold sent to another tile shape, to the register kernel or past its HOT computes the same result."""
import json
import os

import pytest

import fold_dispatch_cases as fdc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_dispatch.json")


def test_fold_dispatch_record_is_whole():
    """The file holds one entry for every call of today's grid, built from the same axes, and stays small."""
    doc = json.load(open(GOLDEN))
    cases = list(fdc.grid())
    assert doc["axes"] == fdc.axes()
    assert doc["cases"] == len(cases) == len(fdc.decode(doc["kernels"], doc["runs"]))
    assert os.path.getsize(GOLDEN) < 256 << 10
    assert len(set(cases)) == len(cases)


@pytest.mark.gpu
def test_fold_dispatch_matches_record():
    doc = json.load(open(GOLDEN))
    cases = list(fdc.grid())
    assert doc["axes"] == fdc.axes(), "the record was made from another grid"
    want = fdc.decode(doc["kernels"], doc["runs"])
    assert len(want) == len(cases), ("grid entries missing from the record", len(want), len(cases))
    got = fdc.run(cases)
    bad = [(c, w, g) for c, w, g in zip(cases, want, got) if w != g]
    assert not bad, "%d of %d calls rerouted (status codes are refusals); the first:\n%s" % (
        len(bad), len(cases), "\n".join("  %s\n    was %s\n    now %s" % b for b in bad[:12]))
