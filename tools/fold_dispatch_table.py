#!/usr/bin/env python3
"""Write tests/golden/fold_dispatch.json: which kernel ftar::launch_reduce reaches, or which status refuses the
call, for every call of tests/fold_dispatch_cases.py's grid (tests/test_gpu_fold_dispatch.py compares).

    tools/fold_dispatch_table.py [--out FILE] [--rev COMMIT --dirty PATHS]

Needs a GPU and the built libraries.  The file records the commit it was made from and the paths that differed
from it (git rev-parse HEAD, git status --porcelain; --rev / --dirty give them where the tree travels without its
history).  It pins the dispatch of that commit: regenerate it only for a change that is meant to reroute a call.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "allreduce-over-mpi_amd"), os.path.join(ROOT, "tests")]

import fold_dispatch_cases as fdc  # noqa: E402


def git(*args):
    return subprocess.run(["git", "-C", ROOT, *args], check=True, capture_output=True, text=True).stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fold_dispatch.json"))
    ap.add_argument("--rev", help="the commit of this tree (default: git rev-parse HEAD)")
    ap.add_argument("--dirty", help="comma-separated paths that differ from it (default: git status --porcelain)")
    a = ap.parse_args()
    rev = a.rev or git("rev-parse", "HEAD").strip()
    if a.dirty is not None:
        dirty = [p for p in a.dirty.split(",") if p]
    else:
        dirty = [l[3:] for l in git("status", "--porcelain").splitlines()]

    cases = list(fdc.grid())
    results = fdc.run(cases)
    table, runs = fdc.encode(results)
    assert fdc.decode(table, runs) == results
    doc = {"commit": rev, "dirty": bool(dirty), "dirty_paths": dirty, "axes": fdc.axes(), "cases": len(cases),
           "kernels": table, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    refused = sum(isinstance(r, int) for r in results)
    print("%d cases: %d launched on %d kernels, %d refused; %d runs, %d bytes -> %s" % (
        len(cases), len(cases) - refused, len(table), refused, len(runs) // 2, os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()
