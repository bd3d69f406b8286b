#!/usr/bin/env python3
"""Every fp32 bit pattern through the stochastic narrowing to e4m3 and e5m2 (include/ftar.h: ftar_cast_scaled_sr),
against the contract in integers, on the GPU (libftar_bench.so: ftar_bench_sr_sweep).  Run once when the narrowing
changes, not in the suite.  Six words per input: 0, 1, 2^31, 2^32 - 1, the input's threshold 2^32 - F (the smallest
word that rounds up) and 2^32 - F - 1 (the largest that rounds down).  Three modes:

  production   SrFmt::pack in every byte position and SrFmt::narrow, the device functions the kernels call
  bare         v_cvt_sr_fp8_f32 / v_cvt_sr_bf8_f32 alone, fed the word as it is
  bare>>       the instruction alone, fed the word shifted right by 32 - d (d = 23 - m dropped bits): the top
               of the word under the dropped bits if the instruction adds the low d bits of its operand

Mismatches are counted per fp32 exponent field (0 .. 255) and printed as ranges of fields, with one example each
(input bits, word, got, want).  The production mode must show none; the bare modes show where the instruction
alone equals the contract, which is what SrFmt's use of it stands on (csrc/cast_impl.h).
python tools/sr_sweep.py [--chunks 16]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "allreduce-over-mpi_amd"))
import ftar  # noqa: E402

MODES, WORDS = ("production", "bare", "bare>>"), ("0", "1", "2^31", "2^32-1", "2^32-F", "2^32-F-1")
ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=16, help="launches per format (progress is printed after each)")
a = ap.parse_args()
hook = ftar.bench_lib().ftar_bench_sr_sweep
hook.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
bad_total = 0
for e5m2, name in ((0, "f8e4m3"), (1, "f8e5m2")):
    bad = np.zeros((3, 6, 256), np.uint64)
    ex = np.full((3, 256, 4), 0xFFFFFFFF, np.uint32)
    step = (1 << 32) // a.chunks
    for c in range(a.chunks):
        first = c * step
        count = (1 << 32) - first if c == a.chunks - 1 else step
        st = hook(e5m2, first, count, bad.ctypes.data, ex.ctypes.data)
        assert st == 0, (st, ftar.last_error())
        print(f"# {name}: {first + count:#x} inputs done", flush=True)
    for m, mode in enumerate(MODES):
        per_exp = bad[m].sum(axis=0)
        ranges, e = [], 0
        while e < 256:
            if per_exp[e]:
                lo = e
                while e + 1 < 256 and per_exp[e + 1]:
                    e += 1
                x = ex[m, lo]
                ranges.append({"exponent_fields": [lo, e], "mismatches": int(per_exp[lo:e + 1].sum()),
                               "example": {"input": hex(int(x[0])), "word": hex(int(x[1])), "got": hex(int(x[2])),
                                           "want": hex(int(x[3]))}})
            e += 1
        print(json.dumps({"format": name, "mode": mode, "mismatches": int(bad[m].sum()),
                          "by_word": {w: int(bad[m, j].sum()) for j, w in enumerate(WORDS)}, "ranges": ranges}), flush=True)
    bad_total += int(bad[0].sum())
print(json.dumps({"production_mismatches": bad_total}))
sys.exit(1 if bad_total else 0)
