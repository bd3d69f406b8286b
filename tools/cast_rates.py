#!/usr/bin/env python3
"""ftar_cast_scaled (wide <-> fp8 times a device scale) on cold data, against the project's copy kernel moving the
same total bytes, in one run.  The wide side is 256 MiB; launches rotate over 4 disjoint (source, destination)
buffer sets, so nothing is left in the Infinity Cache from the launch before; GB/s of bytes read plus bytes
written, median of interleaved rounds with the slowest and fastest round next to it.  Labels:

  f32>f8e4m3          the production dispatch (ftar.cast_scaled), every one of the 12 pairs by default
  f32>f8e4m3+amax     the same with the amax word (a 4-byte memset and the amax kernel)
  f32>f8e4m3+sr       the stochastic-rounding quantize (ftar_cast_scaled_sr, rounding="stochastic") of the six
                      quantize pairs (--sr), interleaved with the RNE quantize of the same pair, its yardstick;
                      the last lines give each pair's ratio of medians
  f32>f8e4m3@L.U      layout candidate L (0 lane-owned vectors, 1 the same staged through LDS, 2 lane-contiguous
                      wide vectors with 4- / 8-byte fp8 accesses) at U vectors per lane and pass, through
                      libftar_bench.so's ftar_debug_cast_variant (--layouts)
  copy:320            launch_copy (ftar.reduce, k = 1, u8) of 160 MiB: 320 MiB moved, an f32 pair's total;
                      copy:384 is a 16-bit pair's
  ...#2               any label again under a name of its own: the tool's own spread between two runs of one
                      kernel, the margin for "as fast as the copy"

Random bytes on both sides, so lanes hold NaN and inf too: the instructions do not care.
python tools/cast_rates.py [--pairs f32>f8e4m3,...] [--layouts] [--amax] [--sr] [--rounds 5] [--reps 8]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "allreduce-over-mpi_amd"))
import torch  # noqa: E402
import ftar  # noqa: E402

WIDE, F8 = ("f32", "bf16", "f16"), ("f8e4m3", "f8e5m2")
ALL = [f"{w}>{f}" for w in WIDE for f in F8] + [f"{f}>{w}" for f in F8 for w in WIDE]
VARIANTS = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (2, 4)]
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", default=",".join(ALL))
ap.add_argument("--layouts", action="store_true", help="also every layout candidate of --layout-pairs")
ap.add_argument("--layout-pairs", default="f32>f8e4m3,bf16>f8e4m3,f8e4m3>f32,f8e4m3>bf16")
ap.add_argument("--amax", action="store_true", help="also every pair with the amax word")
ap.add_argument("--sr", action="store_true", help="also every quantize pair with stochastic rounding")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=8)
a = ap.parse_args()
NB = 256 << 20
S = 4
bufs = [[torch.randint(0, 256, (NB,), dtype=torch.uint8, device="cuda") for _ in range(2)] for _ in range(S)]
stream = torch.cuda.current_stream()
scale = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
word = torch.zeros(1, dtype=torch.float32, device="cuda")
seed = torch.full((1,), 0x5EED, dtype=torch.int64, device="cuda")
hook = ftar.bench_lib().ftar_debug_cast_variant
hook.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                 ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]


def moved(pair):
    s, d = pair.split(">")
    n = NB // max(ftar.dtype_size(s), ftar.dtype_size(d))
    return n, n * (ftar.dtype_size(s) + ftar.dtype_size(d))


def make(label):
    """(launch(i), bytes moved) of one label."""
    base = label.split("#")[0]
    if base.startswith("copy:"):
        total = int(base[5:]) << 20
        return (lambda i: ftar.reduce([bufs[i % S][0]], bufs[i % S][1], total // 2, "u8", "sum", stream=stream)), total
    pair, _, var = base.partition("@")
    pair, plus, _ = pair.partition("+")   # _: "amax" or "sr"
    s, d = pair.split(">")
    n, total = moved(pair)
    if var:
        lay, u = (int(x) for x in var.split("."))

        def launch(i):
            st = hook(lay, u, bufs[i % S][0].data_ptr(), ftar.DTYPE[s], bufs[i % S][1].data_ptr(), ftar.DTYPE[d], n,
                      scale.data_ptr(), stream.cuda_stream)
            assert st == 0, (label, st, ftar.last_error())
        return launch, total
    if plus and _ == "sr":
        return (lambda i: ftar.cast_scaled(bufs[i % S][0], bufs[i % S][1], n, s, d, scale=scale, stream=stream,
                                           rounding="stochastic", seed=seed, offset=i * n)), total
    am = word if plus else None
    return (lambda i: ftar.cast_scaled(bufs[i % S][0], bufs[i % S][1], n, s, d, scale=scale, amax=am, stream=stream)), total


pairs = a.pairs.split(",")
labels = list(pairs) + [pairs[0] + "#2"]
if a.amax:
    labels += [p + "+amax" for p in pairs]
sr_pairs = [p for p in pairs if p.split(">")[1] in F8] if a.sr else []
labels += [p + "+sr" for p in sr_pairs]
if a.layouts:
    labels += [f"{p}@{lay}.{u}" for p in a.layout_pairs.split(",") for lay, u in VARIANTS]
for mib in sorted({moved(p)[1] >> 20 for p in pairs}):
    labels += [f"copy:{mib}", f"copy:{mib}#2"]
runs = {lb: make(lb) for lb in labels}
res = {}
for _ in range(a.rounds):
    for lb, (launch, total) in runs.items():
        for i in range(S):
            launch(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(a.reps):
            launch(i)
        e1.record(stream)
        torch.cuda.synchronize()
        res.setdefault(lb, []).append(e0.elapsed_time(e1) / a.reps)
for lb, ts in res.items():
    total = runs[lb][1]
    med = statistics.median(ts)

    def rate(ms):
        return round(total / ms / 1e6, 1)
    print(json.dumps({"label": lb, "MiB_moved": total >> 20, "ms_med": round(med, 4), "GBps_med": rate(med),
                      "GBps_slowest": rate(max(ts)), "GBps_fastest": rate(min(ts))}), flush=True)
for p in sr_pairs:
    print(json.dumps({"label": p + "+sr / " + p, "ratio_of_medians": round(statistics.median(res[p]) /
                                                                          statistics.median(res[p + "+sr"]), 3)}), flush=True)
