#!/usr/bin/env python3
"""The MX block-scaled casts (ftar_mx_scales, ftar_mx_quantize, ftar_mx_dequantize) on cold data, against
ftar_cast_scaled of the same pair and the project's copy kernel moving the same total bytes, in one run.  The wide
side is 256 MiB; launches rotate over 4 disjoint (source, destination, scales) buffer sets, so nothing is left in
the Infinity Cache from the launch before; GB/s of bytes read plus bytes written (the scale bytes included), median
of interleaved rounds with the slowest and fastest round next to it.  Labels:

  f32>f8e4m3:mx       ftar_mx_quantize, FTAR_MX_COMPUTE (one pass: scales and payload); f8e4m3>f32:mx: ftar_mx_dequantize
  f32>f8e4m3:given    ftar_mx_quantize, FTAR_MX_GIVEN (reads the scale bytes)
  f32>f8e4m3:scales   ftar_mx_scales (reads the source, writes the scale bytes only)
  f32>f8e4m3          ftar_cast_scaled of the pair: the yardstick of its MX kernels
  copy:320            launch_copy (ftar.reduce, k = 1, u8) moving that many MiB in all
  ...#2               a label again under a name of its own: the run's own spread between two labels of one kernel,
                      the margin of every comparison

With --sr, for every quantize pair also:
  f32>f8e4m3:mx-sr    ftar_mx_quantize_sr, FTAR_MX_COMPUTE
  f32>f8e4m3:given-sr ftar_mx_quantize_sr, FTAR_MX_GIVEN
  f32>f8e4m3:sr       ftar_cast_scaled_sr of the pair: the stochastic yardstick

The last lines give each MX label's ratio to its pair's ftar_cast_scaled (medians; > 1 is faster), and with --sr each
stochastic MX label's ratio to its two yardsticks of the same run: the round-to-nearest label of its pair and mode,
and ftar_cast_scaled_sr of its pair.  Random bytes on all sides, so blocks hold NaN and inf too and scale bytes are
any byte: the instructions do not care.
python tools/mx_rates.py [--pairs f32>f8e4m3,...] [--rounds 5] [--reps 8] [--sr]"""
import argparse
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
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", default=",".join(ALL))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--sr", action="store_true", help="also the stochastic quantizes of every quantize pair")
a = ap.parse_args()
NB = 256 << 20
S = 4
bufs = [[torch.randint(0, 256, (NB,), dtype=torch.uint8, device="cuda") for _ in range(2)] for _ in range(S)]
scs = [torch.randint(0, 256, (NB // 2 // 32,), dtype=torch.uint8, device="cuda") for _ in range(S)]
stream = torch.cuda.current_stream()
scale = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
seed = torch.tensor([0x0123456789ABCDEF], dtype=torch.int64, device="cuda")


def shape(pair):
    """(elements, bytes of the two sides, scale bytes)"""
    s, d = pair.split(">")
    n = NB // max(ftar.dtype_size(s), ftar.dtype_size(d))
    return n, n * (ftar.dtype_size(s) + ftar.dtype_size(d)), ftar.mx_nblocks(n)


def make(label):
    """(launch(i), bytes moved) of one label."""
    base = label.split("#")[0]
    if base.startswith("copy:"):
        total = int(base[5:]) << 20
        return (lambda i: ftar.reduce([bufs[i % S][0]], bufs[i % S][1], total // 2, "u8", "sum", stream=stream)), total
    pair, _, kind = base.partition(":")
    s, d = pair.split(">")
    n, both, nb = shape(pair)
    if kind == "sr":
        return (lambda i: ftar.cast_scaled(bufs[i % S][0], bufs[i % S][1], n, s, d, scale=scale, stream=stream,
                                           rounding="stochastic", seed=seed, offset=i * n)), both
    if kind in ("mx-sr", "given-sr"):
        mode = "compute" if kind == "mx-sr" else "given"
        return (lambda i: ftar.mx_quantize(bufs[i % S][0], bufs[i % S][1], scs[i % S], n, s, d, mode=mode, stream=stream,
                                           rounding="stochastic", seed=seed, offset=i * n)), both + nb
    if not kind:
        return (lambda i: ftar.cast_scaled(bufs[i % S][0], bufs[i % S][1], n, s, d, scale=scale, stream=stream)), both
    if kind == "scales":
        return (lambda i: ftar.mx_scales(bufs[i % S][0], scs[i % S], n, s, d, stream=stream)), n * ftar.dtype_size(s) + nb
    if d in F8:
        mode = "compute" if kind == "mx" else "given"
        return (lambda i: ftar.mx_quantize(bufs[i % S][0], bufs[i % S][1], scs[i % S], n, s, d, mode=mode,
                                           stream=stream)), both + nb
    return (lambda i: ftar.mx_dequantize(bufs[i % S][0], scs[i % S], bufs[i % S][1], n, s, d, stream=stream)), both + nb


pairs = a.pairs.split(",")
labels, mx_of = [], {}
for p in pairs:
    kinds = ("mx", "given", "scales") if p.split(">")[1] in F8 else ("mx",)
    mx_of[p] = [f"{p}:{k}" for k in kinds]
    labels += mx_of[p] + [p]
sr_of = {p: [f"{p}:mx-sr", f"{p}:given-sr"] for p in pairs if a.sr and p.split(">")[1] in F8}
for p, lbs in sr_of.items():
    labels += lbs + [f"{p}:sr"]
labels += [mx_of[pairs[0]][0] + "#2", pairs[0] + "#2"]
if sr_of:
    labels += [sr_of[next(iter(sr_of))][0] + "#2"]
for mib in sorted({(shape(p)[1] + shape(p)[2]) >> 20 for p in pairs}):
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
for p in pairs:
    for lb in mx_of[p]:
        print(json.dumps({"label": f"{lb} / {p}", "time_ratio_cast_over_mx": round(statistics.median(res[p]) /
                                                                                  statistics.median(res[lb]), 3),
                          "GBps_ratio_mx_over_cast": round((runs[lb][1] / statistics.median(res[lb])) /
                                                           (runs[p][1] / statistics.median(res[p])), 3)}), flush=True)
for p, lbs in sr_of.items():
    for lb in lbs:
        t = statistics.median(res[lb])
        print(json.dumps({"label": lb, "rate_over_rne": round(statistics.median(res[lb[:-3]]) / t, 3),
                          "rne_label": lb[:-3],
                          "rate_over_cast_scaled_sr": round((runs[lb][1] / t) / (runs[f"{p}:sr"][1] /
                                                                                 statistics.median(res[f"{p}:sr"])), 3),
                          "time_ratio_cast_scaled_sr_over_mx_sr": round(statistics.median(res[f"{p}:sr"]) / t, 3)}),
              flush=True)
