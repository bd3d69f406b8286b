#!/usr/bin/env python3
"""ftar_reduce (the production dispatch) by dtype and k on cold data: launches rotate over 4 disjoint
(k sources + destination) sets of 256 MiB buffers; GB/s of (k+1) x 256 MiB algorithmic bytes, median of
interleaved rounds, with the slowest and fastest round next to it (the run's own spread: the margin when
one (dtype, op) is judged against another of the same width).  --op takes a list; pairs the library
refuses (band on floats, max on bool) are skipped.  "scaled" is ftar_reduce_scaled (the sum times 1 / k before
its rounding: AVG's root fold), to be read against "sum" of the same dtype and k in the same run; "amax" is
ftar_reduce_amax with the same scale (the scaled fold plus the abs-max of what it stores: a 4-byte memset, the
kernel, one atomic per workgroup), to be read against "sum" and "scaled" of that run.  A dtype may
be named twice as "u8,u8#2": the same measurement under a label of its own, interleaved with the rest -- the
tool's own spread between two runs of one kernel, the margin for a comparison across dtypes (the fp8 folds
against the u8 SUM, the lightest fold of their element width; random bytes, so fp8 lanes hold NaN and inf too:
the instructions do not care).
python tools/dtype_rates.py [--ks 2,8] [--dtypes f32,bf16,f16,f64,i32,i16,u8,u8#2,f8e4m3,f8e5m2,bool]
                            [--op sum,max,min,scaled,amax]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "allreduce-over-mpi_amd"))
import torch  # noqa: E402
import ftar  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", default="2,8")
ap.add_argument("--dtypes", default="f32,bf16,f64,i64,i32,i16,u8,bool")
ap.add_argument("--op", default="sum", help="one op or a comma list: sum,band,max,min,scaled,amax")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=8)
a = ap.parse_args()
NB = 256 << 20
ks = [int(k) for k in a.ks.split(",")]
S = 4
bufs = [[torch.randint(0, 256, (NB,), dtype=torch.uint8, device="cuda") for _ in range(max(ks) + 1)] for _ in range(S)]
stream = torch.cuda.current_stream()
amax_word = torch.zeros(1, dtype=torch.float32, device="cuda")
res = {}
ops = a.op.split(",")
refused = set()
for _ in range(a.rounds):
    for label, op in ((d, op) for d in a.dtypes.split(",") for op in ops):
        d = label.split("#")[0]
        n = NB // ftar.dtype_size(d)
        for k in ks:
            def launch(i):
                s = bufs[i % S]
                if op == "scaled":
                    ftar.reduce(s[:k], s[max(ks)], n, d, "sum", stream=stream, scale=1.0 / k)
                elif op == "amax":
                    ftar.reduce(s[:k], s[max(ks)], n, d, "sum", stream=stream, scale=1.0 / k, amax=amax_word)
                else:
                    ftar.reduce(s[:k], s[max(ks)], n, d, op, stream=stream)
            if (label, op) in refused:
                continue
            try:
                for i in range(S):
                    launch(i)
            except ftar.FtarError as e:
                if e.status != 2:   # "unsupported": not a pair of this library
                    raise
                refused.add((label, op))
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(a.reps):
                launch(i)
            e1.record(stream)
            torch.cuda.synchronize()
            res.setdefault((label, op, k), []).append(e0.elapsed_time(e1) / a.reps)
for (d, op, k), ts in res.items():
    med = statistics.median(ts)

    def rate(ms):
        return round((k + 1) * NB / ms / 1e6, 1)
    print(json.dumps({"dtype": d, "op": op, "k": k, "ms_med": round(med, 4), "GBps_med": rate(med),
                      "GBps_slowest": rate(max(ts)), "GBps_fastest": rate(min(ts))}), flush=True)
