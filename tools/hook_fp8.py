#!/usr/bin/env python3
"""The fp8-compressed DDP hook against the fused-mean hook on the same bf16 bucket, on an in-process group,
interleaved in one run: ftar.ddp.fp8_compress_hook (quantize with ftar_cast_scaled, the AllReduce with op="avg" and
amax on an fp8 wire of half the bytes, dequantize) against ftar.ddp.allreduce_hook with average="fused" (the bf16
AllReduce with op="avg") and against that hook with track_amax=True (the like-for-like: both then return the
overflow flag).  Every rank calls its hook on its own thread and stream with a stand-in bucket of --elems bf16
elements; the time is each rank's own stream-event time around the hook call, the call's time that of its slowest
rank, median over --rounds with the fastest and slowest round next to it.  The same on a --small-elems bucket shows
the fixed cost of the two extra launches.  A ONE-GPU PROXY: all ranks share one device and one HBM, the "wire" is
device copies, so no number from this tool is an xGMI number -- on a node the wire's halved bytes cross links that
are 10-20x slower than HBM, while the two casts stay local.
python tools/hook_fp8.py [--ranks 8] [--elems 67108864] [--small-elems 2048] [--rounds 7] [--topo 8] [--fmt e4m3]"""
import argparse
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "allreduce-over-mpi_amd"))
import torch  # noqa: E402
import ftar  # noqa: E402
import ftar.ddp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ranks", type=int, default=8)
ap.add_argument("--elems", type=int, default=64 << 20)
ap.add_argument("--small-elems", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--topo", default=None, help="FT_TOPO syntax; default: the execution model's choice")
ap.add_argument("--fmt", default="e4m3")
a = ap.parse_args()
P = a.ranks
MODES = ("fp8", "fused", "fused+amax")


class Bucket:
    def __init__(self, t):
        self.t = t

    def buffer(self):
        return self.t


group = ftar.Comm.init_local(P)
streams = [torch.cuda.Stream() for _ in range(P)]
states = {"fp8": [ftar.ddp.Fp8CompressState(group[r], fmt=a.fmt, topo=a.topo) for r in range(P)],
          "fused": [ftar.ddp.HookState(group[r], topo=a.topo, average="fused") for r in range(P)],
          "fused+amax": [ftar.ddp.HookState(group[r], topo=a.topo, average="fused", track_amax=True) for r in range(P)]}
hooks = {"fp8": ftar.ddp.fp8_compress_hook, "fused": ftar.ddp.allreduce_hook, "fused+amax": ftar.ddp.allreduce_hook}


def measure(elems):
    src = [(torch.rand(elems, device="cuda") - 0.5).to(torch.bfloat16) for _ in range(P)]
    bufs = [torch.empty_like(x) for x in src]
    torch.cuda.synchronize()

    def one_call(mode):
        """every rank's hook once; returns each rank's stream-event milliseconds"""
        ms, errs = [0.0] * P, []
        for r in range(P):
            bufs[r].copy_(src[r])
        torch.cuda.synchronize()

        def rank(r):
            try:
                with torch.cuda.stream(streams[r]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    hooks[mode](states[mode][r], Bucket(bufs[r])).wait()
                    e1.record()
                    e1.synchronize()
                    ms[r] = e0.elapsed_time(e1)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        if errs:
            raise errs[0]
        return ms

    res = {m: [] for m in MODES}
    execs = {}
    for m in res:          # warm-up: buffers, plans, the model's choice
        one_call(m)
        execs[m] = group[0].last_exec()
    for _ in range(a.rounds):
        for m in res:
            res[m].append(one_call(m))
    print(json.dumps({"ranks": P, "elems": elems, "bucket_KiB": elems * 2 / 2**10, "wire": a.fmt, "rounds": a.rounds,
                      "last_exec": execs, "note": "one-GPU proxy (in-process group): no xGMI number"}))
    med = {}
    for m, rounds in res.items():
        worst = [max(rd) for rd in rounds]    # the call ends when its slowest rank does
        med[m] = statistics.median(worst)
        print(json.dumps({"mode": m, "ms_slowest_rank_med": round(med[m], 4), "ms_slowest_rank_min": round(min(worst), 4),
                          "ms_slowest_rank_max": round(max(worst), 4)}), flush=True)
    for other in ("fused", "fused+amax"):
        print(json.dumps({"fp8_vs": other, "ms_delta": round(med["fp8"] - med[other], 4),
                          "ratio": round(med["fp8"] / med[other], 4)}), flush=True)


measure(a.elems)
measure(a.small_elems)
group.destroy()
