#!/usr/bin/env python3
"""The DDP hook's two means on an in-process group: average="divide" (div_ by the world size, then op="sum")
against average="fused" (op="avg": the 1 / P inside the last fold of each block), interleaved in one run.
Every rank calls ftar.ddp.allreduce_hook on its own thread and stream with a stand-in bucket (an fp16 tensor
of --elems elements); the time is each rank's own stream-event time around its hook call (the division
included), median over --rounds, with the slowest and fastest round next to it.  The expected saving is the
div_ pass: 2 x bucket bytes of HBM traffic per rank.
python tools/hook_avg.py [--ranks 8] [--elems 67108864] [--rounds 7] [--topo 8]"""
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
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--topo", default=None, help="FT_TOPO syntax; default: the execution model's choice")
a = ap.parse_args()
P = a.ranks


class Bucket:
    def __init__(self, t):
        self.t = t

    def buffer(self):
        return self.t


group = ftar.Comm.init_local(P)
streams = [torch.cuda.Stream() for _ in range(P)]
src = [(torch.rand(a.elems, device="cuda") - 0.5).to(torch.float16) for _ in range(P)]
bufs = [torch.empty_like(x) for x in src]
states = {m: [ftar.ddp.HookState(group[r], topo=a.topo, average=m) for r in range(P)] for m in ("divide", "fused")}
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
                ftar.ddp.allreduce_hook(states[mode][r], Bucket(bufs[r])).wait()
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


res = {"divide": [], "fused": []}
for m in res:          # warm-up: buffers, plans, the model's choice
    one_call(m)
for _ in range(a.rounds):
    for m in res:
        res[m].append(one_call(m))
print(json.dumps({"ranks": P, "elems": a.elems, "bucket_MiB": a.elems * 2 / 2**20, "rounds": a.rounds,
                  "last_exec": group[0].last_exec()}))
for m, rounds in res.items():
    per_rank = [statistics.median(rd[r] for rd in rounds) for r in range(P)]
    worst = [max(rd) for rd in rounds]    # the call ends when its slowest rank does
    print(json.dumps({"average": m, "ms_per_rank_med": [round(x, 3) for x in per_rank],
                      "ms_slowest_rank_med": round(statistics.median(worst), 3),
                      "ms_slowest_rank_min": round(min(worst), 3), "ms_slowest_rank_max": round(max(worst), 3)}),
          flush=True)
d = statistics.median(max(rd) for rd in res["divide"])
f = statistics.median(max(rd) for rd in res["fused"])
print(json.dumps({"saved_ms": round(d - f, 3), "saved_share": round((d - f) / d, 4),
                  "div_pass_GBps_implied": round(2 * a.elems * 2 / ((d - f) * 1e-3) / 1e9, 1) if d > f else None}))
group.destroy()
