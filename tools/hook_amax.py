#!/usr/bin/env python3
"""The DDP hook's overflow check on an in-process group, three ways, interleaved in one run: the hook with
track_amax=True (ftar_allreduce_amax: the abs-max comes out of the last fold of each block, then a second,
tiny AllReduce of one word per rank), against today's hook followed by torch.isfinite(t).all(), and against
today's hook followed by t.abs().max() -- the pass over the reduced bucket that GradScaler-style checks and
delayed fp8 scaling make.  Every rank calls ftar.ddp.allreduce_hook on its own thread and stream with a stand-in
bucket (an fp16 tensor of --elems elements); the time is each rank's own stream-event time around the hook call
and the check after it, median over --rounds, with the slowest and fastest round next to it.  The expected
saving is one read of the bucket per rank.  The same three ways on a --small-elems bucket (4 KiB) show the fixed
cost of the second internal round.  A one-GPU proxy: all ranks share one device, so no number here is an xGMI one.
python tools/hook_amax.py [--ranks 8] [--elems 67108864] [--small-elems 2048] [--rounds 7] [--topo 8]"""
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
a = ap.parse_args()
P = a.ranks
MODES = ("amax", "isfinite", "absmax", "plain")     # plain: today's hook alone (the floor)


class Bucket:
    def __init__(self, t):
        self.t = t

    def buffer(self):
        return self.t


group = ftar.Comm.init_local(P)
streams = [torch.cuda.Stream() for _ in range(P)]
states = {m: [ftar.ddp.HookState(group[r], topo=a.topo, track_amax=(m == "amax")) for r in range(P)] for m in MODES}


def measure(elems):
    src = [(torch.rand(elems, device="cuda") - 0.5).to(torch.float16) for _ in range(P)]
    bufs = [torch.empty_like(x) for x in src]
    flags = [None] * P
    torch.cuda.synchronize()

    def one_call(mode):
        """every rank's hook (and check) once; returns each rank's stream-event milliseconds"""
        ms, errs = [0.0] * P, []
        for r in range(P):
            bufs[r].copy_(src[r])
        torch.cuda.synchronize()

        def rank(r):
            try:
                with torch.cuda.stream(streams[r]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    t = ftar.ddp.allreduce_hook(states[mode][r], Bucket(bufs[r])).wait()
                    if mode == "amax":
                        flags[r] = states[mode][r].found_inf()
                    elif mode == "isfinite":
                        flags[r] = torch.isfinite(t).all()
                    elif mode == "absmax":
                        flags[r] = t.abs().max()
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
    for m in res:          # warm-up: buffers, plans, the model's choice
        one_call(m)
    for _ in range(a.rounds):
        for m in res:
            res[m].append(one_call(m))
    print(json.dumps({"ranks": P, "elems": elems, "bucket_KiB": elems * 2 / 2**10, "rounds": a.rounds,
                      "last_exec": group[0].last_exec(), "note": "one-GPU proxy (in-process group)"}))
    med = {}
    for m, rounds in res.items():
        worst = [max(rd) for rd in rounds]    # the call ends when its slowest rank does
        med[m] = statistics.median(worst)
        print(json.dumps({"mode": m, "ms_slowest_rank_med": round(med[m], 4), "ms_slowest_rank_min": round(min(worst), 4),
                          "ms_slowest_rank_max": round(max(worst), 4)}), flush=True)
    for other in ("isfinite", "absmax"):
        d = med[other] - med["amax"]
        print(json.dumps({"amax_vs": other, "saved_ms": round(d, 4), "saved_share": round(d / med[other], 4),
                          "read_pass_GBps_implied": round(elems * 2 / (d * 1e-3) / 1e9, 1) if d > 0 else None}))
    print(json.dumps({"amax_over_plain_ms": round(med["amax"] - med["plain"], 4)}), flush=True)


measure(a.elems)
measure(a.small_elems)
group.destroy()
