#!/usr/bin/env python3
"""The MX block-scaled DDP hook, step by step, against the one-scale fp8 hook and the plain bf16 hook on the same
bucket, on an in-process group, interleaved in one run.  ftar.ddp.mx_compress_hook's five steps -- (1) ftar_mx_scales,
(2) the scale bytes' AllReduce of u8 with op="max", (3) ftar_mx_quantize with the given scales, (4) the wire's
AllReduce with op="avg", (5) ftar_mx_dequantize -- are timed with a stream event between each (mode "mx-steps": the
hook's own calls, spelled out here with the events between them), and the whole hook (mode "mx") against
ftar.ddp.fp8_compress_hook ("fp8") and ftar.ddp.allreduce_hook with average="fused" ("bf16").  Every rank calls on
its own thread and stream with a stand-in bucket of --elems bf16 elements; a call's time is that of its slowest
rank, median over --rounds with the fastest and slowest round next to it; a step's time is the median over rounds of
its slowest rank.  The same on a --small-elems bucket shows the fixed cost of the five launches.
A ONE-GPU PROXY: all ranks share one device and one HBM and the "wire" is device copies, so no number from this
tool is an xGMI number -- on a node the wire's bytes cross links that are 10-20x slower than HBM while the three
casts stay local.  Nobody has measured this hook across GPUs.
--rounding stochastic runs the "mx" and "mx-steps" modes (and the fp8 hook) with stochastic rounding at the quantize;
--rounding both adds the mode "mx-sr" next to "mx", interleaved in the same run, and prints its ratio.
python tools/hook_mx.py [--ranks 8] [--elems 67108864] [--small-elems 2048] [--rounds 7] [--topo 8] [--fmt e4m3]
                        [--rounding nearest|stochastic|both]"""
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
ap.add_argument("--headroom", type=int, default=0)
ap.add_argument("--rounding", default="nearest", choices=("nearest", "stochastic", "both"))
a = ap.parse_args()
P = a.ranks
ROUNDING = "stochastic" if a.rounding == "stochastic" else "nearest"
MODES = ("mx", "mx-steps", "fp8", "bf16") + (("mx-sr",) if a.rounding == "both" else ())
STEPS = ("scales", "allreduce_u8_max", "quantize_given", "allreduce_f8_avg", "dequantize")


class Bucket:
    def __init__(self, t):
        self.t = t

    def buffer(self):
        return self.t


group = ftar.Comm.init_local(P)
streams = [torch.cuda.Stream() for _ in range(P)]
states = {"mx": [ftar.ddp.MxCompressState(group[r], fmt=a.fmt, topo=a.topo, headroom=a.headroom, rounding=ROUNDING)
                 for r in range(P)],
          "mx-sr": [ftar.ddp.MxCompressState(group[r], fmt=a.fmt, topo=a.topo, headroom=a.headroom,
                                             rounding="stochastic") for r in range(P)],
          "fp8": [ftar.ddp.Fp8CompressState(group[r], fmt=a.fmt, topo=a.topo, rounding=ROUNDING) for r in range(P)],
          "bf16": [ftar.ddp.HookState(group[r], topo=a.topo, average="fused") for r in range(P)]}
states["mx-steps"] = states["mx"]
hooks = {"mx": ftar.ddp.mx_compress_hook, "mx-sr": ftar.ddp.mx_compress_hook, "fp8": ftar.ddp.fp8_compress_hook, "bf16": ftar.ddp.allreduce_hook}


def mx_steps(state, t, stream):
    """mx_compress_hook's five calls with an event after each; returns the six events."""
    n, nb = t.numel(), ftar.mx_nblocks(t.numel())
    wire, scales = state._on(t.device, n)
    dt, f8 = ftar._dt(str(t.dtype)), ftar._dt(state.wire_dtype)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    ev[0].record()
    ftar.mx_scales(t, scales, n, dt, f8, headroom=state.headroom, stream=stream)
    ev[1].record()
    state.comm.allreduce(None, scales, nb, "u8", "max", topo_=state.topo, lonely=state.lonely, stream=stream)
    ev[2].record()
    if state.rounding == "stochastic":
        ftar.mx_quantize(t, wire, scales, n, dt, f8, mode="given", stream=stream, rounding="stochastic",
                         seed=state.seed, offset=state.offset)
        state.offset += n
    else:
        ftar.mx_quantize(t, wire, scales, n, dt, f8, mode="given", stream=stream)
    ev[3].record()
    state.comm.allreduce(None, wire, n, f8, "avg", topo_=state.topo, lonely=state.lonely, stream=stream)
    ev[4].record()
    ftar.mx_dequantize(wire, scales, t, n, f8, dt, stream=stream)
    ev[5].record()
    return ev


def measure(elems):
    src = [(torch.rand(elems, device="cuda") - 0.5).to(torch.bfloat16) for _ in range(P)]
    bufs = [torch.empty_like(x) for x in src]
    torch.cuda.synchronize()

    def one_call(mode):
        """every rank's hook once; returns each rank's stream-event milliseconds (mx-steps: the five steps')"""
        ms, errs = [None] * P, []
        for r in range(P):
            bufs[r].copy_(src[r])
        torch.cuda.synchronize()

        def rank(r):
            try:
                with torch.cuda.stream(streams[r]):
                    if mode == "mx-steps":
                        ev = mx_steps(states[mode][r], bufs[r], streams[r])
                        ev[-1].synchronize()
                        ms[r] = [ev[i].elapsed_time(ev[i + 1]) for i in range(5)]
                        return
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
    n = elems
    print(json.dumps({"ranks": P, "elems": n, "bucket_KiB": n * 2 / 2**10, "wire": a.fmt, "headroom": a.headroom,
                      "rounding": a.rounding,
                      "wire_bytes_per_rank": n + 2 * ftar.mx_nblocks(n), "bf16_bytes_per_rank": 2 * n,
                      "rounds": a.rounds, "last_exec": execs,
                      "note": "one-GPU proxy (in-process group): no xGMI number"}))
    med = {}
    for m, rounds in res.items():
        if m == "mx-steps":
            total = 0.0
            for i, step in enumerate(STEPS):
                worst = [max(rd[r][i] for r in range(P)) for rd in rounds]
                total += statistics.median(worst)
                print(json.dumps({"step": step, "ms_slowest_rank_med": round(statistics.median(worst), 4),
                                  "ms_slowest_rank_min": round(min(worst), 4),
                                  "ms_slowest_rank_max": round(max(worst), 4)}), flush=True)
            print(json.dumps({"steps_sum_ms": round(total, 4)}), flush=True)
            continue
        worst = [max(rd) for rd in rounds]    # the call ends when its slowest rank does
        med[m] = statistics.median(worst)
        print(json.dumps({"mode": m, "ms_slowest_rank_med": round(med[m], 4), "ms_slowest_rank_min": round(min(worst), 4),
                          "ms_slowest_rank_max": round(max(worst), 4)}), flush=True)
    if "mx-sr" in med:
        print(json.dumps({"mx-sr_vs": "mx", "ms_delta": round(med["mx-sr"] - med["mx"], 4),
                          "ratio": round(med["mx-sr"] / med["mx"], 4)}), flush=True)
    for other in ("fp8", "bf16"):
        print(json.dumps({"mx_vs": other, "ms_delta": round(med["mx"] - med[other], 4),
                          "ratio": round(med["mx"] / med[other], 4)}), flush=True)


measure(a.elems)
measure(a.small_elems)
group.destroy()
