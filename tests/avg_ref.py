"""Independent CPU expectation for FTAR_AVG and ftar_reduce_scaled (include/ftar.h): PyTorch on the
CPU, the folds written out per schedule as tests/f16_minmax_ref.py writes the fp16 sums, parameterised by the
float format (f16, bf16, f32, f64).

Every node or hop is fp32 adds (f64: f64 adds), left to right, and `.to(dtype)` -- except the root fold of each
block, the one reduce that produces the block's final value, which finishes as

    (acc * r).to(dtype)        r = np.float32(1) / np.float32(P)   (f64: 1.0 / P)

one multiply by the reciprocal in the accumulator's precision, then the fold's single rounding.  Inputs are
f16_minmax_ref.sources() and every comparison goes through f16_minmax_ref.same_bits(), which also holds the
expectation's NaN-lane share under NAN_SHARE_CAP.  Arrays travel as unsigned bit patterns; results are cached
and shared between tests, so callers must not modify what these functions return."""
import functools

import numpy as np

import f16_minmax_ref as ref

FLOAT_DTYPES = ["f16", "bf16", "f32", "f64"]


def _fmt(dt):
    """(torch dtype of the format, same-width signed integer, accumulator dtype)"""
    import torch
    return {"f16": (torch.float16, torch.int16, torch.float32), "bf16": (torch.bfloat16, torch.int16, torch.float32),
            "f32": (torch.float32, torch.int32, torch.float32), "f64": (torch.float64, torch.int64, torch.float64)}[dt]


def _t(dt, bits):
    import torch
    f, i, _ = _fmt(dt)
    a = np.ascontiguousarray(bits).view(ref.storage(dt))
    return torch.from_numpy(a.view(a.dtype.str.replace("u", "i")).copy()).view(f)


def _bits(dt, t):
    _, i, _ = _fmt(dt)
    return t.contiguous().view(i).numpy().view(ref.storage(dt))


def recip(dt, P):
    """r as the kernels hold it: 1.0f / (float)P, a double for f64 (a 0-dim tensor of the accumulator's type)."""
    import torch
    if dt == "f64":
        return torch.tensor(np.float64(1) / np.float64(P), dtype=torch.float64)
    return torch.tensor(np.float32(1) / np.float32(P), dtype=torch.float32)


def scale_of(dt, s):
    """A caller's scale as ftar_reduce_scaled applies it: cast to float unless the dtype is f64."""
    import torch
    if dt == "f64":
        return torch.tensor(np.float64(s), dtype=torch.float64)
    return torch.tensor(np.float32(s), dtype=torch.float32)


def _acc(dt, ins):
    """The fold's accumulator before any rounding: adds in the accumulator's type, left to right."""
    a = _fmt(dt)[2]
    acc = _t(dt, ins[0]).to(a)
    for x in ins[1:]:
        acc = acc + _t(dt, x).to(a)
    return acc


def sum_fold(dt, ins):
    """A SUM node: one rounding."""
    return _bits(dt, _acc(dt, ins).to(_fmt(dt)[0]))


def root_fold(dt, ins, r):
    """The root: the accumulator times r (a 0-dim tensor of the accumulator's type), then the one rounding."""
    acc = _acc(dt, ins)
    assert r.dtype == acc.dtype and r.dim() == 0
    return _bits(dt, (acc * r).to(_fmt(dt)[0]))


def nested(dt, ins, shape, r):
    """ftar_reduce_scaled with a shape: inner nodes are SUM nodes (rounded), the root is scaled, then rounded."""
    vals = list(ins)
    levels = [w for w in shape if w > 1]
    for li, w in enumerate(levels):
        last = li == len(levels) - 1
        vals = [root_fold(dt, vals[i:i + w], r) if last else sum_fold(dt, vals[i:i + w])
                for i in range(0, len(vals), w)]
    assert len(vals) == 1
    return vals[0]


@functools.lru_cache(maxsize=None)
def reduce_case(dt, k, n, scale, shape=None, seed=1):
    """(sources, expectation) of one ftar_reduce_scaled case."""
    ins = ref.sources(dt, max(k, 2), n, seed)[:k]     # (sources() plants its fp16 ties in two sources)
    r = scale_of(dt, scale)
    return ins, (nested(dt, ins, shape, r) if shape else root_fold(dt, ins, r))


# ---- AllReduce, per schedule ------------------------------------------------------------------------------
def ring(dt, ins):
    """The ring: block b is x_b, then + x_{b+j} for j = 1 .. P-1, one rounding per hop; the last hop is the
    root: ((acc + x) * r) rounded once."""
    f, _, a = _fmt(dt)
    P, n = len(ins), ins[0].size
    r = recip(dt, P)
    out = np.empty(n, ref.storage(dt))
    for b, lo, hi in ref._blocks(n, P):
        acc = _t(dt, ins[b][lo:hi])
        for j in range(1, P):
            s = acc.to(a) + _t(dt, ins[(b + j) % P][lo:hi]).to(a)
            acc = (s * r).to(f) if j == P - 1 else s.to(f)
        out[lo:hi] = _bits(dt, acc)
    return out


def tree(dt, ins, widths):
    """Trees without lonely ranks, as f16_minmax_ref.f16_tree: one rounding per node, own value first, then the
    stage group in ascending rank order; block b's node of the last stage on rank b is the root."""
    f, _, a = _fmt(dt)
    P, n = len(ins), ins[0].size
    assert int(np.prod(widths)) == P
    r = recip(dt, P)
    out = np.empty(n, ref.storage(dt))
    for b, lo, hi in ref._blocks(n, P):
        vals = {q: _t(dt, ins[q][lo:hi]) for q in range(P)}
        g = 1
        for si, w in enumerate(widths):
            new = {}
            for q in range(P):
                left = q // (g * w) * g * w + q % g
                acc = vals[q].to(a)
                for j in range(w):
                    p = left + j * g
                    if p != q:
                        acc = acc + vals[p].to(a)
                new[q] = (acc * r).to(f) if si == len(widths) - 1 and q == b else acc.to(f)
            vals = new
            g *= w
        out[lo:hi] = _bits(dt, vals[b])
    return out


@functools.lru_cache(maxsize=None)
def allreduce_case(dt, P, topo, n, seed=1):
    """(per-rank sources, the array every rank must end with) of an AVG AllReduce; topo "1" = ring."""
    ins = ref.sources(dt, P, n, seed)
    widths = [int(w) for w in topo.split(",")]
    return ins, (ring(dt, ins) if 1 in widths else tree(dt, ins, widths))


@functools.lru_cache(maxsize=None)
def exact_case(dt, P, n, seed=1):
    """Integer-valued sources in [-8, 8] times P and their mean, the plain integer sum of the [-8, 8] values:
    every partial sum is a multiple of P below 2^8 multiples, exact in every format, and (P S) * fl(1 / P)
    rounds to S, so the mean is exact for any association (the lonely layouts, whose fold order this helper
    does not restate)."""
    import torch
    small = ref.sources(dt, P, n, seed, small_ints=True)
    vals = [_t(dt, x).double() for x in small]
    ins = tuple(ref.encode(dt, (v * P).numpy()) for v in vals)
    tot = sum(vals)
    assert float(tot.abs().max()) <= 8 * P
    want = ref.encode(dt, tot.numpy())
    a = _fmt(dt)[2]
    assert np.array_equal(_bits(dt, ((tot * P).to(a) * recip(dt, P)).to(_fmt(dt)[0])), want)
    return ins, want
