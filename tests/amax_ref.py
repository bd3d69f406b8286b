"""Independent CPU expectation for the amax entry points (include/ftar.h: ftar_reduce_amax, ftar_allreduce_amax):
the abs-max of an expected result, from its bit patterns alone.

amax_bits(dt, bits) takes the largest |encoding| as an unsigned integer in numpy -- in all five formats that order
is the order of |value|, and every NaN encoding sorts above every number -- and widens the one winner to fp32 bits
through torch's exact cast.  Any NaN element gives NAN ("is a NaN": which one is unspecified).

The results themselves come from the folds the suite already pins (avg_ref.root_fold / nested / ring / tree,
f8_ref.fold / nested / ring / tree) on FINITE inputs (kernel_edges.sources, f8_ref.finite_sources) with one
negative PEAK planted at a known position of one source, zeros in that lane of the others: checked() asserts that
the expectation is finite and that its largest |value| is strictly above the runner-up and sits at the peak, so a
kernel or an engine path that misses that position returns a different word.  Arrays travel as unsigned bit
patterns; results are cached and shared, so callers must not modify what these functions return."""
import functools

import numpy as np

import avg_ref
import f16_minmax_ref as ref
import f8_ref

DTYPES = ["f16", "bf16", "f32", "f8e4m3", "f8e5m2"]
NAN = "nan"
# (storage, |encoding| mask, the first encoding that is no finite number: inf, or e4m3's NaN)
LAYOUT = {"f16": (np.uint16, 0x7FFF, 0x7C00), "bf16": (np.uint16, 0x7FFF, 0x7F80),
          "f32": (np.uint32, 0x7FFFFFFF, 0x7F800000), "f8e4m3": (np.uint8, 0x7F, 0x7F), "f8e5m2": (np.uint8, 0x7F, 0x7C)}
PEAK = {"f16": -1024.0, "bf16": -1024.0, "f32": -1024.0, "f8e4m3": -64.0, "f8e5m2": -64.0}


def is_f8(dt):
    return dt in f8_ref.FORMATS


def storage(dt):
    return LAYOUT[dt][0]


def elems_per_vector(dt):
    return 16 // np.dtype(storage(dt)).itemsize


def keys(dt, bits):
    """|encoding| of every element, as unsigned integers."""
    u, mask, _ = LAYOUT[dt]
    return np.ascontiguousarray(bits).view(u) & u(mask)


def nan_mask(dt, bits):
    return f8_ref.nan_mask(dt, bits) if is_f8(dt) else ref.nan_mask(dt, np.ascontiguousarray(bits).view(storage(dt)))


def widen(dt, enc):
    """The fp32 bit pattern of one encoding (an int), through torch's exact cast."""
    import torch
    if is_f8(dt):
        t = f8_ref._t(dt, np.array([enc], np.uint8))
    else:
        t = avg_ref._t(dt, np.array([enc], storage(dt)))
    return int(t.to(torch.float32).view(torch.int32).numpy().view(np.uint32)[0])


def amax_bits(dt, bits):
    """The word an amax call must leave for a result with these bit patterns: fp32 bits as an int, or NAN."""
    bits = np.ascontiguousarray(bits).view(storage(dt))
    if bits.size == 0:
        return 0
    if nan_mask(dt, bits).any():
        return NAN
    return widen(dt, int(keys(dt, bits).max()))


def matches(got, want):
    """got: the uint32 the call left; want: amax_bits()."""
    got = int(got)
    if want == NAN:
        return (got & 0x7FFFFFFF) > 0x7F800000
    return got == want


def encode(dt, value):
    """One exactly representable value as an encoding of dt."""
    if is_f8(dt):
        return int(f8_ref.encode(dt, [value])[0])
    return int(ref.encode(dt, np.array([value]))[0])


def checked(dt, want, p):
    """Asserts the conditions every non-special case relies on, and returns amax_bits(want): the expectation is
    finite, and its largest |value| sits at p, strictly above the runner-up."""
    k = keys(dt, want).astype(np.uint64)
    assert not nan_mask(dt, want).any() and int(k.max()) < LAYOUT[dt][2], "the expectation is finite"
    rest = np.delete(k, p)
    assert rest.size == 0 or int(k[p]) > int(rest.max()), ("the peak wins strictly", p, int(k[p]), int(rest.max()))
    return amax_bits(dt, want)


def base_sources(dt, k, n, seed=1):
    """k finite sources: |x| < 1 for the 16- and 32-bit floats, |x| < 2 for fp8 (k <= 17)."""
    import kernel_edges
    if is_f8(dt):
        return [x.copy() for x in f8_ref.finite_sources(dt, max(k, 2), n, seed)[:k]]
    return [np.ascontiguousarray(x).view(storage(dt)).copy() for x in kernel_edges.sources(dt, "sum", k, n, seed)]


def plant(dt, xs, p, src, value=None):
    """The peak (or `value`) at position p of source src, +0 in that lane of the others; returns xs."""
    for x in xs:
        x[p] = 0
    xs[src][p] = encode(dt, PEAK[dt] if value is None else value)
    return xs


def fold(dt, ins, scale, shape=None):
    """What ftar_reduce_amax stores: the (nested) fold with its root times scale, rounded once."""
    if is_f8(dt):
        r = f8_ref.scale_of(scale)
        return f8_ref.nested(dt, ins, shape, r) if shape and len(ins) > 1 else f8_ref.fold(dt, ins, r)
    r = avg_ref.scale_of(dt, scale)
    return avg_ref.nested(dt, ins, shape, r) if shape and len(ins) > 1 else avg_ref.root_fold(dt, ins, r)


@functools.lru_cache(maxsize=None)
def reduce_case(dt, k, n, scale, p, shape=None, src=None, seed=1):
    """(sources, expected result, expected amax word) of one ftar_reduce_amax case with the peak at p."""
    p = p % n
    ins = plant(dt, base_sources(dt, k, n, seed), p, (k // 2) if src is None else src)
    want = fold(dt, ins, scale, shape)
    return ins, want, checked(dt, want, p)


def ring(dt, ins, r):
    """avg_ref.ring's schedule with the root's r passed in (avg_ref's own takes 1 / P): block b is x_b, then
    + x_{b+j} for j = 1 .. P-1, every hop one avg_ref.sum_fold of two, the last one avg_ref.root_fold with r.
    r = 1 is an exact multiply: SUM's bits.  tests/test_amax_api.py holds it against avg_ref.ring at r = 1 / P."""
    P, n = len(ins), ins[0].size
    out = np.empty(n, storage(dt))
    for b, lo, hi in ref._blocks(n, P):
        acc = ins[b][lo:hi]
        for j in range(1, P):
            pair = [acc, ins[(b + j) % P][lo:hi]]
            acc = avg_ref.root_fold(dt, pair, r) if j == P - 1 else avg_ref.sum_fold(dt, pair)
        out[lo:hi] = acc
    return out


def tree(dt, ins, widths, r):
    """avg_ref.tree's schedule with the root's r passed in: at every stage rank q folds its own value first, then
    its stage group's in ascending rank order, one avg_ref.sum_fold per node; block b's node of the last stage
    on rank b is the root, one avg_ref.root_fold with r."""
    P, n = len(ins), ins[0].size
    assert int(np.prod(widths)) == P
    out = np.empty(n, storage(dt))
    for b, lo, hi in ref._blocks(n, P):
        vals = {q: ins[q][lo:hi] for q in range(P)}
        g = 1
        for si, w in enumerate(widths):
            new = {}
            for q in range(P):
                left = q // (g * w) * g * w + q % g
                node = [vals[q]] + [vals[left + j * g] for j in range(w) if left + j * g != q]
                root = si == len(widths) - 1 and q == b
                new[q] = avg_ref.root_fold(dt, node, r) if root else avg_ref.sum_fold(dt, node)
            vals = new
            g *= w
        out[lo:hi] = vals[b]
    return out


def schedule(dt, ins, topo, op):
    """The array every rank ends with after a SUM / AVG AllReduce on topo ("1" = ring; no lonely ranks)."""
    widths = [int(w) for w in topo.split(",")]
    P = len(ins)
    if is_f8(dt):
        r = f8_ref.recip(P) if op == "avg" else None
        return f8_ref.ring(dt, ins, r) if 1 in widths else f8_ref.tree(dt, ins, widths, r)
    r = avg_ref.recip(dt, P) if op == "avg" else avg_ref.scale_of(dt, 1.0)
    return ring(dt, ins, r) if 1 in widths else tree(dt, ins, widths, r)


def block_edges(n, P, b):
    """(first, last) element of block b."""
    lo, hi = [(lo, hi) for bb, lo, hi in ref._blocks(n, P) if bb == b][0]
    return lo, hi - 1


@functools.lru_cache(maxsize=None)
def allreduce_case(dt, P, topo, n, op, p, seed=1):
    """(per-rank sources, the array every rank ends with, the amax word) with the peak in rank P // 2's input."""
    ins = plant(dt, base_sources(dt, P, n, seed), p, P // 2)
    want = schedule(dt, ins, topo, op)
    return ins, want, checked(dt, want, p)


@functools.lru_cache(maxsize=None)
def exact_case(dt, P, n, op, p, seed=1):
    """Integer-valued sources (exact for any association: the lonely layouts) plus the peak at p of rank P // 2."""
    if op == "avg":
        ins, want = avg_ref.exact_case(dt, P, n, seed)
        scale = P
    else:
        ins = ref.sources(dt, P, n, seed, small_ints=True)     # integers in [-8, 8]: any association is exact
        want = ref.encode(dt, sum(avg_ref._t(dt, x).double() for x in ins).numpy())
        scale = 1
    ins = plant(dt, [np.array(x).copy() for x in ins], p, P // 2, PEAK[dt] * scale)
    want = np.array(want).copy()
    want[p] = encode(dt, PEAK[dt])
    return ins, want, checked(dt, want, p)
