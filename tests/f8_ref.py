"""Independent CPU expectations for the two OCP fp8 dtypes, f8e4m3 (torch.float8_e4m3fn) and f8e5m2
(torch.float8_e5m2): include/ftar.h, DESIGN §7.  Nothing here calls the library.

  * SUM: PyTorch on the CPU, `.float()` adds and `.to(torch.float8_*)`, written out as the fold each schedule
    performs, as tests/f16_minmax_ref.py writes the fp16 sums: the flat fold (one rounding), the ring (one
    rounding per hop), the trees and the nested fold (one rounding per node).  With r given, the root fold of
    each block finishes as (acc * r).to(fp8), as tests/avg_ref.py writes AVG and ftar_reduce_scaled.
  * The rounding itself once more in integer arithmetic (rne_bits): RNE on the encoding, the mantissa carry
    running into the next encoding, no saturation -- e5m2 overflows to inf, e4m3 to NaN.  tests/test_f8_api.py
    holds it against torch's cast on every tie and its neighbours; it is the specification of the kernels'
    narrowing (ftar_debug_f8_cvt_check checks the same function on the GPU over all 2^32 floats).
  * MAX / MIN: monotone unsigned keys on the bytes (negatives: all bits flipped; non-negatives: the sign bit
    set), reduced as unsigned integers and mapped back; NaN lanes (e4m3: |b| == 0x7f, e5m2: |b| > 0x7c) flagged
    apart.  IEEE 754-2019 maximum / minimum without trusting any library's max.

Inputs (sources()): random bytes with bit 6 cleared, so |x| < 2, no NaN or inf in the bulk, and a 64-way sum
stays finite; lane 0 is ordinary; specials are planted at coprime strides in different sources.  Every
comparison goes through same_bits(), which also asserts that the expectation's NaN-lane share stays below
NAN_SHARE_CAP.  Arrays travel as uint8 bit patterns; results are cached and shared between tests, so callers
must not modify what these functions return."""
import functools

import numpy as np

from f16_minmax_ref import _blocks

ID = {"f8e4m3": 12, "f8e5m2": 13}
FORMATS = ("f8e4m3", "f8e5m2")
# (mantissa bits, exponent bias, the encoding right above the largest finite one: e4m3's NaN, e5m2's inf)
LAYOUT = {"f8e4m3": (3, 7, 0x7F), "f8e5m2": (2, 15, 0x7C)}
MAX_FINITE = {"f8e4m3": 0x7E, "f8e5m2": 0x7B}      # 448, 57344
ONE = {"f8e4m3": 0x38, "f8e5m2": 0x3C}
# RNE ties of a two-source sum (the other sources +0): (a, b, round(a + b)) as encodings
#   e4m3: 16 + 1 = 17 -> 16 (even mantissa), 18 + 1 = 19 -> 20;  e5m2: 8 + 1 = 9 -> 8, 10 + 1 = 11 -> 12
TIES = {"f8e4m3": ((0x58, 0x38, 0x58), (0x59, 0x38, 0x5A)), "f8e5m2": ((0x48, 0x3C, 0x48), (0x49, 0x3C, 0x4A))}
NAN_SHARE_CAP = 0.05
SIGN = 0x80


def torch_dtype(dt):
    import torch
    return {"f8e4m3": torch.float8_e4m3fn, "f8e5m2": torch.float8_e5m2}[dt]


def _t(dt, bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint8).copy()).view(torch_dtype(dt))


def _bits(t):
    import torch
    return t.contiguous().view(torch.uint8).numpy()


def nan_mask(dt, bits):
    a = np.asarray(bits, dtype=np.uint8) & np.uint8(0x7F)
    return a == 0x7F if dt == "f8e4m3" else a > 0x7C


# ---- the rounding, in integers --------------------------------------------------------------------------
def rne_bits(dt, u):
    """float32 bit patterns (uint32 array) -> fp8 encodings: RNE on the encoding, no saturation."""
    mb, bias, over = LAYOUT[dt]
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    sign = (u >> 24) & 0x80
    a = u & 0x7FFFFFFF
    sh = 23 - mb
    # normal results: rebias the exponent, round the dropped bits to nearest even, let the carry run
    r = a - np.minimum(a, (127 - bias) << 23)
    q = (r + ((1 << (sh - 1)) - 1) + ((r >> sh) & 1)) >> sh
    normal = np.minimum(q, over)
    # subnormal results: value = m x 2^(e - 150) in units of the smallest subnormal 2^(1 - bias - mb)
    e = a >> 23
    m = (a & 0x7FFFFF) | 0x800000
    shift = np.clip((151 - bias - mb) - e.astype(np.int64), 1, 26).astype(np.uint64)
    h = m >> shift
    rem = m & ((np.uint64(1) << shift) - 1)
    half = np.uint64(1) << (shift - 1)
    sub = h + ((rem > half) | ((rem == half) & ((h & 1) == 1)))
    sub = np.where(e == 0, 0, sub)
    out = np.where(a >= ((127 - bias + 1) << 23), normal, sub)
    out = np.where(a >= 0x7F800000, over, out)           # inf: the format's overflow
    out = np.where(a > 0x7F800000, 0x7F, out)            # NaN
    return (sign | out).astype(np.uint8)


# ---- inputs ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sources(dt, k, n, seed=1, small_ints=False):
    """k sources of n fp8 elements (a tuple of uint8 arrays).  small_ints: integer values in [-2, 2] instead,
    whose sum over up to 8 sources is exact for any association -- e4m3 holds every integer up to 16; e5m2
    (three significant bits) holds every EVEN integer up to 16, so its values are drawn from {-2, 0, 2}."""
    rng = np.random.default_rng([seed, ID[dt], k, n])
    if small_ints:
        vals = rng.integers(-2, 3, size=(k, n)) if dt == "f8e4m3" else 2 * rng.integers(-1, 2, size=(k, n))
        return tuple(encode(dt, v.astype(np.float32)) for v in vals)
    xs = [rng.integers(0, 256, size=n, dtype=np.uint8) & np.uint8(0xBF) for _ in range(k)]   # bit 6 cleared
    xs[0][31::97] = 0x7F                                    # a NaN (in both formats)
    if dt == "f8e5m2":
        xs[k - 1][3::89] = 0x7C                             # +inf
        xs[k // 2][5::83] = 0xFC                            # -inf
    for j in range(k):                                      # lanes where every source is a zero:
        xs[j][11::101] = SIGN if j % 2 == 0 else 0          #   -0 first, +0 and -0 facing each other
        xs[j][12::101] = 0 if j % 2 == 0 else SIGN          #   +0 first
        xs[j][17::103] = 1 + j                              # encodings 1 .. k: 1 .. k ulp of the subnormals
        xs[j][18::103] = SIGN | (1 + j)                     #   (and on into the first normals), both signs
    xs[k - 1][13::79] = 1                                   # the smallest subnormal among ordinary values
    for j in range(k):                                      # SUM: two ties and an overflow, the rest +0
        for off in (19, 20, 21):
            xs[j][off::107] = 0
    if k >= 2:
        (a0, b0, _), (a1, b1, _) = TIES[dt]
        xs[0][19::107], xs[1][19::107] = a0, b0
        xs[0][20::107], xs[1][20::107] = a1, b1
        xs[0][21::107] = xs[1][21::107] = MAX_FINITE[dt]    # max + max: NaN for e4m3, +inf for e5m2
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def finite_sources(dt, k, n, seed=1):
    """sources() without the NaN, the infs and the overflow lane (the bulk, the zero lanes, the subnormal lanes
    and the ties), for k <= 17: every fold of them is finite, so a result can be compared byte for byte."""
    assert 2 <= k <= 17
    rng = np.random.default_rng([seed, 100 + ID[dt], k, n])
    xs = [rng.integers(0, 256, size=n, dtype=np.uint8) & np.uint8(0xBF) for _ in range(k)]
    (a0, b0, _), (a1, b1, _) = TIES[dt]
    for j in range(k):
        xs[j][11::101] = SIGN if j % 2 == 0 else 0
        xs[j][12::101] = 0 if j % 2 == 0 else SIGN
        xs[j][17::103] = 1 + j
        xs[j][18::103] = SIGN | (1 + j)
        xs[j][19::107] = (a0, b0)[j] if j < 2 else 0
        xs[j][20::107] = (a1, b1)[j] if j < 2 else 0
    return tuple(xs)


def encode(dt, values):
    """Exactly representable values -> fp8 encodings (torch does the conversion)."""
    import torch
    return _bits(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(torch_dtype(dt)))


# ---- comparing ------------------------------------------------------------------------------------------
def same_bits(dt, got, want):
    """got == want bit for bit; NaN lanes compare as NaN or not.  Asserts the NaN-share cap."""
    got, want = np.asarray(got).view(np.uint8), np.asarray(want).view(np.uint8)
    if got.shape != want.shape:
        return False
    ng, nw = nan_mask(dt, got), nan_mask(dt, want)
    share = float(nw.mean()) if nw.size else 0.0
    assert share < NAN_SHARE_CAP, f"the expectation is {share:.1%} NaN lanes: the inputs hide failures"
    return bool(np.array_equal(ng, nw) and np.array_equal(got[~nw], want[~nw]))


def first_diff(dt, got, want):
    """For assertion messages: (lane, got, expected, how many lanes differ) of the first mismatch, or None."""
    got, want = np.asarray(got).view(np.uint8), np.asarray(want).view(np.uint8)
    ng, nw = nan_mask(dt, got), nan_mask(dt, want)
    i = np.flatnonzero((ng != nw) | (~nw & (got != want)))
    return None if not i.size else (int(i[0]), hex(int(got[i[0]])), hex(int(want[i[0]])), int(i.size))


# ---- MAX / MIN ------------------------------------------------------------------------------------------
def keys(bits):
    """key(x) < key(y) exactly when x < y in -inf < ... < -0 < +0 < ... < +inf (NaNs: the caller's)."""
    b = np.asarray(bits, dtype=np.uint8)
    return np.where(b & SIGN, ~b, b | SIGN).astype(np.uint8)


def keys_to_bits(k):
    k = np.asarray(k, dtype=np.uint8)
    return np.where(k & SIGN, k ^ SIGN, ~k).astype(np.uint8)


def minmax(dt, op, ins):
    f = np.maximum if op == "max" else np.minimum
    out = keys_to_bits(f.reduce([keys(x) for x in ins]))
    out[np.logical_or.reduce([nan_mask(dt, x) for x in ins])] = 0x7F
    return out


@functools.lru_cache(maxsize=None)
def minmax_case(dt, op, k, n, seed=1):
    ins = sources(dt, k, n, seed)
    return ins, minmax(dt, op, ins)


# ---- SUM, per schedule; r: the scale of the root fold (a 0-dim float32 tensor), None for a plain SUM ----
def scale_of(s):
    """A scale as the kernels hold it: a float."""
    import torch
    return torch.tensor(np.float32(s), dtype=torch.float32)


def recip(P):
    """AVG's r = 1.0f / (float)P."""
    import torch
    return torch.tensor(np.float32(1) / np.float32(P), dtype=torch.float32)


def _acc(dt, ins):
    acc = _t(dt, ins[0]).float()
    for x in ins[1:]:
        acc = acc + _t(dt, x).float()
    return acc


def fold(dt, ins, r=None):
    """One reduce call: fp32 adds left to right, (times r,) one rounding."""
    acc = _acc(dt, ins)
    return _bits((acc if r is None else acc * r).to(torch_dtype(dt)))


def hop_fold(dt, ins, r=None):
    """The one-round ring fold (round_each, k > 2): every add rounds; with r the accumulator is rounded before
    each add and the last sum times r is rounded once."""
    f = torch_dtype(dt)
    acc = _t(dt, ins[0])
    for j, x in enumerate(ins[1:], 1):
        s = acc.float() + _t(dt, x).float()
        acc = (s * r).to(f) if r is not None and j == len(ins) - 1 else s.to(f)
    return _bits(acc)


def nested(dt, ins, shape, r=None):
    """ftar_reduce_nested / ftar_reduce_scaled with a shape: every node one fold; the root takes r."""
    vals = list(ins)
    levels = [w for w in shape if w > 1]
    for li, w in enumerate(levels):
        rr = r if li == len(levels) - 1 else None
        vals = [fold(dt, vals[i:i + w], rr) for i in range(0, len(vals), w)]
    assert len(vals) == 1
    return vals[0]


def ring(dt, ins, r=None):
    """Block b is x_b, then + x_{b+j} for j = 1 .. P-1, one rounding per hop; the last hop is the root."""
    P, n = len(ins), ins[0].size
    out = np.empty(n, np.uint8)
    for b, lo, hi in _blocks(n, P):
        out[lo:hi] = hop_fold(dt, [ins[(b + j) % P][lo:hi] for j in range(P)], r)
    return out


def tree(dt, ins, widths, r=None):
    """Trees without lonely ranks, as f16_minmax_ref.f16_tree: one rounding per node, own value first, then the
    stage group in ascending rank order; block b's node of the last stage on rank b is the root."""
    f = torch_dtype(dt)
    P, n = len(ins), ins[0].size
    assert int(np.prod(widths)) == P
    out = np.empty(n, np.uint8)
    for b, lo, hi in _blocks(n, P):
        vals = {q: _t(dt, ins[q][lo:hi]) for q in range(P)}
        g = 1
        for si, w in enumerate(widths):
            new = {}
            for q in range(P):
                left = q // (g * w) * g * w + q % g
                acc = vals[q].float()
                for j in range(w):
                    p = left + j * g
                    if p != q:
                        acc = acc + vals[p].float()
                root = r is not None and si == len(widths) - 1 and q == b
                new[q] = (acc * r if root else acc).to(f)
            vals = new
            g *= w
        out[lo:hi] = _bits(vals[b])
    return out


@functools.lru_cache(maxsize=None)
def fold_case(dt, k, n, seed=1):
    ins = sources(dt, k, n, seed)
    return ins, fold(dt, ins)


@functools.lru_cache(maxsize=None)
def allreduce_case(dt, P, topo, n, avg=False, seed=1):
    """(per-rank sources, the array every rank must end with) of a SUM (avg: AVG) AllReduce; topo "1" = ring."""
    ins = sources(dt, P, n, seed)
    widths = [int(w) for w in topo.split(",")]
    r = recip(P) if avg else None
    return ins, (ring(dt, ins, r) if 1 in widths else tree(dt, ins, widths, r))


@functools.lru_cache(maxsize=None)
def exact_sum_case(dt, P, n, seed=1):
    """Integer-valued sources in [-2, 2] (sources(small_ints=True)) and their plain sum, exact for any
    association up to P = 8: the lonely layouts, whose fold order this helper does not restate."""
    assert P <= 8
    ins = sources(dt, P, n, seed, small_ints=True)
    tot = sum(_t(dt, x).double() for x in ins)
    want = encode(dt, tot.numpy())
    assert np.array_equal(_t(dt, want).double().numpy(), tot.numpy()), "the sum is representable"
    return ins, want
