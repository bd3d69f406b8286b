"""Independent CPU expectations for the extensions that have no reference and no oracle entry: the fp16
(IEEE binary16) SUM and the MAX / MIN reductions of every dtype (include/ftar.h).

  * fp16 SUM: PyTorch on the CPU, `.float()` adds and `.to(torch.float16)` (round to nearest even, overflow
    to inf, gradual underflow), written out as the fold each schedule performs, exactly as
    tests/test_bf16_torch_pin.py writes bf16: the flat fold (one rounding), the ring (one rounding per hop),
    and the trees (one rounding per node, own value first, then the stage group in ascending rank order).
  * MAX / MIN of integers: numpy maximum.reduce / minimum.reduce on the typed arrays.
  * MAX / MIN of floats: the bit patterns mapped to monotone unsigned keys (negatives: all bits flipped;
    non-negatives: sign bit set), the keys reduced as unsigned integers and mapped back; NaN lanes (any NaN
    source) are flagged separately.  This is IEEE 754-2019 maximum / minimum without trusting any
    library's max: -0 < +0, subnormals are ordinary values, the result is one of the sources bit for bit.

The helper builds its own inputs (sources()): random bit patterns whose all-ones exponents are replaced so the
bulk is finite (raw 16-bit patterns are 3 % NaN per source: at k = 16 that is 40 % NaN lanes, which would hide
failures), with specials planted at fixed strides in different sources.  Every comparison goes through
same_bits(), which also asserts that the expectation's NaN-lane share stays below NAN_SHARE_CAP.

Float arrays travel as their unsigned bit patterns (uint16 / uint32 / uint64); results are cached and shared
between tests, so callers must not modify what these functions return."""
import functools

import numpy as np

ID = {"u8": 0, "i8": 1, "u16": 2, "i16": 3, "i32": 4, "i64": 5, "f32": 6, "f64": 7, "bool": 8, "bf16": 9, "f16": 10}
INTS = {"u8": np.uint8, "i8": np.int8, "u16": np.uint16, "i16": np.int16, "i32": np.int32, "i64": np.int64}
# float formats: (unsigned storage type, bits, exponent mask, lowest exponent bit)
FLOATS = {"f16": (np.uint16, 16, 0x7C00, 0x0400), "bf16": (np.uint16, 16, 0x7F80, 0x0080),
          "f32": (np.uint32, 32, 0x7F800000, 0x00800000),
          "f64": (np.uint64, 64, 0x7FF0000000000000, 0x0010000000000000)}
MINMAX_DTYPES = ["u8", "i8", "u16", "i16", "i32", "i64", "f32", "f64", "bf16", "f16"]
NAN_SHARE_CAP = 0.05


def storage(dt):
    return INTS[dt] if dt in INTS else FLOATS[dt][0]


def _fmt(dt):
    u, bits, emask, elow = FLOATS[dt]
    sign = 1 << (bits - 1)
    return u, bits, u(emask), u(elow), u(sign), u(sign - 1)


def nan_mask(dt, bits):
    u, _, emask, _, _, amask = _fmt(dt)
    return (np.asarray(bits, dtype=u) & amask) > emask


# ---- inputs --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sources(dt, k, n, seed=1, small_ints=False):
    """k sources of n elements of dtype dt (a tuple of arrays; floats as bit patterns).  Lane 0 is never a
    planted special, so n = 1 is an ordinary finite lane.  small_ints: integer values in [-8, 8] instead
    (every association of their sum is exact in fp16 and bf16)."""
    rng = np.random.default_rng([seed, ID[dt], k, n])
    if small_ints:
        vals = rng.integers(-8, 9, size=(k, n))
        if dt in INTS:
            return tuple(v.astype(INTS[dt]) for v in vals)
        return tuple(encode(dt, v.astype(np.float64)) for v in vals)
    if dt in INTS:
        t = np.dtype(INTS[dt])
        u = np.dtype(f"u{t.itemsize}")
        xs = [rng.integers(0, 1 << (8 * t.itemsize), size=n, dtype=u, endpoint=False).view(t) for _ in range(k)]
        info = np.iinfo(t)
        xs[0][29::97] = info.max            # the extremes, where signed and unsigned compares part
        xs[k - 1][31::89] = info.min
        xs[k // 2][37::83] = -1 if info.min < 0 else info.max // 2 + 1   # 0xFF.. / 0x80..: the sign bit
        return tuple(xs)
    u, bits, emask, elow, sign, amask = _fmt(dt)
    xs = []
    for _ in range(k):
        b = rng.integers(0, 1 << bits, size=n, dtype=u, endpoint=False)
        xs.append(np.where((b & emask) == emask, b & ~elow, b).astype(u))   # all-ones exponent -> finite
    xs[0][31::97] = emask | (elow >> u(1)) | u(1)          # a quiet NaN with a payload
    xs[k - 1][3::89] = emask                                # +inf
    xs[k // 2][5::83] = sign | emask                        # -inf
    for j in range(k):                                      # lanes where every source is a zero:
        xs[j][11::101] = sign if j % 2 == 0 else 0          #   -0 first, +0 and -0 facing each other
        xs[j][12::101] = 0 if j % 2 == 0 else sign          #   +0 first
        xs[j][17::103] = u(1 + j)                           # lanes of positive subnormals 1 .. k ulp
        xs[j][18::103] = sign | u(1 + j)                    # lanes of negative subnormals
    xs[k - 1][13::79] = u(1)                                # the smallest subnormal among ordinary values
    if dt == "f16":   # SUM: ties that round to even, and a sum that overflows to inf (other sources: +0)
        for j in range(k):
            for off in (19, 20, 21):
                xs[j][off::107] = 0
        xs[0][19::107], xs[1][19::107] = 0x6800, 0x3C00     # 2048 + 1 = 2049  -> 2048 (even mantissa)
        xs[0][20::107], xs[1][20::107] = 0x6801, 0x3C00     # 2050 + 1 = 2051  -> 2052
        xs[0][21::107], xs[1][21::107] = 0x7BFF, 0x4C00     # 65504 + 16 = 65520 -> +inf
    return tuple(xs)


def encode(dt, values):
    """Exactly representable float64 values -> bit patterns of float dtype dt (torch does the conversion)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64))
    if dt == "f16":
        return t.to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    if dt == "bf16":
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    if dt == "f32":
        return t.to(torch.float32).numpy().view(np.uint32)
    return t.numpy().view(np.uint64)


# ---- comparing ------------------------------------------------------------------------------------------
def same_bits(dt, got, ref):
    """got == ref bit for bit; float NaN lanes compare as NaN or not.  Asserts the NaN-share cap."""
    got, ref = np.asarray(got).view(storage(dt)), np.asarray(ref).view(storage(dt))
    if got.shape != ref.shape:
        return False
    if dt in INTS:
        return bool(np.array_equal(got, ref))
    ng, nr = nan_mask(dt, got), nan_mask(dt, ref)
    share = float(nr.mean()) if nr.size else 0.0
    assert share < NAN_SHARE_CAP, f"the expectation is {share:.1%} NaN lanes: the inputs hide failures"
    return bool(np.array_equal(ng, nr) and np.array_equal(got[~nr], ref[~nr]))


def first_diff(dt, got, ref):
    """For assertion messages: (lane, got bits, expected bits) of the first mismatch, or None."""
    got, ref = np.asarray(got).view(storage(dt)), np.asarray(ref).view(storage(dt))
    bad = got != ref
    if dt in FLOATS:
        ng, nr = nan_mask(dt, got), nan_mask(dt, ref)
        bad = (ng != nr) | (~nr & bad)
    i = np.flatnonzero(bad)
    return None if not i.size else (int(i[0]), hex(int(got[i[0]])), hex(int(ref[i[0]])), int(i.size))


# ---- MAX / MIN ------------------------------------------------------------------------------------------
def float_keys(dt, bits):
    """Monotone unsigned keys of float bit patterns: key(x) < key(y) exactly when x < y in the total order
    -inf < ... < -0 < +0 < ... < +inf (NaNs sort outside it and are handled by the caller)."""
    u, _, _, _, sign, _ = _fmt(dt)
    b = np.asarray(bits, dtype=u)
    return np.where(b & sign, ~b, b | sign).astype(u)


def keys_to_bits(dt, keys):
    u, _, _, _, sign, _ = _fmt(dt)
    k = np.asarray(keys, dtype=u)
    return np.where(k & sign, k ^ sign, ~k).astype(u)


def minmax(dt, op, ins):
    """Expected MAX / MIN (op = "max" | "min") of the sources, any association.  Float NaN lanes hold a NaN."""
    f = np.maximum if op == "max" else np.minimum
    if dt in INTS:
        return f.reduce([np.asarray(x, dtype=INTS[dt]) for x in ins])
    u, _, emask, elow, _, _ = _fmt(dt)
    out = keys_to_bits(dt, f.reduce([float_keys(dt, x) for x in ins]))
    nan = np.logical_or.reduce([nan_mask(dt, x) for x in ins])
    out[nan] = emask | elow >> u(1)
    return out


@functools.lru_cache(maxsize=None)
def minmax_case(dt, op, k, n, seed=1):
    """(sources, expectation) of one MAX / MIN case, computed once."""
    ins = sources(dt, k, n, seed)
    return ins, minmax(dt, op, ins)


# ---- fp16 SUM, per schedule -----------------------------------------------------------------------------
def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16).copy()).view(torch.float16)


def _bits(t):
    import torch
    return t.view(torch.int16).numpy().view(np.uint16)


def f16_fold(ins):
    """ftar_reduce: round(x0 + x1 + ... + x_{k-1}), fp32 adds left to right, one rounding."""
    import torch
    acc = _t(ins[0]).float()
    for x in ins[1:]:
        acc = acc + _t(x).float()
    return _bits(acc.to(torch.float16))


@functools.lru_cache(maxsize=None)
def f16_fold_case(k, n, seed=1):
    ins = sources("f16", k, n, seed)
    return ins, f16_fold(ins)


def f16_nested(ins, shape):
    """ftar_reduce_nested: level 0 folds shape[0] consecutive leaves, level 1 folds shape[1] consecutive
    level-0 results, ...; every node is one f16_fold (so every inner node is rounded)."""
    vals = list(ins)
    for w in shape:
        vals = [f16_fold(vals[i:i + w]) if w > 1 else vals[i] for i in range(0, len(vals), w)]
    assert len(vals) == 1
    return vals[0]


def _blocks(n, P):
    split = -(-n // P)
    return [(b, b * split, min(n, (b + 1) * split)) for b in range(P) if b * split < min(n, (b + 1) * split)]


def f16_ring(ins):
    """The ring: block b is x_b, then + x_{b+j} for j = 1 .. P-1 with one rounding per hop
    (mpi_mod.hpp:1689-1703); every rank ends with the same array."""
    import torch
    P, n = len(ins), ins[0].size
    ref = np.empty(n, np.uint16)
    for b, lo, hi in _blocks(n, P):
        acc = _t(ins[b][lo:hi])
        for j in range(1, P):
            acc = (acc.float() + _t(ins[(b + j) % P][lo:hi]).float()).to(torch.float16)
        ref[lo:hi] = _bits(acc)
    return ref


def f16_tree(ins, widths):
    """Trees without lonely ranks: at stage s rank q's partial of block b folds its own value first, then
    its stage group's partials in ascending rank order (group = left + j*g, mpi_mod.hpp:274, :369), and is
    rounded once -- per node of the tree.  widths = [P] is the single-stage tree."""
    import torch
    P, n = len(ins), ins[0].size
    assert int(np.prod(widths)) == P
    ref = np.empty(n, np.uint16)
    for b, lo, hi in _blocks(n, P):
        vals = {q: _t(ins[q][lo:hi]) for q in range(P)}
        g = 1
        for w in widths:
            new = {}
            for q in range(P):
                left = q // (g * w) * g * w + q % g
                acc = vals[q].float()
                for j in range(w):
                    p = left + j * g
                    if p != q:
                        acc = acc + vals[p].float()
                new[q] = acc.to(torch.float16)
            vals = new
            g *= w
        ref[lo:hi] = _bits(vals[b])
    return ref


@functools.lru_cache(maxsize=None)
def f16_allreduce_case(P, topo, n, seed=1):
    """(per-rank sources, the array every rank must end with) of an fp16 SUM AllReduce; topo "1" = ring."""
    ins = sources("f16", P, n, seed)
    widths = [int(w) for w in topo.split(",")]
    return ins, (f16_ring(ins) if 1 in widths else f16_tree(ins, widths))


@functools.lru_cache(maxsize=None)
def exact_sum_case(dt, P, n, seed=1):
    """Integer-valued sources in [-8, 8] and their plain sum (exact in fp16 for any association: the lonely
    layouts, whose fold order this helper does not restate)."""
    ins = sources(dt, P, n, seed, small_ints=True)
    import torch
    tt = {"f16": torch.float16, "bf16": torch.bfloat16}[dt]
    tot = sum(torch.from_numpy(x.view(np.int16).copy()).view(tt).double() for x in ins)
    assert float(tot.abs().max()) <= 8 * P
    return ins, encode(dt, tot.numpy())
