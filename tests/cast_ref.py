"""Independent CPU expectation for the scaled casts (include/ftar.h: ftar_cast_scaled).  Nothing here calls the
library.

cast(dt_src, dt_dst, bits, r_bits) is dst = cvt_dst(fp32(widen(src)) * r) written from what already pins these
formats: the widening is torch's exact cast of every encoding, taken once as a table (what amax_ref.widen does one
encoding at a time); the product is numpy's float32 multiply (correctly rounded, subnormals kept); the narrowing is
f8_ref.rne_bits for fp8 and rne16_bits below, the same integer RNE for the two 16-bit layouts (tests/test_cast_api.py
holds both against torch's casts).  That is two roundings whenever dst is narrower than fp32.

witnesses(dt_dst, dt_src) are operands whose EXACT product rounds differently once (straight to dst) than twice
(to fp32, then to dst), found by a search in exact rational arithmetic: random inputs hit no such case in 2^20
draws, so a kernel that fuses the multiply into the conversion passes everything else here.

Arrays travel as unsigned bit patterns; scales as fp32 bit patterns (ints).  Results may be cached by callers and
must not be modified."""
import functools
from fractions import Fraction

import numpy as np

import f16_minmax_ref as ref
import f8_ref

WIDE = ("f32", "bf16", "f16")
F8 = f8_ref.FORMATS
ID = {"f32": 6, "bf16": 9, "f16": 10, "f8e4m3": 12, "f8e5m2": 13}
PAIRS = [(w, f) for w in WIDE for f in F8] + [(f, w) for f in F8 for w in WIDE]       # the 12 that run
STORAGE = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16, "f8e4m3": np.uint8, "f8e5m2": np.uint8}
FMT = {"f32": (23, 127), "bf16": (7, 127), "f16": (10, 15), "f8e4m3": (3, 7), "f8e5m2": (2, 15)}   # mantissa bits, bias
ONE = 0x3F800000
THIRD = 0x3EAAAAAB
SCALES = (ONE, 0x3F000000, 0x40400000, THIRD, 0x35800000, 0x49800000)       # 1, 0.5, 3, 1/3, 2^-20, 2^20
ODD_SCALES = {"zero": 0x00000000, "minus one": 0xBF800000, "inf": 0x7F800000, "nan": 0x7FC00000,
              "subnormal": 0x00000123, "flt_max": 0x7F7FFFFF}

assert np.float32(2.0 ** -126) * np.float32(0.5) != 0, "numpy's float32 multiply keeps subnormal products here"


def storage(dt):
    return STORAGE[dt]


def is_f8(dt):
    return dt in F8


def nan_mask(dt, bits):
    return f8_ref.nan_mask(dt, bits) if is_f8(dt) else ref.nan_mask(dt, np.asarray(bits).view(storage(dt)))


def same_bits(dt, got, want):
    """got == want bit for bit, NaN lanes as "NaN or not": the comparison of f8_ref.same_bits / f16_minmax_ref.
    same_bits on their own nan_mask, without their cap on the expectation's NaN share -- a cast at scale 2^20 is
    NaN (e4m3) in most lanes by design, and those lanes are what such a case checks."""
    got, want = np.asarray(got).view(storage(dt)), np.asarray(want).view(storage(dt))
    if got.shape != want.shape:
        return False
    ng, nw = nan_mask(dt, got), nan_mask(dt, want)
    return bool(np.array_equal(ng, nw) and np.array_equal(got[~nw], want[~nw]))


def first_diff(dt, got, want):
    got, want = np.asarray(got).view(storage(dt)), np.asarray(want).view(storage(dt))
    ng, nw = nan_mask(dt, got), nan_mask(dt, want)
    i = np.flatnonzero((ng != nw) | (~nw & (got != want)))
    return None if not i.size else (int(i[0]), hex(int(got[i[0]])), hex(int(want[i[0]])), int(i.size))


# ---- widening: torch's exact cast of every encoding, once -----------------------------------------------
@functools.lru_cache(maxsize=None)
def _widen_table(dt):
    import torch

    import avg_ref
    if is_f8(dt):
        t = f8_ref._t(dt, np.arange(256, dtype=np.uint8))
    else:
        t = avg_ref._t(dt, np.arange(65536, dtype=np.uint16))
    return t.to(torch.float32).view(torch.int32).numpy().view(np.uint32).copy()


def widen_bits(dt, bits):
    """fp32 bit patterns of the elements (exact in every format here)."""
    bits = np.asarray(bits).view(storage(dt))
    return bits.astype(np.uint32) if dt == "f32" else _widen_table(dt)[bits]


# ---- narrowing to a 16-bit format, in integers ------------------------------------------------------------
def rne16_bits(dt, u):
    """float32 bit patterns -> bf16 / f16 encodings: RNE on the encoding, the mantissa carry running into the next
    encoding, overflow to inf, gradual underflow; a NaN becomes the quiet NaN of its sign (f8_ref.rne_bits'
    construction on a layout with an inf)."""
    mb, bias = FMT[dt]
    inf = ((1 << (15 - mb)) - 1) << mb
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    sign = (u >> np.uint64(16)) & np.uint64(0x8000)
    a = u & np.uint64(0x7FFFFFFF)
    sh = 23 - mb
    r = a - np.minimum(a, np.uint64((127 - bias) << 23))
    q = (r + np.uint64((1 << (sh - 1)) - 1) + ((r >> np.uint64(sh)) & np.uint64(1))) >> np.uint64(sh)
    normal = np.minimum(q, np.uint64(inf))
    e = (a >> np.uint64(23)).astype(np.int64)
    m = (a & np.uint64(0x7FFFFF)) | np.where(e > 0, np.uint64(0x800000), np.uint64(0))
    shift = np.clip((151 - bias - mb) - np.maximum(e, 1), 1, 26).astype(np.uint64)
    h = m >> shift
    rem = m & ((np.uint64(1) << shift) - np.uint64(1))
    half = np.uint64(1) << (shift - np.uint64(1))
    sub = h + ((rem > half) | ((rem == half) & ((h & np.uint64(1)) == 1))).astype(np.uint64)
    out = np.where(a >= np.uint64((127 - bias + 1) << 23), normal, sub)
    out = np.where(a >= np.uint64(0x7F800000), np.uint64(inf), out)
    out = np.where(a > np.uint64(0x7F800000), np.uint64(inf | (1 << (mb - 1))), out)
    return (sign | out).astype(np.uint16)


def narrow_bits(dt, u):
    u = np.asarray(u, dtype=np.uint32)
    if dt == "f32":
        return u
    return f8_ref.rne_bits(dt, u) if is_f8(dt) else rne16_bits(dt, u)


# ---- the cast -------------------------------------------------------------------------------------------
def cast(dt_src, dt_dst, bits, r_bits=None):
    """What ftar_cast_scaled stores for these source bit patterns and this scale (fp32 bits; None: no scale, the
    multiply by 1.0f)."""
    r = np.array([ONE if r_bits is None else r_bits], np.uint32).view(np.float32)[0]
    x = widen_bits(dt_src, bits).view(np.float32)
    with np.errstate(all="ignore"):
        p = (x * r).astype(np.float32)
    return narrow_bits(dt_dst, p.view(np.uint32))


def torch_cast(dt_src, dt_dst, bits, r_bits=None):
    """The same through torch on the CPU: (src.to(float32) * r).to(dst_dtype)."""
    import torch

    import avg_ref
    tt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f8e4m3": torch.float8_e4m3fn,
          "f8e5m2": torch.float8_e5m2}
    bits = np.ascontiguousarray(np.asarray(bits).view(storage(dt_src)))
    if is_f8(dt_src):
        s = f8_ref._t(dt_src, bits)
    elif dt_src == "f32":
        s = torch.from_numpy(bits.view(np.float32).copy())
    else:
        s = avg_ref._t(dt_src, bits)
    r = torch.from_numpy(np.array([ONE if r_bits is None else r_bits], np.uint32).view(np.float32).copy())
    out = (s.to(torch.float32) * r).to(tt[dt_dst])
    if is_f8(dt_dst):
        return f8_ref._bits(out)
    if dt_dst == "f32":
        return out.numpy().view(np.uint32)
    return out.view(torch.int16).numpy().view(np.uint16)


# ---- exact arithmetic on encodings ------------------------------------------------------------------------
def frac_of(dt, enc):
    """The exact value of a finite non-negative encoding."""
    mb, bias = FMT[dt]
    e, m = enc >> mb, enc & ((1 << mb) - 1)
    if e == 0:
        return Fraction(m) * Fraction(2) ** (1 - bias - mb)
    return Fraction((1 << mb) | m) * Fraction(2) ** (e - bias - mb)


def round_frac(dt, v):
    """The encoding a positive rational rounds to (RNE, gradual underflow; below the overflow threshold)."""
    mb, bias = FMT[dt]
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    e = max(e, 1 - bias)
    q = v / Fraction(2) ** (e - mb)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    # n in [0, 2^(mb+1)]: the encoding is (e + bias - 1) << mb plus n (n carries the implicit bit, or overflows
    # into the next exponent, or stays below it for a subnormal)
    return ((e + bias - 1) << mb) + n


def enc_of(dt, v):
    """The encoding of a positive rational if dt holds it exactly, else None."""
    enc = round_frac(dt, v)
    return enc if frac_of(dt, enc) == v else None


@functools.lru_cache(maxsize=None)
def witnesses(dt_dst, dt_src="f32", want=3):
    """`want` pairs (x, r): x an encoding of dt_src, r fp32 bits, both positive and finite, whose exact product
    lies just above a tie t of dt_dst with the even neighbour below -- so close that fp32 rounds it down onto t.
    Two roundings give the even encoding below t, one rounding the odd one above.  Every pair is verified here in
    exact arithmetic: (x, r, encoding after two roundings, encoding after one)."""
    assert dt_dst != "f32" and dt_src in ("f32",) + F8
    mb, bias = FMT[dt_dst]
    smb, _ = FMT[dt_src]
    out = []
    if dt_src == "f32":
        fixed = [("r", Fraction(k)) for k in range(3, 33, 2)]               # the scale; x is solved for
    else:   # every source value 1.m with an odd numerator; r is solved for
        fixed = [("x", Fraction((1 << smb) | m, 1 << smb)) for m in range(1, 1 << smb, 2)]
    ties = [((e << mb) | m) for e in (bias, bias + 1, bias - 2, bias + 3, bias - 1, bias + 2, bias - 3)
            for m in range(0, 1 << mb, 2)]                                  # even mantissas around 1, 2, 1/4, 8, ...
    for d0 in ties:
        t = (frac_of(dt_dst, d0) + frac_of(dt_dst, d0 + 1)) / 2
        ulp32 = Fraction(2) ** (round_frac("f32", t) >> 23) / Fraction(2) ** (127 + 23)
        for eps in (Fraction(1, 4), Fraction(1, 8), Fraction(3, 8)):        # of an fp32 ulp: rounds down onto t
            p = t + ulp32 * eps
            for which, a in fixed:
                b = enc_of("f32", p / a)
                if b is None:
                    continue
                x, r = (b, enc_of("f32", a)) if which == "r" else (enc_of(dt_src, a), b)
                exact = frac_of(dt_src, x) * frac_of("f32", r)
                assert exact == p
                once = round_frac(dt_dst, exact)
                twice = round_frac(dt_dst, frac_of("f32", round_frac("f32", exact)))
                assert (twice, once) == (d0, d0 + 1), (dt_dst, dt_src, hex(x), hex(r))
                out.append((x, r, twice, once))
                if len(out) == want:
                    return tuple(out)
    raise AssertionError(f"no double-rounding witness found for {dt_src} -> {dt_dst}")


def witness_pairs():
    """(dt_src, dt_dst) of every pair that has witnesses: an f32 source into both fp8 formats, and both fp8 sources
    into bf16 / f16 (a 16-bit source times an fp32 scale into fp8 is searched as f32's: its values are f32's)."""
    return [("f32", f) for f in F8] + [(f, w) for f in F8 for w in ("bf16", "f16")]
