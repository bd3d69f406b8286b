"""Independent CPU expectation for ftar_cast_half_sr (include/ftar.h): sr16(p, U) in numpy integers on fp32 bit
patterns, for "bf16" (m = 7, emin = -126) and "f16" (m = 10, emin = -14).  The product, the words and the indices
are cast_ref's and sr_ref's.  Nothing here calls the library."""
import numpy as np

import cast_ref
import sr_ref

U32, U64 = np.uint32, np.uint64
INF = {"bf16": 0x7F80, "f16": 0x7C00}


def _split(dt, u):
    """|p| = (lo + F / 2^32) ulps: (sign, lo on the encoding's scale, F, |p|'s bits)."""
    mb, bias = cast_ref.FMT[dt]
    u = np.asarray(u, dtype=U32).astype(U64)
    a = u & U64(0x7FFFFFFF)
    e8 = (a >> U64(23)).astype(np.int64)
    sig = (a & U64(0x7FFFFF)) | np.where(e8 > 0, U64(0x800000), U64(0))
    ef = np.maximum(e8, 1) - 127 + bias                  # the exponent field |p| would have in the format
    drop = (23 - mb) + np.maximum(1 - ef, 0)             # bits of sig below one ulp
    x = (sig << U64(32)) >> np.minimum(drop, 63).astype(U64)
    base = np.maximum(ef - 1, 0).astype(U64) << U64(mb)
    return (u >> U64(16)) & U64(0x8000), base + (x >> U64(32)), x & U64(0xFFFFFFFF), a


def frac32(dt, u):
    """F = floor(frac * 2^32) of each fp32 bit pattern (0 for a representable value, and for inf / NaN)."""
    _, _, f, a = _split(dt, u)
    return np.where(a >= U64(0x7F800000), U64(0), f).astype(U32)


def sr16_bits(dt, u, words):
    """fp32 bit patterns and one 32-bit word each -> the 16-bit encodings sr16 stores."""
    sign, lo, f, a = _split(dt, u)
    w = np.broadcast_to(np.asarray(words, dtype=U32), a.shape).astype(U64)
    enc = np.minimum(lo + ((f + w) >> U64(32)), U64(INF[dt]))
    enc = np.where(a > U64(0x7F800000), U64(INF[dt] | 1), enc)
    return (sign | enc).astype(np.uint16)


def widen(dt, enc):
    with np.errstate(invalid="ignore"):
        return cast_ref.widen_bits(dt, enc).view(np.float32).astype(np.float64)


def sr_cast_words(dt, bits, r_bits, w):
    return sr16_bits(dt, sr_ref.product_bits("f32", bits, r_bits), w)


def sr_cast(dt, bits, r_bits, seed, offset=0):
    """What ftar_cast_half_sr stores for these f32 bit patterns, this scale, seed value and offset."""
    return sr_cast_words(dt, bits, r_bits, sr_ref.words(seed, sr_ref.indices(offset, np.asarray(bits).size)))
