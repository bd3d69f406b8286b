"""Independent CPU expectation for the MX block-scaled casts (include/ftar.h: ftar_mx_scales, ftar_mx_quantize,
ftar_mx_dequantize).  Nothing here calls the library.

The scale byte of a block is the header's integer rule on the block's largest sign-cleared fp32 bit pattern
(cast_ref.widen_bits: torch's exact widening as a table).  The payload and the dequantize are cast_ref.cast on each
block with r_bits = q(s) / d(s) -- blocks that share a scale byte go through one call, element-wise the same -- and a
block whose byte is 255 dequantizes to NaN.  tests/test_mx_api.py holds the rule against torch.frexp on the CPU.

Arrays travel as unsigned bit patterns (cast_ref.storage), scale bytes as uint8.  Compare with cast_ref.same_bits
(NaN lanes as "NaN or not")."""
import numpy as np

import cast_ref

BLOCK = 32
EMAX = {"f8e4m3": 8, "f8e5m2": 15}
MAX_FINITE = {"f8e4m3": 448.0, "f8e5m2": 57344.0}          # 1.75 x 2^emax
NAN_BITS = {"f32": 0x7FC00000, "bf16": 0x7FC0, "f16": 0x7E00}
F32_INF = 0x7F800000


def nblocks(n):
    return (int(n) + BLOCK - 1) // BLOCK


def scale_of(a, f8, headroom=0):
    """The rule, on sign-cleared fp32 bit patterns `a` (an array or an int): uint8 scale bytes."""
    a = np.atleast_1d(np.asarray(a, dtype=np.uint32)).astype(np.int64)
    e = (a >> 23) - EMAX[f8] + ((a & 0x7FFFFF) > 0x600000)
    s = np.minimum(254, np.maximum(0, e) + int(headroom))
    return np.where(a >= F32_INF, 255, s).astype(np.uint8)


def peaks(src_dt, bits):
    """Per block (a partial last block on its own elements): the unsigned maximum of bits(widen(x)) & 0x7fffffff."""
    a = cast_ref.widen_bits(src_dt, bits) & np.uint32(0x7FFFFFFF)
    pad = np.zeros(nblocks(a.size) * BLOCK, np.uint32)
    pad[:a.size] = a
    return pad.reshape(-1, BLOCK).max(axis=1)


def scales(src_dt, f8, bits, headroom=0):
    """What ftar_mx_scales stores for a wide source."""
    return scale_of(peaks(src_dt, bits), f8, headroom)


def q_bits(s):
    s = int(s)
    return (254 - s) << 23 if s <= 253 else 0x00400000 if s == 254 else 0x3F800000


def d_bits(s):
    """fp32 bits of 2^(s - 127), s in 0..254."""
    s = int(s)
    assert s != 255
    return 0x00400000 if s == 0 else s << 23


def _per_element(sc, n):
    sc = np.asarray(sc, dtype=np.uint8)
    assert sc.size >= nblocks(n)
    return np.repeat(sc[:nblocks(n)], BLOCK)[:n]


def quantize(src_dt, f8, bits, sc):
    """What ftar_mx_quantize stores with these scale bytes (given, or scales() for the compute mode)."""
    bits = np.asarray(bits).view(cast_ref.storage(src_dt))
    per = _per_element(sc, bits.size)
    out = np.zeros(bits.size, np.uint8)
    for s in np.unique(per):
        m = per == s
        out[m] = cast_ref.cast(src_dt, f8, bits[m], q_bits(s))
    return out


def dequantize(f8, dst_dt, bits, sc):
    """What ftar_mx_dequantize stores; a block whose byte is 255 is NaN in every element."""
    bits = np.asarray(bits).view(np.uint8)
    per = _per_element(sc, bits.size)
    out = np.zeros(bits.size, cast_ref.storage(dst_dt))
    for s in np.unique(per):
        m = per == s
        out[m] = NAN_BITS[dst_dt] if s == 255 else cast_ref.cast(f8, dst_dt, bits[m], d_bits(s))
    return out
