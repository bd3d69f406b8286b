"""Independent CPU expectation for the stochastic-rounding quantize (include/ftar.h: ftar_cast_scaled_sr).  Nothing
here calls the library.

sr_bits(dt, u, words) is the header's sr_dst(p, U) in integers, on fp32 bit patterns: the dropped bits of |p| aligned
under the top of the 32-bit word, the carry adding one unit in the last place, running into the next encoding and
past the largest finite one into e5m2's inf / e4m3's NaN.  frac32(dt, u) is F = floor(frac * 2^32), so that
2^32 - F is the smallest word that rounds p up.  words(seed, g) restates the generator U(seed, g).
sr_cast(src_dt, dst_dt, bits, r_bits, seed, offset) is what a whole call stores: cast_ref's exact widening and
float32 multiply, then sr_bits on the generator's words for the global indices offset + i.

Arrays travel as unsigned bit patterns; scales as fp32 bit patterns (ints); seeds and offsets as Python ints taken
modulo 2^64."""
import numpy as np

import cast_ref

M64 = (1 << 64) - 1
U32 = np.uint32
U64 = np.uint64


def _fmt(dt):
    mb, bias = cast_ref.FMT[dt]
    top = 0x7C if dt == "f8e5m2" else 0x7F          # inf / NaN: what an overflow becomes
    return mb, bias, top


def _split(dt, u):
    """|p| as lo units of its ulp plus F / 2^32 of one: (sign byte, exponent base of the encoding, lo, F, special)."""
    mb, bias, _ = _fmt(dt)
    u = np.asarray(u, dtype=U32).astype(U64)
    sign = (u >> U64(24)) & U64(0x80)
    a = u & U64(0x7FFFFFFF)
    e8 = (a >> U64(23)).astype(np.int64)
    sig = (a & U64(0x7FFFFF)) | np.where(e8 > 0, U64(0x800000), U64(0))
    ef = np.maximum(e8, 1) - 127 + bias               # the exponent field |p| would have in the format
    drop = (23 - mb) + np.maximum(1 - ef, 0)          # bits of sig below one ulp
    # sig / 2^drop = lo + F / 2^32 + (less than 2^-32): in 64 bits, (sig << 32) >> drop, drop capped where all is lost
    x = (sig << U64(32)) >> np.minimum(drop, 63).astype(U64)
    base = (np.maximum(ef - 1, 0).astype(U64)) << U64(mb)
    return sign, base, x >> U64(32), x & U64(0xFFFFFFFF), a


def frac32(dt, u):
    """F = floor(frac * 2^32) of each fp32 bit pattern (0 for a representable value, and for inf / NaN)."""
    _, _, _, f, a = _split(dt, u)
    return np.where(a >= U64(0x7F800000), U64(0), f).astype(U32)


def sr_bits(dt, u, words):
    """fp32 bit patterns and one 32-bit word each -> the fp8 encodings sr_dst stores."""
    _, _, top = _fmt(dt)
    sign, base, lo, f, a = _split(dt, u)
    w = np.broadcast_to(np.asarray(words, dtype=U32), a.shape).astype(U64)
    enc = base + lo + ((f + w) >> U64(32))
    enc = np.minimum(enc, U64(top))                   # from 480 / 65536 on, and inf: NaN / inf
    enc = np.where(a > U64(0x7F800000), U64(0x7F), enc)
    return (sign | enc).astype(np.uint8)


def trunc_bits(dt, u):
    """Truncation toward zero written on its own (what U = 0 must give): the largest encoding of the sign whose
    magnitude does not exceed |p|, by searching the table of the format's finite values."""
    mb, bias, top = _fmt(dt)
    u = np.asarray(u, dtype=U32)
    finite = np.arange(0x7C if dt == "f8e5m2" else 0x7F, dtype=np.uint8)
    vals = cast_ref.widen_bits(dt, finite).view(np.float32).astype(np.float64)     # increasing
    with np.errstate(invalid="ignore"):
        a = (u & U32(0x7FFFFFFF)).view(np.float32).astype(np.float64)
    idx = np.searchsorted(vals, a, side="right") - 1
    nxt = 2.0 ** (16 if dt == "f8e5m2" else 8) * (1.0 if dt == "f8e5m2" else 1.875)   # 65536 / 480
    enc = np.where(a >= nxt, top, idx)
    enc = np.where(np.isnan(a), 0x7F, enc)
    return (((u >> U32(24)) & U32(0x80)) | enc.astype(U32)).astype(np.uint8)


# ---- the generator --------------------------------------------------------------------------------------
def keys(seed):
    """(ka, kb): the splitmix64 finaliser of seed + the golden gamma, low and high word."""
    z = (int(seed) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z & 0xFFFFFFFF, z >> 32


def words(seed, g):
    """U(seed, g) for an array (or a scalar) of 64-bit global indices."""
    ka, kb = keys(seed)
    g = np.asarray(g, dtype=U64)
    gl, gh = (g & U64(0xFFFFFFFF)).astype(U32), (g >> U64(32)).astype(U32)
    with np.errstate(over="ignore"):
        x = gl ^ U32(ka)
        x = (x ^ (x >> U32(16))) * U32(0x7FEB352D)
        x = x + (U32(kb) ^ (gh * U32(0x9E3779B9)))
        x = (x ^ (x >> U32(15))) * U32(0x846CA68B)
        return x ^ (x >> U32(16))


def indices(offset, n):
    """The global indices offset + i, i < n, modulo 2^64."""
    with np.errstate(over="ignore"):
        return U64(int(offset) & M64) + np.arange(n, dtype=U64)


def rank_seed(seed, rank):
    """The device seed ftar.ddp.Fp8CompressState derives for a rank: the splitmix64 finaliser of seed + (rank + 1)
    golden gammas."""
    z = (int(seed) + (int(rank) + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ---- a whole call ---------------------------------------------------------------------------------------
def product_bits(src_dt, bits, r_bits=None):
    """fp32 bit patterns of mul_rn_f32(widen(src), r)."""
    r = np.array([cast_ref.ONE if r_bits is None else r_bits], U32).view(np.float32)[0]
    x = cast_ref.widen_bits(src_dt, bits).view(np.float32)
    with np.errstate(all="ignore"):
        return (x * r).astype(np.float32).view(U32)


def sr_cast_words(src_dt, dst_dt, bits, r_bits, w):
    return sr_bits(dst_dt, product_bits(src_dt, bits, r_bits), w)


def sr_cast(src_dt, dst_dt, bits, r_bits, seed, offset=0):
    """What ftar_cast_scaled_sr stores for these source bit patterns, this scale, seed value and offset."""
    bits = np.asarray(bits)
    return sr_cast_words(src_dt, dst_dt, bits, r_bits, words(seed, indices(offset, bits.size)))
