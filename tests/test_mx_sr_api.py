"""The stochastic MX quantize (include/ftar.h: ftar_mx_quantize_sr) and the MX gradient hook's rounding switch,
without a GPU: the symbol, every refusal on host buffers that must keep their bytes (nothing here may reach HIP), the
Python checks, the properties of the composed reference tests/mx_sr_ref.py (mx_ref's products through sr_ref's
narrowing), and its unbiasedness against the round-to-nearest payload."""
import ctypes
import os

import numpy as np
import pytest

import cast_ref
import mx_ref
import mx_sr_ref
import sr_ref
from test_gpu_mx import spread

INVALID_ARG, UNSUPPORTED = 1, 2
WIDE_IDS = [cast_ref.ID[w] for w in cast_ref.WIDE]
F8_IDS = [cast_ref.ID[f] for f in cast_ref.F8]
COMBOS = [(w, f) for w in cast_ref.WIDE for f in cast_ref.F8]
TOP = (1 << 32) - 1
SEED = 0x0123456789ABCDEF


class Host:
    """Host buffers standing in for device memory: a refused call must leave every byte."""

    def __init__(self):
        self.src = (ctypes.c_ubyte * 512)(*([0x5A] * 512))
        self.dst = (ctypes.c_ubyte * 512)(*([0xA5] * 512))
        self.sc = (ctypes.c_ubyte * 64)(*([0xC3] * 64))
        self.seed = (ctypes.c_uint64 * 4)(*([0x1111111111111111] * 4))

    def ptrs(self):
        seed = ctypes.addressof(self.seed)
        assert seed % 8 == 0
        return ctypes.addressof(self.src), ctypes.addressof(self.dst), ctypes.addressof(self.sc), seed

    def untouched(self):
        return (bytes(self.src) == b"\x5a" * 512 and bytes(self.dst) == b"\xa5" * 512 and bytes(self.sc) == b"\xc3" * 64
                and bytes(self.seed) == b"\x11" * 32)


def call(src, sdt, dst, ddt, n, mode, headroom, sc, seed, offset=0):
    import ftar
    return ftar.lib().ftar_mx_quantize_sr(src, sdt, dst, ddt, n, mode, headroom, sc, seed, offset, None)


# ---- the entry point --------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared():
    import ftar
    assert hasattr(ftar.lib(), "ftar_mx_quantize_sr")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ftar.h")).read()
    assert "ftar_mx_quantize_sr(" in header
    assert "stochastic rounding of the MX quantize" not in header and "MXFP6 / MXFP4 are not covered" in header


def test_every_pair_but_the_six_is_refused_first():
    """All dtype ids 0..13 squared: an unsupported pair is status 2 whatever else is wrong with the call (NULL
    pointers, a bad mode, a bad headroom, a NULL or misaligned seed, count 0); a supported one gets past that check."""
    h = Host()
    src, dst, sc, seed = h.ptrs()
    passed = []
    for a in range(14):
        for b in range(14):
            st = call(None, a, None, b, 1, 0, 0, None, seed)
            assert st in (INVALID_ARG, UNSUPPORTED), (a, b, st)
            if st == INVALID_ARG:
                passed.append((a, b))
                continue
            assert call(src, a, dst, b, 64, 7, 99, sc, None) == UNSUPPORTED
            assert call(src, a, dst, b, 64, 0, 0, sc, seed + 4) == UNSUPPORTED
            assert call(src, a, dst, b, 64, 0, 0, sc, seed) == UNSUPPORTED
            assert call(src, a, dst, b, 0, 0, 0, sc, seed) == UNSUPPORTED
    assert sorted(passed) == sorted((w, f) for w in WIDE_IDS for f in F8_IDS) and len(passed) == 6
    for bad in (-1, 11, 14, 255):
        assert call(src, bad, dst, 12, 64, 0, 0, sc, seed) == UNSUPPORTED
        assert call(src, 6, dst, bad, 64, 0, 0, sc, seed) == UNSUPPORTED
    for f in F8_IDS:        # the dequantize direction has no stochastic form
        for w in WIDE_IDS:
            assert call(src, f, dst, w, 64, 0, 0, sc, seed) == UNSUPPORTED
    assert h.untouched()


@pytest.mark.parametrize("f8", F8_IDS)
@pytest.mark.parametrize("wide", WIDE_IDS)
def test_invalid_arguments_in_the_headers_order_leave_the_buffers(wide, f8):
    """Mode, headroom, seed, pointers: each alone, each with everything after it in the order wrong too, and at
    count == 0, where the mode, the headroom and the seed are still checked and the pointers are not."""
    h = Host()
    src, dst, sc, seed = h.ptrs()
    ok = dict(src=src, dst=dst, n=64, mode=0, headroom=0, sc=sc, seed=seed)

    def st(**kw):
        a = {**ok, **kw}
        return call(a["src"], wide, a["dst"], f8, a["n"], a["mode"], a["headroom"], a["sc"], a["seed"])
    later = dict(seed=None, src=None, dst=None, sc=None)
    for mode in (2, -1, 7):
        assert st(mode=mode) == INVALID_ARG and st(mode=mode, headroom=99, **later) == INVALID_ARG
        assert st(mode=mode, n=0) == INVALID_ARG
    for mode, headroom in ((0, -1), (0, 32), (1, 1), (1, 31)):
        assert st(mode=mode, headroom=headroom) == INVALID_ARG and st(mode=mode, headroom=headroom, **later) == INVALID_ARG
        assert st(mode=mode, headroom=headroom, n=0) == INVALID_ARG
    assert st(seed=None) == INVALID_ARG and st(seed=None, src=None, dst=None, sc=None) == INVALID_ARG
    assert st(seed=None, n=0) == INVALID_ARG and st(seed=None, n=0, src=None, dst=None, sc=None) == INVALID_ARG
    for off in range(1, 8):
        assert st(seed=seed + off) == INVALID_ARG and st(seed=seed + off, n=0) == INVALID_ARG
    for kw in (dict(src=None), dict(dst=None), dict(sc=None)):
        assert st(**kw) == INVALID_ARG and st(mode=1, **kw) == INVALID_ARG
    # count == 0 with a good mode, headroom and seed: success without device work, NULL pointers or not
    assert st(n=0) == 0 and st(n=0, mode=1) == 0 and st(n=0, headroom=31) == 0
    assert st(n=0, src=None, dst=None, sc=None) == 0
    assert call(None, wide, None, f8, 0, 0, 0, None, seed + 8, TOP << 32) == 0
    assert h.untouched()


def test_the_python_calls_raise_with_the_status_or_a_value_error():
    import torch

    import ftar
    h = Host()
    src, dst, sc, seed = h.ptrs()
    for bad in ("bogus", "Stochastic", None, 1):
        with pytest.raises(ValueError):
            ftar.mx_quantize(src, dst, sc, 64, "bf16", "f8e4m3", rounding=bad, seed=seed)
    with pytest.raises(ValueError):
        ftar.mx_quantize(src, dst, sc, 64, "bf16", "f8e4m3", rounding="stochastic")
    with pytest.raises(ValueError):
        ftar.mx_quantize(src, dst, sc, 64, "bf16", "f8e4m3", mode="fit", rounding="stochastic", seed=seed)
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_quantize(src, dst, sc, 64, "f32", "f16", rounding="stochastic", seed=seed)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_quantize(src, dst, sc, 64, "f32", "f8e5m2", rounding="stochastic", seed=seed + 4)
    assert e.value.status == INVALID_ARG
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_quantize(src, dst, sc, 64, "f32", "f8e5m2", mode="given", headroom=1, rounding="stochastic", seed=seed)
    assert e.value.status == INVALID_ARG
    ftar.mx_quantize(None, None, None, 0, "bf16", "f8e5m2", rounding="stochastic", seed=seed, offset=(1 << 64) - 1)
    a = torch.zeros(64, dtype=torch.bfloat16)
    b = torch.zeros(64, dtype=torch.float8_e4m3fn)
    s = torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ftar.mx_quantize_tensor(a, b, s, rounding="bogus")
    with pytest.raises(ValueError):
        ftar.mx_quantize_tensor(a, b, s, rounding="stochastic")
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1), 7,
                torch.zeros(1, dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError):
            ftar.mx_quantize_tensor(a, b, s, rounding="stochastic", seed=bad)
    with pytest.raises(ValueError):        # the tensors' own checks still run
        ftar.mx_quantize_tensor(a, b[:63], s, rounding="stochastic", seed=torch.zeros(1, dtype=torch.int64))
    e0 = torch.zeros(0, dtype=torch.float32)
    out = ftar.mx_quantize_tensor(e0, torch.zeros(0, dtype=torch.float8_e5m2), torch.zeros(0, dtype=torch.uint8),
                                  rounding="stochastic", seed=torch.zeros(1, dtype=torch.int64))
    assert out.numel() == 0
    assert h.untouched()


def test_mx_compress_state_rounding_arguments():
    import ftar.ddp as ddp
    for kw in (dict(rounding="bogus"), dict(rounding=None), dict(rounding="Stochastic"), dict(seed=1.5), dict(seed=True),
               dict(seed="7"), dict(headroom=32, rounding="stochastic")):
        with pytest.raises(ValueError):
            ddp.MxCompressState(None, **kw)
    s = ddp.MxCompressState(None)
    assert (s.rounding, s.seed, s.offset) == ("nearest", None, 0)
    s = ddp.MxCompressState(None, fmt="e5m2", headroom=2, rounding="stochastic", seed=5)
    assert (s.rounding, s.base_seed, s.seed, s.offset, s.headroom, s.wire_dtype) == ("stochastic", 5, None, 0, 2, "f8e5m2")
    assert "state.seed.add_(1)" in ddp.MxCompressState.__doc__ and "ftar_mx_quantize_sr" in ddp.mx_compress_hook.__doc__


# ---- the composed reference's own properties --------------------------------------------------------------
def finite_inputs(wide):
    """Every finite bf16 / fp16 encoding, or 2^18 random finite f32, once in ascending order of the encodings (a
    block's elements lie just under its peak) and once shuffled (they lie anywhere under it)."""
    rng = np.random.default_rng(5)
    if wide == "f32":
        x = rng.integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32)
        x = x[(x & np.uint32(0x7FFFFFFF)) < np.uint32(0x7F800000)]
    else:
        x = np.arange(65536, dtype=np.uint16)
        x = x[~cast_ref.nan_mask(wide, x) & ((x & 0x7FFF) != (0x7F80 if wide == "bf16" else 0x7C00))]
    return np.concatenate([np.sort(x), rng.permutation(x)])


def magnitude(enc):
    return (enc & 0x7F).astype(np.int64)


@pytest.mark.parametrize("headroom", [0, 3])
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_compute_blocks_hold_no_nan_or_inf_and_rne_lies_between_the_extreme_words(wide, f8, headroom):
    """Under the bytes ftar_mx_scales gives, for the words 0, 2^31 and 2^32 - 1: no stored element of a finite block
    is NaN or inf; U = 0 is truncation toward zero; the RNE encoding lies between the U = 0 and the U = 2^32 - 1
    encodings, which differ by at most one."""
    x = finite_inputs(wide)
    sc = mx_ref.scales(wide, f8, x, headroom)
    assert not (sc == 255).any()
    lo, mid, hi = (mx_sr_ref.quantize_words(wide, f8, x, sc, w) for w in (0, 1 << 31, TOP))
    rne = mx_ref.quantize(wide, f8, x, sc)
    top = 0x7C if f8 == "f8e5m2" else 0x7F
    for enc in (lo, mid, hi, rne):
        assert (magnitude(enc) < top).all(), "finite"
    assert ((lo & 0x80) == (hi & 0x80)).all() and ((lo & 0x80) == (mid & 0x80)).all()
    assert (magnitude(hi) - magnitude(lo) <= 1).all() and (magnitude(hi) >= magnitude(lo)).all()
    assert ((magnitude(lo) <= magnitude(mid)) & (magnitude(mid) <= magnitude(hi))).all()
    assert ((magnitude(lo) <= magnitude(rne)) & (magnitude(rne) <= magnitude(hi))).all()
    assert (magnitude(hi) > magnitude(lo)).any() and (magnitude(rne) > magnitude(lo)).any()
    per = mx_ref._per_element(sc, x.size)
    for s in np.unique(per)[::7]:
        m = per == s
        assert np.array_equal(lo[m], sr_ref.trunc_bits(f8, sr_ref.product_bits(wide, x[m], mx_ref.q_bits(s)))), s


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_representable_products_are_stored_unchanged_under_any_word(wide, f8):
    """Every finite fp8 value is exact in the three wide formats; at the scale byte 127 (q = 1) and at 120 with the
    value 2^-7 lower where that is still exact, the product is the value and every word stores its encoding."""
    enc = np.arange(256, dtype=np.uint8)
    enc = enc[(enc & 0x7F) < (0x7C if f8 == "f8e5m2" else 0x7F)]
    vals = cast_ref.widen_bits(f8, enc).view(np.float32)
    x = cast_ref.cast("f32", wide, vals.view(np.uint32)) if wide != "f32" else vals.view(np.uint32)
    assert np.array_equal(cast_ref.widen_bits(wide, x).view(np.float32), vals), "exact in the wide format"
    rng = np.random.default_rng(6)
    sc = np.full(mx_ref.nblocks(enc.size), 127, np.uint8)
    for w in (0, 1, 1 << 31, TOP, rng.integers(0, 1 << 32, enc.size, dtype=np.uint64).astype(np.uint32)):
        assert np.array_equal(mx_sr_ref.quantize_words(wide, f8, x, sc, w), enc)
    for seed in (0, SEED):
        assert np.array_equal(mx_sr_ref.quantize(wide, f8, x, sc, seed, 1 << 40), enc)


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_block_b_is_the_stochastic_scaled_cast_on_that_block_at_offset_plus_32b(wide, f8):
    n, offset = 4099, (1 << 32) - 100
    x = spread(wide, n, seed=3)
    x[70] = (0x7F800000 if wide == "f32" else 0x7F80 if wide == "bf16" else 0x7C00)      # block 2: s = 255, q = 1
    sc = mx_ref.scales(wide, f8, x, 1)
    assert sc[2] == 255 and (sc != 255).sum() == sc.size - 1
    got = mx_sr_ref.quantize(wide, f8, x, sc, SEED, offset)
    for b in range(mx_ref.nblocks(n)):
        blk = slice(32 * b, min(32 * b + 32, n))
        want = sr_ref.sr_cast(wide, f8, x[blk], mx_ref.q_bits(sc[b]), SEED, offset + 32 * b)
        assert cast_ref.same_bits(f8, got[blk], want), b
    assert cast_ref.same_bits(f8, got[64:96], sr_ref.sr_cast(wide, f8, x[64:96], None, SEED, offset + 64)), "the plain cast"
    # and the words array form on the generator's words
    w = sr_ref.words(SEED, sr_ref.indices(offset, n))
    assert np.array_equal(mx_sr_ref.quantize_words(wide, f8, x, sc, w), got)
    # a split at a multiple of 32 with the running offset
    cut = 32 * 17
    parts = np.concatenate([mx_sr_ref.quantize(wide, f8, x[:cut], sc[:17], SEED, offset),
                            mx_sr_ref.quantize(wide, f8, x[cut:], sc[17:], SEED, offset + cut)])
    assert np.array_equal(parts, got)


# ---- unbiasedness -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_the_average_over_seeds_is_four_times_closer_than_round_to_nearest(wide, f8):
    """spread's inputs: magnitudes within 5 binades of each block's top, n = 100 003, the scales ftar_mx_scales gives.
    The mean relative error of the dequantized payload averaged over the 64 seeds 100..163 must be under a quarter of
    the round-to-nearest payload's mean relative error: a zero-mean error averages down as 1 / sqrt(64) = 1 / 8 (its
    single-draw size is about 1.2 to 1.3 times RNE's), a biased one does not.  Measured on this reference: 0.15 to
    0.16 of the RNE error for all six pairs."""
    n = 100_003
    x = spread(wide, n, seed=9)
    sc = mx_ref.scales(wide, f8, x, 0)

    def values(enc):
        return mx_ref.dequantize(f8, "f32", enc, sc).view(np.float32).astype(np.float64)
    true = cast_ref.widen_bits(wide, x).view(np.float32).astype(np.float64)
    keep = true != 0                     # fp16's lowest blocks hold elements under its smallest subnormal: zeros
    assert keep.sum() > 0.95 * n
    rne = values(mx_ref.quantize(wide, f8, x, sc))
    total = np.zeros(n)
    for seed in range(100, 164):
        total += values(mx_sr_ref.quantize(wide, f8, x, sc, seed))
    rel_sr = float((np.abs(total / 64 - true)[keep] / np.abs(true[keep])).mean())
    rel_rne = float((np.abs(rne - true)[keep] / np.abs(true[keep])).mean())
    print(f"{wide}->{f8}: averaged SR {rel_sr:.3e}, RNE {rel_rne:.3e}, ratio {rel_sr / rel_rne:.3f}")
    assert rel_rne > 0 and rel_sr < rel_rne / 4, (rel_sr, rel_rne, rel_sr / rel_rne)
