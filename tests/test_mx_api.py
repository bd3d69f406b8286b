"""The MX block-scaled casts (include/ftar.h: ftar_mx_scales, ftar_mx_quantize, ftar_mx_dequantize) and the MX
gradient hook's host side, without a GPU: tests/mx_ref.py's integer scale rule held against torch.frexp on every
listed peak, the scaled peak's interval, q and d as inverses, every refusal in the header's order on host buffers
that must keep their bytes (nothing here may reach HIP), count == 0, the Python checks and the hook's ValueErrors."""
import ctypes

import numpy as np
import pytest

import cast_ref
import mx_ref

INVALID_ARG, UNSUPPORTED = 1, 2
WIDE_IDS = [cast_ref.ID[w] for w in cast_ref.WIDE]
F8_IDS = [cast_ref.ID[f] for f in cast_ref.F8]
MANTISSAS = (0, 0x5FFFFF, 0x600000, 0x600001, 0x7FFFFF)


def f32_peaks():
    """Every fp32 exponent field 0..254 x the mantissas around the 1.75 boundary."""
    return np.array([(e << 23) | m for e in range(255) for m in MANTISSAS], np.uint32)


def peak_lists():
    return {"f32": f32_peaks(), "bf16": np.arange(65536, dtype=np.uint16), "f16": np.arange(65536, dtype=np.uint16)}


def _values(dt, bits):
    """The encodings as an fp32 torch tensor (exact)."""
    import torch
    return torch.from_numpy(cast_ref.widen_bits(dt, bits).view(np.float32).copy())


# ---- the reference against torch ------------------------------------------------------------------------
@pytest.mark.parametrize("headroom", [0, 3])
@pytest.mark.parametrize("f8", cast_ref.F8)
@pytest.mark.parametrize("dt", cast_ref.WIDE)
def test_the_integer_rule_is_the_smallest_fitting_exponent_by_frexp(dt, f8, headroom):
    """peak = m x 2^e with m in [0.5, 1) (torch.frexp): peak x 2^(127 - s) <= 1.75 x 2^emax = 0.875 x 2^(emax + 1)
    holds from s = e + 126 - emax on if m <= 0.875, else from one more; clamped at 0, plus the headroom; a zero peak
    gives the headroom alone, an inf or a NaN 255."""
    import torch
    bits = peak_lists()[dt]
    x = _values(dt, bits).abs()
    m, e = torch.frexp(x)
    s = (e.to(torch.int64) + 126 - mx_ref.EMAX[f8] + (m > 0.875).to(torch.int64)).clamp(min=0)
    s = torch.where(x == 0, torch.zeros_like(s), s) + headroom
    s = torch.where(torch.isfinite(x), s.clamp(max=254), torch.full_like(s, 255))
    a = cast_ref.widen_bits(dt, bits) & np.uint32(0x7FFFFFFF)
    got = mx_ref.scale_of(a, f8, headroom)
    assert np.array_equal(got, s.numpy().astype(np.uint8)), np.flatnonzero(got != s.numpy())[:5]
    # one-element blocks through the block reduction give the same bytes
    assert np.array_equal(mx_ref.scales(dt, f8, bits[:1], headroom), got[:1])
    assert (got != 255).sum() > 1000 and (got == 255).any() == (dt != "f32")


@pytest.mark.parametrize("headroom", [0, 3])
@pytest.mark.parametrize("f8", cast_ref.F8)
@pytest.mark.parametrize("dt", cast_ref.WIDE)
def test_the_scaled_peak_fits_the_format_and_fills_its_top_binade(dt, f8, headroom):
    """Unless s was clamped at 0, peak x q(s) -- exact, a power of two times the peak -- lies in
    (0.875, 1.75] x 2^(emax - headroom), and what torch's cast stores for it is finite and lies in the closed
    interval (a product just above 0.875 x 2^emax rounds down onto it, which fp8 holds exactly)."""
    import torch
    bits = peak_lists()[dt]
    a = cast_ref.widen_bits(dt, bits) & np.uint32(0x7FFFFFFF)
    s = mx_ref.scale_of(a, f8, headroom)
    keep = (a != 0) & (a < mx_ref.F32_INF) & (s > headroom)
    assert keep.sum() > 1000
    x = _values(dt, bits).abs()[torch.from_numpy(keep)]
    q = torch.from_numpy(np.array([mx_ref.q_bits(v) for v in s[keep]], np.uint32).view(np.float32).copy())
    p = x * q
    top = mx_ref.MAX_FINITE[f8] * 2.0 ** -headroom
    assert bool(((p > top / 2) & (p <= top)).all())
    tt = {"f8e4m3": torch.float8_e4m3fn, "f8e5m2": torch.float8_e5m2}[f8]
    stored = p.to(tt).to(torch.float32)
    assert bool(torch.isfinite(stored).all()) and bool(((stored >= top / 2) & (stored <= top)).all())
    # the reference's payload is that cast
    for i in np.flatnonzero(keep)[:: max(1, int(keep.sum()) // 64)]:
        enc = mx_ref.quantize(dt, f8, bits[i:i + 1], s[i:i + 1])
        assert cast_ref.same_bits(f8, enc, cast_ref.torch_cast(dt, f8, bits[i:i + 1], mx_ref.q_bits(s[i])))


def test_q_and_d_are_exact_inverses():
    for s in range(1, 254):
        q = np.array([mx_ref.q_bits(s)], np.uint32).view(np.float32)[0]
        d = np.array([mx_ref.d_bits(s)], np.uint32).view(np.float32)[0]
        assert q * d == np.float32(1.0) and float(d) == 2.0 ** (s - 127) and float(q) == 2.0 ** (127 - s)
    assert mx_ref.q_bits(254) == 0x00400000 and mx_ref.d_bits(0) == 0x00400000        # 2^-127, subnormal
    assert mx_ref.q_bits(0) == 0x7F000000 and mx_ref.d_bits(254) == 0x7F000000        # 2^127
    assert mx_ref.q_bits(255) == cast_ref.ONE
    assert [mx_ref.nblocks(n) for n in (0, 1, 32, 33, 64)] == [0, 1, 1, 2, 2]


def test_zero_and_nan_blocks_of_the_reference():
    x = np.zeros(70, np.uint16)
    x[3] = 0x8000
    x[40] = 0x7F80                                   # +inf in block 1
    assert mx_ref.scales("bf16", "f8e4m3", x, 5).tolist() == [5, 255, 5]
    x[69] = 0x3F80                                   # 1.0 in the partial block: 127 - 8
    sc = mx_ref.scales("bf16", "f8e4m3", x)
    assert sc.tolist() == [0, 255, 119]
    pay = mx_ref.quantize("bf16", "f8e4m3", x, sc)
    assert pay[3] == 0x80 and pay[69] == 0x78 and cast_ref.nan_mask("f8e4m3", pay).tolist() == [i == 40 for i in range(70)]
    back = mx_ref.dequantize("f8e4m3", "bf16", pay, sc)
    assert cast_ref.nan_mask("bf16", back).tolist() == [32 <= i < 64 for i in range(70)]
    assert back[69] == 0x3F80 and back[3] == 0x8000


# ---- the entry points' refusals -------------------------------------------------------------------------
class Host:
    """Host buffers standing in for device memory: a refused call must leave every byte."""

    def __init__(self):
        self.src = (ctypes.c_ubyte * 512)(*([0x5A] * 512))
        self.dst = (ctypes.c_ubyte * 512)(*([0xA5] * 512))
        self.sc = (ctypes.c_ubyte * 64)(*([0xC3] * 64))

    def ptrs(self):
        return ctypes.addressof(self.src), ctypes.addressof(self.dst), ctypes.addressof(self.sc)

    def untouched(self):
        return bytes(self.src) == b"\x5a" * 512 and bytes(self.dst) == b"\xa5" * 512 and bytes(self.sc) == b"\xc3" * 64


def _scales(src, sdt, f8, n, headroom, sc):
    import ftar
    return ftar.lib().ftar_mx_scales(src, sdt, f8, n, headroom, sc, None)


def _quant(src, sdt, dst, ddt, n, mode, headroom, sc):
    import ftar
    return ftar.lib().ftar_mx_quantize(src, sdt, dst, ddt, n, mode, headroom, sc, None)


def _dequant(src, sdt, sc, dst, ddt, n):
    import ftar
    return ftar.lib().ftar_mx_dequantize(src, sdt, sc, dst, ddt, n, None)


def test_the_symbols_are_exported_and_declared():
    import os

    import ftar
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ftar.h")).read()
    for name in ("ftar_mx_scales", "ftar_mx_quantize", "ftar_mx_dequantize"):
        assert hasattr(ftar.lib(), name) and name + "(" in header
    assert "#define FTAR_MX_BLOCK 32" in header and "FTAR_MX_COMPUTE = 0, FTAR_MX_GIVEN = 1" in header
    assert ftar.MX_BLOCK == 32 and ftar.MX_MODE == {"compute": 0, "given": 1}
    assert [ftar.mx_nblocks(n) for n in (0, 1, 31, 32, 33, 100_003)] == [0, 1, 1, 1, 2, 3126]


def test_every_pair_but_the_six_plus_six_is_refused_first():
    """All dtype ids 0..13 squared: an unsupported pair is status 2 whatever else is wrong with the call (NULL
    pointers, a bad mode, a bad headroom, count 0); a supported one gets past that check."""
    h = Host()
    src, dst, sc = h.ptrs()
    quant, dequant, scal = [], [], []
    for a in range(14):
        for b in range(14):
            st = _quant(None, a, None, b, 1, 0, 0, None)
            assert st in (INVALID_ARG, UNSUPPORTED)
            if st == INVALID_ARG:
                quant.append((a, b))
            else:
                assert _quant(src, a, dst, b, 64, 7, 99, sc) == UNSUPPORTED and _quant(src, a, dst, b, 0, 0, 0, sc) == UNSUPPORTED
            st = _dequant(None, a, None, None, b, 1)
            assert st in (INVALID_ARG, UNSUPPORTED)
            if st == INVALID_ARG:
                dequant.append((a, b))
            else:
                assert _dequant(src, a, sc, dst, b, 0) == UNSUPPORTED
            st = _scales(None, a, b, 1, 0, None)
            assert st in (INVALID_ARG, UNSUPPORTED)
            if st == INVALID_ARG:
                scal.append((a, b))
            else:
                assert _scales(src, a, b, 64, -1, sc) == UNSUPPORTED and _scales(src, a, b, 0, 0, sc) == UNSUPPORTED
    six = sorted((w, f) for w in WIDE_IDS for f in F8_IDS)
    assert sorted(quant) == six and sorted(scal) == six and sorted(dequant) == sorted((f, w) for w, f in six)
    for bad in (-1, 11, 14, 255):
        assert _quant(src, bad, dst, 12, 64, 0, 0, sc) == UNSUPPORTED and _dequant(src, 12, sc, dst, bad, 64) == UNSUPPORTED
    assert h.untouched()


@pytest.mark.parametrize("f8", F8_IDS)
@pytest.mark.parametrize("wide", WIDE_IDS)
def test_invalid_arguments_leave_the_buffers(wide, f8):
    h = Host()
    src, dst, sc = h.ptrs()
    for args in ((None, wide, dst, f8, 64, 0, 0, sc), (src, wide, None, f8, 64, 0, 0, sc), (src, wide, dst, f8, 64, 0, 0, None),
                 (src, wide, dst, f8, 64, 2, 0, sc), (src, wide, dst, f8, 64, -1, 0, sc),           # the mode
                 (src, wide, dst, f8, 64, 0, -1, sc), (src, wide, dst, f8, 64, 0, 32, sc),           # the headroom
                 (src, wide, dst, f8, 64, 1, 1, sc), (src, wide, dst, f8, 64, 1, 31, sc),            # GIVEN takes none
                 (src, wide, dst, f8, 0, 2, 0, sc), (src, wide, dst, f8, 0, 0, 32, sc), (src, wide, dst, f8, 0, 1, 1, sc)):
        assert _quant(*args) == INVALID_ARG, args
    for args in ((None, wide, f8, 64, 0, sc), (src, wide, f8, 64, 0, None), (src, wide, f8, 64, -1, sc),
                 (src, wide, f8, 64, 32, sc), (src, wide, f8, 0, 32, sc)):
        assert _scales(*args) == INVALID_ARG, args
    for args in ((None, f8, sc, dst, wide, 64), (src, f8, None, dst, wide, 64), (src, f8, sc, None, wide, 64)):
        assert _dequant(*args) == INVALID_ARG, args
    # count == 0 succeeds and writes nothing, NULL pointers or not, in both modes and with a headroom
    assert _quant(None, wide, None, f8, 0, 0, 0, None) == 0 and _quant(src, wide, dst, f8, 0, 1, 0, sc) == 0
    assert _quant(src, wide, dst, f8, 0, 0, 31, sc) == 0
    assert _scales(None, wide, f8, 0, 0, None) == 0 and _scales(src, wide, f8, 0, 31, sc) == 0
    assert _dequant(None, f8, None, None, wide, 0) == 0 and _dequant(src, f8, sc, dst, wide, 0) == 0
    assert h.untouched()


def test_the_python_calls_raise_with_the_status_or_a_value_error():
    import ftar
    h = Host()
    src, dst, sc = h.ptrs()
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_quantize(src, dst, sc, 64, "f32", "f16")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_dequantize(src, sc, dst, 64, "bf16", "f8e4m3")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_scales(src, sc, 64, "f64", "f8e4m3")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_quantize(src, dst, sc, 64, "bf16", "f8e5m2", mode="given", headroom=1)
    assert e.value.status == INVALID_ARG
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_scales(src, None, 64, "bf16", "f8e5m2")
    assert e.value.status == INVALID_ARG
    for mode in ("fit", 0, None, "GIVEN"):
        with pytest.raises(ValueError):
            ftar.mx_quantize(src, dst, sc, 64, "bf16", "f8e5m2", mode=mode)
    ftar.mx_quantize(None, None, None, 0, "bf16", "f8e5m2")
    ftar.mx_dequantize(None, None, None, 0, "f8e5m2", "f16")
    ftar.mx_scales(None, None, 0, "f32", "f8e4m3", headroom=31)
    assert h.untouched()


def test_the_tensor_forms_value_errors():
    import torch

    import ftar
    a = torch.zeros(64, dtype=torch.bfloat16)
    b = torch.zeros(64, dtype=torch.float8_e4m3fn)
    sc = torch.zeros(2, dtype=torch.uint8)
    bad = [(a, b[:63], sc),                                                            # numel
           (a, b, sc[:1]),                                                             # too few scale bytes
           (a, b, torch.zeros(2, dtype=torch.int8)), (a, b, torch.zeros(2)),           # scales' dtype
           (torch.zeros(8, 16, dtype=torch.bfloat16).t()[:, :4], b, sc),               # contiguity
           (a, b, torch.zeros(4, dtype=torch.uint8)[::2]),
           (a, b.to("meta"), sc), (a, b, sc.to("meta"))]                               # device
    for w, f, s in bad:
        with pytest.raises(ValueError):
            ftar.mx_quantize_tensor(w, f, s)
        with pytest.raises(ValueError):
            ftar.mx_dequantize_tensor(f, s, w)
    with pytest.raises(ValueError):
        ftar.mx_quantize_tensor(a, b, sc, mode="fit")
    with pytest.raises(ftar.FtarError) as e:        # the pair itself: the library's refusal
        ftar.mx_quantize_tensor(a, torch.zeros(64, dtype=torch.float16), sc)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_dequantize_tensor(a, sc, torch.zeros(64))
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.mx_quantize_tensor(a, b, sc, mode="given", headroom=2)
    assert e.value.status == INVALID_ARG
    e0 = torch.zeros(0, dtype=torch.float32)
    assert ftar.mx_quantize_tensor(e0, torch.zeros(0, dtype=torch.float8_e5m2), torch.zeros(0, dtype=torch.uint8)).numel() == 0


# ---- the hook's host side -------------------------------------------------------------------------------
def test_mx_compress_state_argument_checks():
    import ftar.ddp as ddp
    for kw in (dict(fmt="e3m4"), dict(fmt="f8e4m3"), dict(headroom=-1), dict(headroom=32), dict(headroom=1.0),
               dict(headroom=True)):
        with pytest.raises(ValueError):
            ddp.MxCompressState(None, **kw)
    s = ddp.MxCompressState(None, fmt="e5m2", topo="2,2", headroom=2)
    assert (s.fmt, s.wire_dtype, s.topo, s.lonely, s.headroom, s.calls) == ("e5m2", "f8e5m2", "2,2", 0, 2, 0)
    assert not hasattr(s, "update_scale") and not hasattr(s, "amax")
    with pytest.raises(RuntimeError):
        s.found_inf()
    s.reset()        # a no-op before the first bucket


def test_mx_compress_hook_refuses_other_buckets_before_any_device_work():
    import torch

    import ftar.ddp as ddp

    class Bucket:
        def __init__(self, t):
            self.t = t

        def buffer(self):
            return self.t
    s = ddp.MxCompressState(None)
    for dt in (torch.int32, torch.float64, torch.float8_e4m3fn, torch.uint8):
        with pytest.raises(ValueError):
            ddp.mx_compress_hook(s, Bucket(torch.zeros(64).to(dt)))
    with pytest.raises(ValueError):
        ddp.mx_compress_hook(s, Bucket(torch.zeros(8, 16).t()))
    assert s._wire is None and s._inf is None and s.calls == 0
    for point in ("cannot overflow at headroom=0", "headroom >= ceil(log2 P)", "n + 2 * ceil(n / 32) bytes"):
        assert point in ddp.mx_compress_hook.__doc__
