"""The scaled casts (include/ftar.h: ftar_cast_scaled) and the fp8 gradient hook's host side, without a GPU: the
symbol, every refusal (with fake pointers: nothing here may reach HIP), the Python checks, tests/cast_ref.py held
against torch's own casts on the CPU, and the scale policy of ftar.ddp.Fp8CompressState on CPU tensors."""
import ctypes

import numpy as np
import pytest

import cast_ref

INVALID_ARG, UNSUPPORTED = 1, 2
FAKE_SRC, FAKE_DST, FAKE_WORD = 0x10000, 0x20000, 0x30000
NAMES = {6: "f32", 9: "bf16", 10: "f16", 12: "f8e4m3", 13: "f8e5m2"}


def call(src, sdt, dst, ddt, count, scale=None, amax=None):
    import ftar
    return ftar.lib().ftar_cast_scaled(src, sdt, dst, ddt, count, scale, amax, None)


def test_the_symbol_is_exported_and_declared():
    import os

    import ftar
    assert hasattr(ftar.lib(), "ftar_cast_scaled")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "ftar_cast_scaled(" in open(os.path.join(root, "include", "ftar.h")).read()


def test_every_pair_but_the_twelve_is_refused_first():
    """All dtype ids 0..13 squared, NULL src and dst with count 1: an unsupported pair is status 2 whatever the
    pointers; a supported one gets past that check and is refused for its NULL pointers, status 1."""
    passed = []
    for s in range(14):
        for d in range(14):
            st = call(None, s, None, d, 1)
            assert st in (INVALID_ARG, UNSUPPORTED), (s, d, st)
            if st == INVALID_ARG:
                passed.append((s, d))
            else:   # ... and before anything else: with fake pointers and misaligned words too
                assert call(FAKE_SRC, s, FAKE_DST, d, 1, FAKE_WORD + 1, FAKE_WORD + 2) == UNSUPPORTED
                assert call(FAKE_SRC, s, FAKE_DST, d, 0) == UNSUPPORTED
    want = sorted((cast_ref.ID[a], cast_ref.ID[b]) for a, b in cast_ref.PAIRS)
    assert len(want) == 12 and sorted(passed) == want
    for s in (-1, 14, 11, 255):
        assert call(FAKE_SRC, s, FAKE_DST, 12, 1) == UNSUPPORTED and call(FAKE_SRC, 12, FAKE_DST, s, 1) == UNSUPPORTED


@pytest.mark.parametrize("sdt,ddt", [(cast_ref.ID[a], cast_ref.ID[b]) for a, b in cast_ref.PAIRS])
def test_null_and_misaligned_arguments(sdt, ddt):
    assert call(None, sdt, FAKE_DST, ddt, 5) == INVALID_ARG
    assert call(FAKE_SRC, sdt, None, ddt, 5) == INVALID_ARG
    for off in (1, 2, 3):
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 5, FAKE_WORD + off, None) == INVALID_ARG
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 5, None, FAKE_WORD + off) == INVALID_ARG
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 0, FAKE_WORD + off, None) == INVALID_ARG
    assert call(None, sdt, None, ddt, 0) == 0        # nothing to do, no amax: success without device work


def test_python_cast_scaled_raises_with_the_status():
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.cast_scaled(FAKE_SRC, FAKE_DST, 4, "f32", "f16")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.cast_scaled(FAKE_SRC, FAKE_DST, 4, "f64", "f8e4m3")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.cast_scaled(None, FAKE_DST, 4, "bf16", "f8e5m2")
    assert e.value.status == INVALID_ARG


def test_cast_scaled_tensor_value_errors():
    import torch

    import ftar
    a = torch.zeros(8, dtype=torch.bfloat16)
    b = torch.zeros(8, dtype=torch.float8_e4m3fn)
    one = torch.ones(1)
    with pytest.raises(ValueError):
        ftar.cast_scaled_tensor(a, b[:7])
    with pytest.raises(ValueError):
        ftar.cast_scaled_tensor(torch.zeros(4, 4, dtype=torch.bfloat16).t(), torch.zeros(16, dtype=torch.float8_e4m3fn))
    with pytest.raises(ValueError):
        ftar.cast_scaled_tensor(a, b.to("meta"))
    for bad in (torch.ones(2), torch.ones(1, dtype=torch.float64), torch.ones(1, device="meta"), 1.0):
        with pytest.raises(ValueError):
            ftar.cast_scaled_tensor(a, b, scale=bad)
        with pytest.raises(ValueError):
            ftar.cast_scaled_tensor(a, b, scale=one, amax=bad)
    with pytest.raises(ftar.FtarError) as e:        # the pair itself: the library's refusal
        ftar.cast_scaled_tensor(a, torch.zeros(8, dtype=torch.float16))
    assert e.value.status == UNSUPPORTED
    assert ftar._dt(torch.float8_e4m3fn) == 12 and ftar._dt(torch.float8_e5m2) == 13


# ---- cast_ref against torch ---------------------------------------------------------------------------
def _same(dt, got, want, what):
    assert cast_ref.same_bits(dt, got, want), (what, cast_ref.first_diff(dt, got, want))


@pytest.mark.parametrize("r", cast_ref.SCALES + tuple(cast_ref.ODD_SCALES.values()), ids=hex)
@pytest.mark.parametrize("dst", cast_ref.F8)
@pytest.mark.parametrize("src", ["bf16", "f16"])
def test_ref_quantizes_every_16_bit_encoding_as_torch_does(src, dst, r):
    bits = np.arange(65536, dtype=np.uint16)
    _same(dst, cast_ref.cast(src, dst, bits, r), cast_ref.torch_cast(src, dst, bits, r), (src, dst, hex(r)))


@pytest.mark.parametrize("r", cast_ref.SCALES + tuple(cast_ref.ODD_SCALES.values()), ids=hex)
@pytest.mark.parametrize("dst", cast_ref.WIDE)
@pytest.mark.parametrize("src", cast_ref.F8)
def test_ref_dequantizes_every_fp8_encoding_as_torch_does(src, dst, r):
    bits = np.arange(256, dtype=np.uint8)
    _same(dst, cast_ref.cast(src, dst, bits, r), cast_ref.torch_cast(src, dst, bits, r), (src, dst, hex(r)))


def f32_sweep(low):
    """All 2^16 high halves over one low half."""
    return (np.arange(65536, dtype=np.uint32) << np.uint32(16)) | np.uint32(low)


@pytest.mark.parametrize("low", [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], ids=hex)
@pytest.mark.parametrize("dst", cast_ref.F8)
def test_ref_quantizes_f32_as_torch_does(dst, low):
    bits = f32_sweep(low)
    for r in cast_ref.SCALES:
        _same(dst, cast_ref.cast("f32", dst, bits, r), cast_ref.torch_cast("f32", dst, bits, r), (dst, hex(r)))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_the_16_bit_integer_rne_is_torchs_cast(dt):
    """rne16_bits on every high half over the low halves around the ties, and on random floats."""
    import torch
    tt = {"bf16": torch.bfloat16, "f16": torch.float16}[dt]
    rng = np.random.default_rng(5)
    sets = [f32_sweep(low) for low in (0, 1, 0x0FFF, 0x1000, 0x1001, 0x1FFF, 0x2000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)]
    sets.append(rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32))
    for u in sets:
        want = torch.from_numpy(u.view(np.float32).copy()).to(tt).view(torch.int16).numpy().view(np.uint16)
        _same(dt, cast_ref.rne16_bits(dt, u), want, dt)


@pytest.mark.parametrize("src,dst", cast_ref.witness_pairs() + [("f32", "f16")])
def test_witnesses_round_differently_once_than_twice_and_torch_rounds_twice(src, dst):
    ws = cast_ref.witnesses(dst, src)
    assert len(ws) >= 3
    for x, r, twice, once in ws:
        assert once != twice
        bits = np.array([x], cast_ref.storage(src))
        assert int(cast_ref.cast(src, dst, bits, r)[0]) == twice
        assert int(cast_ref.torch_cast(src, dst, bits, r)[0]) == twice


def test_the_fp16_witness_worked_out_by_hand():
    """x = (2 + 9/1024 + 2^-24) / 3 and r = 3: fp16 0x4004 in two roundings, 0x4005 in one."""
    from fractions import Fraction
    x = (2 + Fraction(9, 1024) + Fraction(1, 1 << 24)) / 3
    xe = cast_ref.enc_of("f32", x)
    assert xe is not None
    exact = cast_ref.frac_of("f32", xe) * 3
    assert cast_ref.round_frac("f16", exact) == 0x4005
    assert cast_ref.round_frac("f16", cast_ref.frac_of("f32", cast_ref.round_frac("f32", exact))) == 0x4004
    assert int(cast_ref.torch_cast("f32", "f16", np.array([xe], np.uint32), 0x40400000)[0]) == 0x4004
    assert int(cast_ref.rne16_bits("f16", cast_ref.cast("f32", "f32", np.array([xe], np.uint32), 0x40400000))[0]) == 0x4004


# ---- the scale policy ---------------------------------------------------------------------------------
def _f(x):
    import torch
    return torch.tensor([x], dtype=torch.float32)


def _is_pow2(t):
    import torch
    m, _ = torch.frexp(t)
    return bool((m == 0.5).all())


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 10, 2.0 ** -20])
@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("fmt,fmax", [("e4m3", 448.0), ("e5m2", 57344.0)])
def test_next_fp8_scale_around_a_power_of_two_boundary(fmt, fmax, margin, scale):
    """amax exactly at the target keeps the scale; one fp32 ulp under it too; one ulp over it halves the scale."""
    import torch

    from ftar.ddp import next_fp8_scale
    target = np.float32(fmax * 2.0 ** -margin)
    at, under, over = target, np.nextafter(target, np.float32(0)), np.nextafter(target, np.float32(np.inf))
    for amax, want in ((at, scale), (under, scale), (over, scale / 2), (at / 2, scale * 2),
                       (np.nextafter(at / 2, np.float32(np.inf)), scale), (at * 4, scale / 4)):
        got = next_fp8_scale(_f(scale), _f(float(amax)), fmt, margin, 0.5)
        assert got.dtype == torch.float32 and got.shape == (1,)
        assert float(got) == want, (fmt, margin, scale, float(amax), float(got), want)
        assert _is_pow2(got) and float(got * (1.0 / got)) == 1.0
        # the largest power of two that keeps the unscaled amax times it at or under the target
        unscaled = float(amax) / scale
        assert float(got) * unscaled <= float(target) < 2 * float(got) * unscaled


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_next_fp8_scale_specials(fmt):
    from ftar.ddp import next_fp8_scale
    for scale in (1.0, 64.0, 2.0 ** -30):
        assert float(next_fp8_scale(_f(scale), _f(0.0), fmt, 1, 0.5)) == scale
        for bad in (float("inf"), float("nan")):
            assert float(next_fp8_scale(_f(scale), _f(bad), fmt, 1, 0.5)) == scale / 2
            got = next_fp8_scale(_f(scale), _f(bad), fmt, 1, 0.3)       # 0.3 x scale, down to a power of two
            assert float(got) == scale / 4 and _is_pow2(got)
    # clamped to fp32's normal powers of two
    assert float(next_fp8_scale(_f(2.0 ** -126), _f(float("inf")), fmt, 1, 0.5)) == 2.0 ** -126
    assert float(next_fp8_scale(_f(1.0), _f(1e-45), fmt, 0, 0.5)) == 2.0 ** 127
    assert float(next_fp8_scale(_f(2.0 ** -126), _f(3e38), fmt, 0, 0.5)) == 2.0 ** -126
    with pytest.raises(ValueError):
        next_fp8_scale(_f(1.0), _f(1.0), "e3m4")


def test_fp8_compress_state_argument_checks():
    import ftar.ddp as ddp
    for kw in (dict(fmt="e3m4"), dict(fmt="f8e4m3"), dict(margin=-1), dict(margin=0.5), dict(margin=True),
               dict(backoff=0.0), dict(backoff=1.0), dict(backoff="half")):
        with pytest.raises(ValueError):
            ddp.Fp8CompressState(None, **kw)
    s = ddp.Fp8CompressState(None, fmt="e5m2", topo="2,2", margin=0, backoff=0.25)
    assert (s.fmt, s.wire_dtype, s.topo, s.margin, s.backoff, s.calls) == ("e5m2", "f8e5m2", "2,2", 0, 0.25, 0)
    assert s.scale is None and s.amax is None
    for fn in (s.found_inf, s.update_scale):
        with pytest.raises(RuntimeError):
            fn()
    s.reset_amax()      # a no-op before the first bucket, as on HookState


def test_fp8_compress_hook_refuses_other_buckets_before_any_device_work():
    import torch

    import ftar.ddp as ddp

    class Bucket:
        def __init__(self, t):
            self.t = t

        def buffer(self):
            return self.t
    s = ddp.Fp8CompressState(None)
    for dt in (torch.int32, torch.float64, torch.float8_e4m3fn, torch.uint8):
        with pytest.raises(ValueError):
            ddp.fp8_compress_hook(s, Bucket(torch.zeros(8).to(dt)))
    assert s.scale is None and s.calls == 0
