"""The amax entry points (include/ftar.h: ftar_reduce_amax, ftar_allreduce_amax, ftar_allreduce_amax_group) at
the API surface, without a GPU: the symbols, every refusal that must come before any device work (fake pointers:
nothing may touch HIP), the self-checks of the CPU expectation (tests/amax_ref.py) that tests/test_gpu_amax.py
compares against, and the DDP hook's argument check."""
import ctypes

import numpy as np
import pytest

import amax_ref

INVALID_ARG, UNSUPPORTED = 1, 2
REFUSED_DTYPES = ["i32", "f64", "u8", "i64", "bool", "u16"]


def test_the_three_symbols_exist():
    import ftar
    for name in ("ftar_reduce_amax", "ftar_allreduce_amax", "ftar_allreduce_amax_group"):
        assert hasattr(ftar.lib(), name), name


@pytest.mark.parametrize("dt", REFUSED_DTYPES)
def test_reduce_amax_refuses_other_dtypes_before_any_device_work(dt):
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048], 4096, 10, dt, amax=8192)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048, 4096, 8192], 16384, 10, dt, scale=0.25, shape=[2, 2], amax=32768)
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_reduce_amax_refuses_a_null_or_misaligned_amax_a_bad_scale_and_a_bad_shape(dt):
    import ftar
    lib = ftar.lib()
    arr = (ctypes.c_void_p * 2)(1024, 2048)
    sh = (ctypes.c_int * 1)()
    assert lib.ftar_reduce_amax(arr, 2, 4096, 10, ftar.DTYPE[dt], 1.0, sh, 0, None, None) == INVALID_ARG
    assert lib.ftar_reduce_amax(arr, 2, 4096, 10, ftar.DTYPE[dt], 1.0, sh, 0, 8194, None) == INVALID_ARG
    for scale in (float("inf"), float("nan")):
        with pytest.raises(ftar.FtarError) as e:
            ftar.reduce([1024, 2048], 4096, 10, dt, scale=scale, amax=8192)
        assert e.value.status == INVALID_ARG
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048, 4096, 8192], 16384, 10, dt, shape=[2, 3], amax=32768)
    assert e.value.status == INVALID_ARG


def test_amax_goes_with_sum_only():
    import ftar
    with pytest.raises(ValueError):
        ftar.reduce([1024, 2048], 4096, 10, "f32", "max", amax=8192)


@pytest.mark.parametrize("dt,op", [(dt, "sum") for dt in REFUSED_DTYPES] +
                         [("f32", "max"), ("f16", "min"), ("bf16", "band"), ("f8e4m3", "max")])
def test_allreduce_amax_refuses_dtypes_and_ops_before_it_looks_at_anything_else(dt, op):
    """No communicator and fake buffers: the refusal is the first thing the call decides."""
    import ftar
    lib = ftar.lib()
    assert lib.ftar_allreduce_amax(1024, 2048, 10, ftar.DTYPE[dt], ftar.OP[op], None, None, 4096, None) == UNSUPPORTED
    P = 2
    bufs = (ctypes.c_void_p * P)(1024, 2048)
    comms = (ctypes.c_void_p * P)(64, 128)         # never dereferenced: refused first
    am = (ctypes.c_void_p * P)(4096, 8192)
    assert lib.ftar_allreduce_amax_group(None, bufs, 10, ftar.DTYPE[dt], ftar.OP[op], None, comms, P, am,
                                         None) == UNSUPPORTED


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_allreduce_amax_refuses_a_null_amax(dt, op):
    import ftar
    lib = ftar.lib()
    assert lib.ftar_allreduce_amax(1024, 2048, 10, ftar.DTYPE[dt], ftar.OP[op], None, None, None, None) == INVALID_ARG
    P = 2
    bufs = (ctypes.c_void_p * P)(1024, 2048)
    comms = (ctypes.c_void_p * P)(64, 128)
    am = (ctypes.c_void_p * P)(4096, None)
    assert lib.ftar_allreduce_amax_group(None, bufs, 10, ftar.DTYPE[dt], ftar.OP[op], None, comms, P, am,
                                         None) == INVALID_ARG
    assert lib.ftar_allreduce_amax_group(None, bufs, 10, ftar.DTYPE[dt], ftar.OP[op], None, comms, P, None,
                                         None) == INVALID_ARG


# ---- the expectation's self-checks --------------------------------------------------------------------------
def _torch_absmax_bits(dt, enc):
    """fp32 bits of torch's abs().max() over the non-NaN encodings `enc`."""
    import torch

    import avg_ref
    import f8_ref
    t = f8_ref._t(dt, enc) if amax_ref.is_f8(dt) else avg_ref._t(dt, enc)
    m = t.to(torch.float32).abs().max()
    return int(m.view(torch.int32).numpy().view(np.uint32))


@pytest.mark.parametrize("dt", ["f16", "bf16", "f8e4m3", "f8e5m2"])
def test_amax_ref_agrees_with_torch_on_every_encoding(dt):
    """All 2^16 (2^8) encodings: every single one, every prefix maximum of a shuffled order, and NaNs apart."""
    u = amax_ref.storage(dt)
    enc = np.arange(1 << (8 * np.dtype(u).itemsize), dtype=np.uint32).astype(u)
    nan = amax_ref.nan_mask(dt, enc)
    assert nan.any()
    for e in enc[nan][:: max(1, int(nan.sum()) // 64)]:
        assert amax_ref.amax_bits(dt, np.array([0, e, 1], u)) == amax_ref.NAN
    fin = enc[~nan]
    import torch

    import avg_ref
    import f8_ref
    t = (f8_ref._t(dt, fin) if amax_ref.is_f8(dt) else avg_ref._t(dt, fin)).to(torch.float32).abs()
    want_each = t.view(torch.int32).numpy().view(np.uint32)
    key = amax_ref.keys(dt, fin)
    # widening is monotone in the key, so the per-element words are amax_bits of one-element arrays
    order = np.argsort(key, kind="stable")
    assert np.all(np.diff(want_each[order].astype(np.int64)) >= 0), "the key order is the order of |value|"
    for e, w in list(zip(fin, want_each))[:: 97 if fin.size > 256 else 1]:
        assert amax_ref.amax_bits(dt, np.array([e], u)) == int(w)
    rng = np.random.default_rng(5)
    for _ in range(32):
        pick = rng.choice(fin, size=int(rng.integers(1, 200)))
        assert amax_ref.amax_bits(dt, pick) == _torch_absmax_bits(dt, pick)
    assert amax_ref.amax_bits(dt, fin) == _torch_absmax_bits(dt, fin)


def test_amax_ref_zeros_empty_and_matches():
    for dt in amax_ref.DTYPES:
        u = amax_ref.storage(dt)
        sign = 1 << (8 * np.dtype(u).itemsize - 1)
        assert amax_ref.amax_bits(dt, np.array([0, sign, 0], u)) == 0
        assert amax_ref.amax_bits(dt, np.array([], u)) == 0
    assert amax_ref.matches(0x7FC00000, amax_ref.NAN) and amax_ref.matches(0x7F800001, amax_ref.NAN)
    assert not amax_ref.matches(0x7F800000, amax_ref.NAN) and not amax_ref.matches(0, amax_ref.NAN)
    assert amax_ref.matches(0x44800000, 0x44800000) and not amax_ref.matches(0x44800001, 0x44800000)


@pytest.mark.parametrize("k", [2, 8, 17])
@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_the_peak_wins_in_every_reduce_expectation(dt, k):
    """n = 4099, r = 1 and r = 1 / k: finite, and the peak at least 3x over the runner-up (asserted strictly by
    checked(); the margin is what the test design relies on)."""
    n = 4099
    for scale in (1.0, float(np.float32(1) / np.float32(k))):
        ins, want, word = amax_ref.reduce_case(dt, k, n, scale, 1234)
        key = amax_ref.keys(dt, want).astype(np.int64)
        top = amax_ref.widen(dt, int(key[1234]))
        second = amax_ref.widen(dt, int(np.delete(key, 1234).max()))
        f = lambda b: float(np.array([b], np.uint32).view(np.float32)[0])  # noqa: E731
        assert word == top and f(top) >= 3 * f(second), (dt, k, scale, f(top), f(second))


@pytest.mark.parametrize("P,topo", [(2, "1"), (3, "3"), (4, "2,2"), (6, "2,3"), (8, "1"), (8, "2,2,2")])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_the_schedules_with_r_passed_in_are_avg_refs(dt, P, topo):
    """amax_ref.ring / tree (the root's r an argument, so SUM is r = 1) against avg_ref's own at r = 1 / P, on
    avg_ref's inputs (NaN and inf lanes included), and against f16_minmax_ref's fp16 SUM schedules at r = 1."""
    import avg_ref
    import f16_minmax_ref as ref
    n = 4099
    ins, want = avg_ref.allreduce_case(dt, P, topo, n)
    assert ref.same_bits(dt, amax_ref.schedule(dt, ins, topo, "avg"), want)
    if dt == "f16":
        ins, want = ref.f16_allreduce_case(P, topo, n)
        assert ref.same_bits(dt, amax_ref.schedule(dt, ins, topo, "sum"), want)


def test_hook_rejects_a_bad_track_amax():
    import ftar.ddp
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError):
            ftar.ddp.HookState(None, track_amax=bad)
    s = ftar.ddp.HookState(None, track_amax=True)
    assert s.track_amax is True and s.amax is None
    assert ftar.ddp.HookState(None).track_amax is False
    with pytest.raises(RuntimeError):
        ftar.ddp.HookState(None).found_inf()
