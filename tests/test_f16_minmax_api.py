"""The fp16 dtype and the MAX / MIN ops at the API surface, without a GPU: the enum tables, what is refused
before any device work, the plan flag the fp16 ring fold depends on, and the self-checks of the CPU
expectations (tests/f16_minmax_ref.py) that the GPU tests in tests/test_gpu_f16_minmax.py compare against."""
import numpy as np
import pytest

import f16_minmax_ref as ref

UNSUPPORTED = 2   # FTAR_ERR_UNSUPPORTED


def test_enum_tables_and_sizes():
    import ftar
    assert ftar.DTYPE["f16"] == 10 and ftar.OP["max"] == 2 and ftar.OP["min"] == 3
    assert ftar.dtype_size("f16") == 2
    assert ftar._dt("torch.float16") == 10
    assert {n: ftar.DTYPE[n] for n in ref.ID} == ref.ID
    for name in ("MPI_MAX", "MPI_MIN"):     # the MPI names stay the reference's list
        assert name not in ftar.OP


@pytest.mark.parametrize("dt,op", [("bool", "max"), ("bool", "min"), ("f16", "band"), ("f32", "band"),
                                   ("bf16", "band")])
def test_unsupported_pairs_are_refused_before_any_device_work(dt, op):
    """Fake pointers: the refusal must come before anything touches HIP."""
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048], 4096, 10, dt, op)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048, 4096, 8192], 16384, 10, dt, op, shape=[2, 2])
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("dt,op", [(11, 0), (11, 2), (-1, 0), (6, 4), (10, 4), (6, -1)])
def test_out_of_range_dtype_and_op_are_refused(dt, op):
    import ftar
    with pytest.raises(ftar.FtarError):
        ftar.reduce([1024, 2048], 4096, 10, dt, op)
    assert ftar.dtype_size(11) == 0


def test_f16_conversion_hook_lives_in_the_bench_library_only():
    import ftar
    assert hasattr(ftar.bench_lib(), "ftar_debug_f16_cvt_check")
    assert not hasattr(ftar.lib(), "ftar_debug_f16_cvt_check")


@pytest.mark.parametrize("P", [2, 4, 8])
def test_one_round_ring_plan_rounds_every_hop(P):
    """The one-round ring folds P copies with one reduce; fp16 (like bf16) reproduces the staged ring only
    if that reduce rounds after every add: the plan's item must say so, and the staged ring and the trees
    must not (their items are one rounding each)."""
    import ftar
    n = 50_001
    for r in range(P):
        items = [it for st in ftar.plan_json("1", P, r, n)["stages"] for it in st["reduces"]]
        assert len(items) == 1 and items[0]["round_each"] == 1 and len(items[0]["srcs"]) == P
        staged = [it for st in ftar.plan_json("1", P, r, n, allgather="stages", reduce_scatter="stages")["stages"]
                  for it in st["reduces"]]
        assert staged and all(len(it["srcs"]) == 2 for it in staged)
    if P >= 4:
        tree = [it for st in ftar.plan_json(f"2,{P // 2}", P, 0, n)["stages"] for it in st["reduces"]]
        assert tree and all(it["round_each"] == 0 for it in tree)


# ---- the helper's own checks ----------------------------------------------------------------------------
def test_float_keys_order_hand_written_cases():
    """f16 bit patterns in ascending order of value, -0 below +0, subnormals in place."""
    asc = [0xFC00, 0xFBFF, 0xBC00, 0x8400, 0x83FF, 0x8001, 0x8000, 0x0000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF,
           0x7C00]
    keys = ref.float_keys("f16", np.array(asc, np.uint16)).astype(np.int64)
    assert np.all(np.diff(keys) > 0)
    assert np.array_equal(ref.keys_to_bits("f16", ref.float_keys("f16", np.array(asc, np.uint16))), np.array(asc, np.uint16))
    for dt in ref.FLOATS:   # the round trip on every pattern class of every format
        x = np.concatenate(ref.sources(dt, 3, 4099))
        assert np.array_equal(ref.keys_to_bits(dt, ref.float_keys(dt, x)), x)


def test_minmax_hand_written_cases():
    f16 = lambda *v: np.array(v, np.uint16)   # noqa: E731
    # lanes: (-0, +0), (+0, -0), (1 ulp, 2 ulp), (-1 ulp, -2 ulp), (-inf, 1), (NaN, +inf), (65504, +inf)
    a = f16(0x8000, 0x0000, 0x0001, 0x8001, 0xFC00, 0x7E01, 0x7BFF)
    b = f16(0x0000, 0x8000, 0x0002, 0x8002, 0x3C00, 0x7C00, 0x7C00)
    mx, mn = ref.minmax("f16", "max", [a, b]), ref.minmax("f16", "min", [a, b])
    assert mx[:5].tolist() == [0x0000, 0x0000, 0x0002, 0x8001, 0x3C00] and mx[6] == 0x7C00
    assert mn[:5].tolist() == [0x8000, 0x8000, 0x0001, 0x8002, 0xFC00] and mn[6] == 0x7BFF
    assert ref.nan_mask("f16", mx)[5] and ref.nan_mask("f16", mn)[5] and not ref.nan_mask("f16", mx)[:5].any()
    # integers compare by signedness: 0x80 is the largest u8 and the smallest i8
    u, i = np.array([0x80, 0x7F], np.uint8), np.array([0x7F, 0x01], np.uint8)
    assert ref.minmax("u8", "max", [u, i]).tolist() == [0x80, 0x7F]
    assert ref.minmax("i8", "max", [u.view(np.int8), i.view(np.int8)]).view(np.uint8).tolist() == [0x7F, 0x7F]
    assert ref.minmax("i8", "min", [u.view(np.int8), i.view(np.int8)]).view(np.uint8).tolist() == [0x80, 0x01]


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_float_minmax_agrees_with_numpy_where_numpy_is_defined(dt):
    """Away from NaN and signed zeros numpy's own maximum is the same function: a cross-check of the keys
    against real float compares (bf16 through its fp32 widening)."""
    ins = ref.sources(dt, 5, 4099)
    u = ref.storage(dt)
    as_float = {"f16": lambda x: x.view(np.float16), "f32": lambda x: x.view(np.float32),
                "f64": lambda x: x.view(np.float64),
                "bf16": lambda x: (x.astype(np.uint32) << np.uint32(16)).view(np.float32)}[dt]
    vals = [as_float(x) for x in ins]
    for op, f in (("max", np.maximum), ("min", np.minimum)):
        want = f.reduce(vals)
        got = as_float(ref.minmax(dt, op, ins).astype(u))
        ok = ~np.isnan(want) & (want != 0)
        assert ok.mean() > 0.9 and np.array_equal(got[ok], want[ok])


@pytest.mark.parametrize("dt", ref.MINMAX_DTYPES)
@pytest.mark.parametrize("k", [2, 17])
def test_sources_carry_the_planted_specials_and_few_nans(dt, k):
    n = 100_003
    ins = ref.sources(dt, k, n)
    assert len(ins) == k and all(x.size == n and x.dtype == ref.storage(dt) for x in ins)
    if dt in ref.INTS:
        info = np.iinfo(ref.INTS[dt])
        assert (ins[0] == info.max).any() and (ins[k - 1] == info.min).any()
        return
    u, bits, emask, elow = ref.FLOATS[dt]
    sign = 1 << (bits - 1)
    per_source = [float(ref.nan_mask(dt, x).mean()) for x in ins]
    assert per_source[0] > 0 and max(per_source[1:]) == 0           # NaNs only where planted
    assert (ins[k - 1] == emask).any() and (ins[k // 2] == (sign | emask)).any()
    assert ins[0][11] == sign and ins[1][11] == 0 and ins[0][12] == 0 and ins[1][12] == sign
    assert ins[k - 1][13] == 1 and ins[0][17] == 1 and ins[1][18] == (sign | 2)
    for op in ("max", "min"):
        out = ref.minmax(dt, op, ins)
        share = float(ref.nan_mask(dt, out).mean())
        assert 0 < share < 0.02 and ref.same_bits(dt, out, out)
    assert ref.minmax(dt, "max", ins)[11] == 0 and ref.minmax(dt, "min", ins)[12] == sign   # -0 < +0
    assert ref.minmax(dt, "max", ins)[17] == k and ref.minmax(dt, "min", ins)[18] == (sign | k)


def test_nan_share_cap_trips_on_raw_patterns():
    """What the cap is for: raw 16-bit patterns at k = 16 are ~40 % NaN lanes."""
    rng = np.random.default_rng(0)
    raw = [rng.integers(0, 1 << 16, size=20_000, dtype=np.uint16) for _ in range(16)]
    out = ref.minmax("f16", "max", raw)
    assert float(ref.nan_mask("f16", out).mean()) > 0.3
    with pytest.raises(AssertionError, match="NaN lanes"):
        ref.same_bits("f16", out, out)


def test_same_bits_sees_a_single_wrong_lane_and_ignores_nan_payloads():
    ins, want = ref.f16_fold_case(3, 4099)
    assert ref.same_bits("f16", want, want) and ref.first_diff("f16", want, want) is None
    nan = np.flatnonzero(ref.nan_mask("f16", want))
    got = want.copy()
    got[nan[0]] = 0xFE00                       # another NaN: the same
    assert ref.same_bits("f16", got, want)
    got[nan[0]] = 0x7C00                       # inf where a NaN belongs
    assert not ref.same_bits("f16", got, want) and ref.first_diff("f16", got, want)[0] == nan[0]
    got = want.copy()
    got[7] ^= 1
    assert not ref.same_bits("f16", got, want) and ref.first_diff("f16", got, want)[0] == 7


def test_f16_sum_expectations_round_as_specified():
    """The planted fp16 SUM lanes: ties to even, overflow to inf; NaN share of every schedule under the cap;
    schedules differ from each other (else the per-schedule tests would pin nothing)."""
    ins, flat = ref.f16_fold_case(8, 50_001)
    assert flat[19] == 0x6800 and flat[20] == 0x6802 and flat[21] == 0x7C00
    assert flat[11] == 0x0000 and flat[12] == 0x0000                 # -0 + +0 = +0 under RNE
    assert flat[17] == 36 and flat[18] == (0x8000 | 36)              # subnormals add exactly: 1 + ... + 8
    ring, tree, nested = ref.f16_ring(ins), ref.f16_tree(ins, [2, 4]), ref.f16_nested(ins, [2, 4])
    for out in (flat, ring, tree, nested):
        assert float(ref.nan_mask("f16", out).mean()) < 0.02 and ref.same_bits("f16", out, out)
    assert not ref.same_bits("f16", ring, flat) and not ref.same_bits("f16", tree, ring)
    for a in (ring, tree, nested):
        assert a[19] == 0x6800 and a[21] == 0x7C00
    ins4, want = ref.exact_sum_case("f16", 5, 1001)
    assert ref.same_bits("f16", ref.f16_fold(ins4), want) and ref.same_bits("f16", ref.f16_ring(ins4), want)
