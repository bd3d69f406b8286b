"""FTAR_AVG and ftar_reduce_scaled at the API surface, without a GPU: the enum, what is refused before any
device work, where the plans put their root folds (the one place AVG scales), a numpy model of the engine that
scales there and nowhere else, and the self-checks of the CPU expectation (tests/avg_ref.py) that the GPU tests
in tests/test_gpu_avg.py compare against."""
import collections
import random

import numpy as np
import pytest

import avg_ref
import f16_minmax_ref as ref
import golden_cases as gc

INVALID_ARG, UNSUPPORTED = 1, 2


def test_avg_is_op_4_without_an_mpi_alias():
    import ftar
    assert ftar.OP["avg"] == 4
    assert not [name for name in ftar.OP if name.startswith("MPI_") and ftar.OP[name] == 4]


@pytest.mark.parametrize("dt", ["i32", "bool", "u8", "i64"])
def test_scaled_reduce_refuses_other_dtypes_before_any_device_work(dt):
    """Fake pointers: the refusal must come before anything touches HIP."""
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048], 4096, 10, dt, scale=0.5)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048, 4096, 8192], 16384, 10, dt, scale=0.25, shape=[2, 2])
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("scale", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_scaled_reduce_refuses_a_non_finite_scale(dt, scale):
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048], 4096, 10, dt, scale=scale)
    assert e.value.status == INVALID_ARG


@pytest.mark.parametrize("shape", [[2, 3], [2, 2, 2], [2, 0, 2], [2, 2, 2, 2, 2]])
def test_scaled_reduce_refuses_a_shape_that_is_not_k(shape):
    """More than one level: the product must be k (one level or none is the flat fold, as ftar_reduce_nested)."""
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048, 4096, 8192], 16384, 10, "f32", scale=0.25, shape=shape)
    assert e.value.status == INVALID_ARG


def test_scale_goes_with_sum_only():
    import ftar
    with pytest.raises(ValueError):
        ftar.reduce([1024, 2048], 4096, 10, "f32", "max", scale=0.5)


# ---- where the plans put the root ---------------------------------------------------------------------------
def _topologies():
    seen, out = set(), []
    for c in gc.allreduce_cases(max_n=70000):
        key = (c["P"], c["topo"], c["lonely"], c["n"])
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out


def _random_topologies(seed=4, count=60):
    """random_cases.random_topology draws the reference can run (oracle_lib refuses the others)."""
    import oracle_lib
    import random_cases
    rng, out = random.Random(seed), []
    while len(out) < count:
        P = rng.randint(2, 12)
        topo, lonely = random_cases.random_topology(rng, P)
        n = rng.choice([1, P - 1, P, P + 1, rng.randint(2, 200), rng.randint(200, 3000)])
        try:
            oracle_lib.allreduce([np.zeros(n, np.float32) for _ in range(P)], topo, lonely, 6, 0)
        except RuntimeError:
            continue
        out.append((P, topo, lonely, n))
    return out


def _plans(P, topo, lonely, n, form):
    import ftar
    t = ftar.topo(topo, lonely)
    return [ftar.plan_json(t, P, r, n, allgather=form, reduce_scatter=form) for r in range(P)]


def _blocks(P, n):
    split = -(-n // P)
    return {b: (b * split, min(n, (b + 1) * split) - b * split) for b in range(P) if b * split < n}


def check_roots(P, topo, lonely, n, form):
    plans = _plans(P, topo, lonely, n, form)
    ring = 1 in [int(w) for w in topo.split(",")]
    blocks = _blocks(P, n)
    roots = collections.defaultdict(list)   # (off, len) -> [rank]
    for r, p in enumerate(plans):
        for st in p["stages"]:
            for it in st["reduces"]:
                assert it["root"] in (0, 1)
                if it["root"]:
                    roots[(it["off"], it["len"])].append(r)
    what = (P, topo, lonely, n, form)
    assert sorted(roots) == sorted(blocks.values()), what      # exactly the non-empty blocks' ranges
    for b, rng_ in blocks.items():
        owner = (b - 1) % P if ring else b
        assert roots[rng_] == [owner], (what, b)               # one root item, on the owning rank
        off, ln = rng_
        seen_root = False
        for st in plans[owner]["stages"]:                       # and nothing on that rank writes the range later
            for it in st["reduces"]:
                overlaps = it["off"] < off + ln and off < it["off"] + it["len"]
                assert not (seen_root and overlaps), (what, b)
                seen_root = seen_root or (it["root"] and (it["off"], it["len"]) == rng_)
        assert seen_root
    return plans


def simulate_avg(plans, inputs):
    """This file's copy of test_plan.simulate (numpy model of the engine, stage-synchronous, in place) for f32
    inputs whose every partial sum is exact: a fold is the plain sum of its sources, whatever its shape, and
    root items, only they, multiply by fl(1 / P)."""
    P = len(plans)
    r = np.float32(1) / np.float32(P)
    dst = [x.copy() for x in inputs]
    scratch = [np.zeros(max(1, 2 * p["scratch_half"]), np.float32) for p in plans]
    bufs = [{"src": dst[q], "dst": dst[q], "scratch": scratch[q]} for q in range(P)]
    nst = len(plans[0]["stages"])
    assert all(len(p["stages"]) == nst for p in plans)
    for s in range(nst):
        wire = collections.defaultdict(collections.deque)
        for q in range(P):
            for peer, buf, off, ln in plans[q]["stages"][s]["sends"]:
                wire[(q, peer)].append(bufs[q][buf][off:off + ln].copy())
        for q in range(P):
            for peer, buf, off, ln in plans[q]["stages"][s]["recvs"]:
                msg = wire[(peer, q)].popleft()
                assert msg.size == ln
                bufs[q][buf][off:off + ln] = msg
        assert all(not w for w in wire.values()), "unmatched send"
        for q in range(P):
            for it in plans[q]["stages"][s]["reduces"]:
                off, ln = it["off"], it["len"]
                acc = bufs[q][it["srcs"][0][0]][it["srcs"][0][1]:it["srcs"][0][1] + ln].copy()
                for b, o in it["srcs"][1:]:
                    acc = acc + bufs[q][b][o:o + ln]
                bufs[q]["dst"][off:off + ln] = acc * r if it["root"] else acc
    return dst


def check_model_mean(plans, P, n, seed):
    """Small integers times P: every partial sum is exact, so every rank must end with fl(P S * fl(1 / P)), S the
    integer sum, bit for bit, whatever the association -- the exact mean S itself wherever that product rounds
    back to S (every lane at P = 2, 3, 4, 5, 6, 8, ...; at P = 7, 13 and 14, which the golden topologies include,
    fl(1 / P) is far enough from 1 / P that some lanes land one ulp off S, e.g. -98 * fl(1 / 7) = -14.000001).
    A flag on an inner item gives (a r + b), a missing one leaves the sum."""
    rng = np.random.default_rng([seed, P, n])
    small = rng.integers(-8, 9, size=(P, n))
    ins = [(small[q] * P).astype(np.float32) for q in range(P)]
    mean = small.sum(axis=0).astype(np.float32)
    want = (mean * np.float32(P)) * (np.float32(1) / np.float32(P))
    if P in (2, 3, 4, 5, 6, 8, 9, 10, 12, 16):
        assert want.tobytes() == mean.tobytes()
    outs = simulate_avg(plans, ins)
    for q in range(P):
        assert outs[q].tobytes() == want.tobytes(), (q, np.flatnonzero(outs[q] != want)[:4])


@pytest.mark.parametrize("form", ["stages", "direct"])
@pytest.mark.parametrize("P,topo,lonely,n", _topologies(), ids=lambda v: str(v))
def test_plan_roots_golden_topologies(P, topo, lonely, n, form):
    plans = check_roots(P, topo, lonely, n, form)
    check_model_mean(plans, P, n, 1)


def test_plan_roots_random_topologies():
    lonely_seen = 0
    for P, topo, lonely, n in _random_topologies():
        lonely_seen += lonely > 0
        for form in ("stages", "direct"):
            plans = check_roots(P, topo, lonely, n, form)
            check_model_mean(plans, P, n, 2)
    assert lonely_seen >= 5


def test_root_flag_is_independent_of_everything_but_the_plan():
    """P = 1 has no stages; the collective all-gather keeps the reduce-scatter's roots."""
    import ftar
    assert ftar.plan_json("1", 1, 0, 100)["stages"] == []
    for r in range(4):
        a = ftar.plan_json("2,2", 4, r, 4000, allgather="collective")
        b = ftar.plan_json("2,2", 4, r, 4000)
        assert a["allgather"] == "collective"
        assert [it["root"] for st in a["stages"] for it in st["reduces"]] == \
               [it["root"] for st in b["stages"] for it in st["reduces"]] == [1]


# ---- the expectation itself --------------------------------------------------------------------------------
def _one(dt, *vals):
    return [np.array([v], ref.storage(dt)) for v in vals]


def test_expectation_fp16_mean_is_finite_where_the_sum_is_inf():
    ins = _one("f16", 0x7BFF, 0x7BFF)                           # 65504 + 65504
    assert avg_ref.sum_fold("f16", ins)[0] == 0x7C00            # the sum: +inf
    assert avg_ref.root_fold("f16", ins, avg_ref.recip("f16", 2))[0] == 0x7BFF
    assert avg_ref.ring("f16", [np.repeat(x, 2) for x in ins]).tolist() == [0x7BFF, 0x7BFF]


def test_expectation_rounds_ties_to_even_after_scaling():
    r = avg_ref.recip("f16", 2)
    assert avg_ref.root_fold("f16", _one("f16", 0x6C00, 0x4000), r)[0] == 0x6800   # (4096 + 2) / 2 = 2049 -> 2048
    assert avg_ref.root_fold("f16", _one("f16", 0x6C01, 0x4000), r)[0] == 0x6802   # (4100 + 2) / 2 = 2051 -> 2052
    rb = avg_ref.recip("bf16", 2)
    assert avg_ref.root_fold("bf16", _one("bf16", 0x4400, 0x4000), rb)[0] == 0x4380    # (512 + 2) / 2 = 257 -> 256
    assert avg_ref.root_fold("bf16", _one("bf16", 0x4401, 0x4000), rb)[0] == 0x4382    # (516 + 2) / 2 = 259 -> 260


def test_expectation_keeps_a_subnormal_f32_product():
    r = avg_ref.recip("f32", 2)
    assert avg_ref.root_fold("f32", _one("f32", 0x00800003, 0), r)[0] == 0x00400002    # tie -> even, subnormal
    assert avg_ref.root_fold("f32", _one("f32", 0x00800002, 0), r)[0] == 0x00400001    # exact, subnormal
    assert avg_ref.root_fold("f32", _one("f32", 0x80000003, 0x80000000), r)[0] == 0x80000002   # -3 ulp / 2: tie
    r64 = avg_ref.recip("f64", 2)
    assert avg_ref.root_fold("f64", _one("f64", 0x0010000000000002, 0), r64)[0] == 0x0008000000000001


def test_expectation_is_not_vacuous():
    """At P = 3 the multiply by fl(1 / 3) must differ from a division by 3 in at least 1 % of f32 lanes, and the
    fp16 root (scaled, then rounded once) from the round-twice result in at least 1 % of lanes: else the GPU
    tests could not tell these apart."""
    import torch
    n, P = 100_003, 3
    ins = ref.sources("f32", P, n)
    want = avg_ref.root_fold("f32", ins, avg_ref.recip("f32", P))
    acc = avg_ref._acc("f32", ins)
    div = avg_ref._bits("f32", acc / 3.0)
    ok = ~ref.nan_mask("f32", want)
    share = float((div[ok] != want[ok]).mean())
    print(f"f32 P=3 multiply vs divide: {share:.1%} of lanes differ")
    assert share >= 0.01
    ins = ref.sources("f16", P, n)
    want = avg_ref.root_fold("f16", ins, avg_ref.recip("f16", P))
    acc = avg_ref._acc("f16", ins)
    twice = avg_ref._bits("f16", (acc.to(torch.float16).float() * avg_ref.recip("f16", P)).to(torch.float16))
    ok = ~ref.nan_mask("f16", want)
    share = float((twice[ok] != want[ok]).mean())
    print(f"f16 P=3 round once vs twice: {share:.1%} of lanes differ")
    assert share >= 0.01


@pytest.mark.parametrize("k", [2, 3, 8, 16])
@pytest.mark.parametrize("dt", avg_ref.FLOAT_DTYPES)
def test_expectation_nan_share_stays_under_the_cap(dt, k):
    ins, want = avg_ref.reduce_case(dt, k, 4099, 0.125)
    assert ref.same_bits(dt, want, want)        # asserts the cap
    assert float(ref.nan_mask(dt, want).mean()) < ref.NAN_SHARE_CAP


def test_exact_case_is_its_own_mean():
    for dt in ("f16", "bf16", "f32"):
        for P in (5, 8):
            ins, want = avg_ref.exact_case(dt, P, 4099)
            assert ref.same_bits(dt, avg_ref.root_fold(dt, ins, avg_ref.recip(dt, P)), want)
