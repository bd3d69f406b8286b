"""Write footprint and tile-edge sizes of every fold and copy kernel (csrc/reduce_impl.h).

Every launch writes into a guarded arena (tests/kernel_edges.py): the payload must equal the pinned reference bit
for bit, every byte of the arena outside [dst, dst + n) must still hold its position-dependent filler, and every
source that is not the destination must be unchanged.  The counts sit on the edges of the launched kernel's own
geometry (head + nvec x VE + tail around one wave tile, one workgroup tile and three of them), which is read from
the kernel's name, so a retune of the (U, W) tables moves the edges and these tests follow.  Inputs are finite and
free of NaN; expectations come from the references the suite pins elsewhere (the oracle, avg_ref, f16_minmax_ref,
f8_ref for the two fp8 formats) and the hop folds written out in torch, computed once per case over the longest
length.  (tests/test_gpu_f8_edges.py holds six more fp8 cases; tests/test_gpu_amax_edges.py runs the footprint
cases of this file under the amax finish.)"""
import numpy as np
import pytest

import kernel_edges as ke
from test_gpu_avg import FAMILIES

pytestmark = pytest.mark.gpu

THIRD = float(np.float32(1) / np.float32(3))
QUARTER = 0.25
ELEMENTWISE = ("reduce_elem_kernel", "reduce_tree_elem_kernel")


# ---- launchers: (source pointers, destination pointer, count) -> one call ---------------------------------
def api(dt, op="sum", shape=None, scale=None):
    """Through the public entry points (ftar_reduce, ftar_reduce_nested, ftar_reduce_scaled)."""
    def launch(srcs, dst, n):
        import ftar
        ftar.reduce(srcs, dst, n, dt, op, shape=list(shape) if shape else None, scale=scale)
    return launch


def ex(dt, op="sum", **kw):
    """Through ftar_debug_reduce_ex: what only the engine passes (round_each, lds = false)."""
    def launch(srcs, dst, n):
        ke.reduce_ex(srcs, dst, n, dt, op, **kw)
    return launch


def probe(launch, dt, k, shifts=None):
    """The id of the kernel `launch` takes for co-aligned pointers (but for `shifts`) and a count with vectors."""
    import ftar
    import torch
    esz = ke.esize(dt)
    rows = torch.zeros((k + 1, 66 * 16 + 32), dtype=torch.uint8, device="cuda")
    shifts = shifts or [0] * k
    launch([rows[j].data_ptr() + shifts[j] * esz for j in range(k)], rows[k].data_ptr(), 65 * (16 // esz))
    torch.cuda.synchronize()
    return ftar.last_kernel()


def fold_for(dt, op, k, length, shape=None, scale=None, hop=False, shifts=None, stair=None):
    """stair: boundaries of kernel_edges.staircase inputs (SUM; finite at any k) in place of the ordinary ones."""
    if stair is not None:
        return ke.Fold(*ke.staircase(dt, k, stair, length, scale=scale, shape=shape, hop=hop), shifts=shifts)
    ins = ke.sources(dt, op, k, length)
    return ke.Fold(ins, ke.expected(dt, op, ins, shape=shape, scale=scale, hop=hop), shifts=shifts)


def run_counts(launch, fold, edges, alias=None):
    """Every count of `edges` at the offset that gives its head; returns the kernel ids of the counts with
    vectors."""
    import ftar
    ids = set()
    for e in edges:
        off = ke.head_offset(fold.ve, e.head)
        srcs, dst = fold.pointers(off, alias)
        launch(srcs, dst, e.n)
        bad = fold.verify(off, e.n, alias)
        assert bad is None, (e, alias, ftar.last_kernel(), bad)
        if e.nvec >= 1:
            ids.add(ftar.last_kernel())
    return ids


def edges_of(symbol, ve):
    g = ke.geometry(symbol)
    edges = ke.edge_counts(ve, g.wg_tile)
    if g.family in ELEMENTWISE:     # its tile is 256 elements, not vectors: those exact multiples too
        edges += [e for e in ke.edge_counts(1, g.wg_tile) if e not in edges]
    return g, edges


def run_edges(launch, dt, op, k, shape=None, scale=None, hop=False, shifts=None, check_id=None, stair=False):
    """The whole of one case: probe the kernel, take its edges, build inputs and expectation once, run.  stair:
    staircase inputs that step up where each count ends."""
    symbol = probe(launch, dt, k, shifts)
    if check_id:
        check_id(symbol)
    ve = 16 // ke.esize(dt)
    g, edges = edges_of(symbol, ve)
    ends = [ke.head_offset(ve, e.head) + e.n for e in edges] if stair else None
    fold = fold_for(dt, op, k, max(e.n for e in edges) + ve, shape, scale, hop, shifts, stair=ends)
    ids = run_counts(launch, fold, edges)
    assert ids == {symbol}, "one kernel for every count with vectors"
    return g


# ---- footprint at the edges, every family in both finishes ------------------------------------------------
def _named(want_id, scaled):
    def check(symbol):
        w = want_id
        if scaled:
            w = (tuple(x.replace("_kernel<", "_scaled_kernel<") for x in w) if isinstance(w, tuple)
                 else w.replace("_kernel<", "_scaled_kernel<"))
        if isinstance(w, str):
            assert symbol == w
        else:
            assert symbol.startswith(w[0]) and all(x in symbol for x in w[1:]), (symbol, w)
    return check


def _family_cases():
    out = {}
    for name, (call, want_id) in FAMILIES.items():          # reached as tests/test_gpu_avg.py reaches them
        out[name] = dict(dt=call["dt"], k=call["k"], shape=call.get("shape"), shifts=call.get("offsets"),
                         via="api", want_id=want_id)
    for dt, fmt in (("bf16", "Bf16Fmt<"), ("f16", "HalfFmt>")):
        for k in (3, 8):    # the hop folds: plain rounds after every add, scaled before (H16SumHopPreT)
            out[f"hop_{dt}_k{k}"] = dict(dt=dt, k=k, via="ex", kw=dict(round_each=True), hop=True,
                                         want_id=(f"reduce_lds_kernel<H16SumHop", f"T<{fmt}", f", {k}, "))
    for dt, fmt in (("f8e4m3", "T<F8Fmt<false>"), ("f8e5m2", "T<F8Fmt<true>")):
        for k in (3, 8):    # fp8's: F8SumHopT, and F8SumHopPreT under a scaled finish (at 0.25)
            out[f"hop_{dt}_k{k}"] = dict(dt=dt, k=k, via="ex", kw=dict(round_each=True), hop=True, scale=QUARTER,
                                         want_id=("reduce_lds_kernel<F8SumHop", fmt, f", {k}, "))
    for dt, tr in (("f32", "F32Sum"), ("bf16", "H16SumT<Bf16Fmt<")):
        out[f"vec_ab_{dt}_k3"] = dict(dt=dt, k=3, via="ex", kw=dict(lds=False),     # the peer forms' ":vec" A/B
                                      want_id=(f"reduce_vec_kernel<{tr}", ", 0, 2, true, true, 512>"))
    out["tree_reg_f32_2x2"] = dict(dt="f32", k=4, shape=(2, 2), via="ex", kw=dict(lds=False),
                                   want_id=("reduce_tree_kernel<F32Sum, 4, 2, ", "StaticShape<2, 2>"))
    out["tree_reg_f32_2x3"] = dict(dt="f32", k=6, shape=(2, 3), via="ex", kw=dict(lds=False),
                                   want_id=("reduce_tree_kernel<F32Sum, 6, 2, ", "RuntimeShape"))
    return out


FAMILY_CASES = _family_cases()


def _launcher(c, scale):
    if c["via"] == "api":
        return api(c["dt"], shape=c.get("shape"), scale=scale)
    return ex(c["dt"], shape=c.get("shape"), scale=scale, **c["kw"])


@pytest.mark.parametrize("finish", ["plain", "scaled"])
@pytest.mark.parametrize("family", sorted(FAMILY_CASES))
def test_footprint_at_the_edges_of_every_family(family, finish):
    c = FAMILY_CASES[family]
    scale = c.get("scale", THIRD) if finish == "scaled" else None
    want_id = c["want_id"]
    if c.get("hop") and scale is not None:      # under a scaled finish the hop fold is the Pre trait
        want_id = (want_id[0] + "Pre",) + want_id[1:]
    run_edges(_launcher(c, scale), c["dt"], "sum", c["k"], shape=c.get("shape"), scale=scale, hop=c.get("hop", False),
              shifts=c.get("shifts"), check_id=_named(want_id, scale is not None))


# ---- every LDS shape of the table --------------------------------------------------------------------------
WIDTHS = ["u8", "bf16", "f32", "f64"]                       # one SUM trait per element width
ALL_K = list(range(1, 18)) + [33, 64]
OTHER_TRAITS = ([(dt, "sum") for dt in ("i16", "i32", "i64", "bool", "f16")] + [("u8", "band"), ("i64", "band")] +
                [(dt, op) for dt in ("i8", "u16", "f32", "f64", "bf16", "f16") + ke.F8 for op in ("max", "min")])
F8_K = list(range(2, 18))                                   # what f8_ref.finite_sources covers: the LDS kernels up
#                                                             to 8, the runtime-k register kernel above
F8_STAIR_K = [33, 64]                                       # on staircase inputs, finite at any k
SUM_CASES = [(dt, k) for dt in WIDTHS for k in ALL_K] + [(dt, k) for dt in ke.F8 for k in F8_K + F8_STAIR_K]


@pytest.mark.parametrize("dt,k", SUM_CASES, ids=[f"{d}-{k}" for d, k in SUM_CASES])
def test_sum_at_the_edges_of_every_k(dt, k):
    run_edges(api(dt), dt, "sum", k, stair=dt in ke.F8 and k in F8_STAIR_K)


@pytest.mark.parametrize("k", [2, 8, 9, 16, 17])
@pytest.mark.parametrize("dt,op", OTHER_TRAITS, ids=[f"{d}-{o}" for d, o in OTHER_TRAITS])
def test_every_other_trait_at_the_edges(dt, op, k):
    run_edges(api(dt, op), dt, op, k)


@pytest.mark.parametrize("dt", WIDTHS)
def test_the_parsed_lds_shapes_differ_across_k(dt):
    """A guard against a parser that returns a constant: the (U, W) table has several shapes per element width."""
    shapes = set()
    for k in range(2, 17):
        g = ke.geometry(probe(api(dt), dt, k))
        if g.lds_shape:
            assert g.family == "reduce_lds_kernel" and g.wg_tile == g.lds_shape[0] * g.lds_shape[1] * 64
            shapes.add(g.lds_shape)
    assert len(shapes) > 1, shapes


# ---- dense small sweep (independent of the name parser) ---------------------------------------------------
DENSE = [(dt, k) for dt in WIDTHS for k in (2, 8)] + [("f8e4m3", 2), ("f8e5m2", 8)]


@pytest.mark.parametrize("dt,k", DENSE, ids=[f"{d}-{k}" for d, k in DENSE])
def test_dense_small_counts(dt, k):
    """Every count from 0 to two wave tiles and two vectors, at heads 0 and 1."""
    ve = 16 // ke.esize(dt)
    top = 2 * 64 * ve + 2 * ve
    fold = fold_for(dt, "sum", k, top + ve)
    launch = api(dt)
    for head in (0, 1):
        if head >= ve:
            continue
        off = ke.head_offset(ve, head)
        for n in range(top + 1):
            srcs, dst = fold.pointers(off)
            launch(srcs, dst, n)
            bad = fold.verify(off, n)
            assert bad is None, (n, head, bad)


# ---- dst == srcs[j] at every position ---------------------------------------------------------------------
ALIAS = {
    "lds_k2": dict(dt="f32", k=2),
    "lds_k8": dict(dt="bf16", k=8),
    "vec_k17": dict(dt="f32", k=17),
    "elem": dict(dt="f32", k=3, shifts=[0, 1, 0]),
    "tree_lds_2x4": dict(dt="f32", k=8, shape=(2, 4)),
    "tree_reg_f64_2x2": dict(dt="f64", k=4, shape=(2, 2)),
    "f8_lds_k8": dict(dt="f8e4m3", k=8),
    "f8_tree_lds_2x2": dict(dt="f8e5m2", k=4, shape=(2, 2)),
}
ALIAS_FAMILY = {"lds_k2": "reduce_lds_kernel", "lds_k8": "reduce_lds_kernel", "vec_k17": "reduce_vec_kernel",
                "elem": "reduce_elem_kernel", "tree_lds_2x4": "reduce_tree_lds_kernel",
                "tree_reg_f64_2x2": "reduce_tree_kernel", "f8_lds_k8": "reduce_lds_kernel",
                "f8_tree_lds_2x2": "reduce_tree_lds_kernel"}


@pytest.mark.parametrize("finish", ["plain", "scaled"])
@pytest.mark.parametrize("family", sorted(ALIAS))
def test_dst_may_be_any_one_source(family, finish):
    """dst == srcs[j] for the first, a middle and the last j (the one-round forms hand the fold its sources in
    leaf order, so in place the destination is whichever source the rank's position gives): counts with a head, a
    partial tile and a tail; the other sources stay as they were."""
    c = ALIAS[family]
    dt, k, shape, shifts = c["dt"], c["k"], c.get("shape"), c.get("shifts")
    scale = THIRD if finish == "scaled" else None
    launch = api(dt, shape=shape, scale=scale)
    symbol = probe(launch, dt, k, shifts)
    g = ke.geometry(symbol)
    assert g.family == ALIAS_FAMILY[family], symbol
    ve = 16 // ke.esize(dt)
    edges = [e for e in ke.edge_counts(ve, g.wg_tile)
             if (e.head, e.tail) == (ve - 1, ve - 1) and e.nvec in (g.wg_tile + 1, 3 * g.wg_tile - 1)]
    assert len(edges) == 2
    fold = fold_for(dt, "sum", k, max(e.n for e in edges) + ve, shape, scale, shifts=shifts)
    for j in sorted({0, k // 2, k - 1}):
        ids = run_counts(launch, fold, edges, alias=j)
        assert ids == {symbol}


# ---- the element-wise kernels' grid-stride loops ----------------------------------------------------------
STRIDE_N = 8192 * 256 + 256 + 3        # past the 8192-workgroup grid: a whole second pass, then a partial one


@pytest.mark.parametrize("dt,k,shape,scale", [("u8", 2, None, None), ("f32", 3, None, None), ("bf16", 2, None, THIRD),
                                              ("f32", 4, (2, 2), None), ("f8e4m3", 2, None, None)],
                         ids=["u8_k2", "f32_k3", "bf16_k2_scaled", "tree_elem_f32_2x2", "f8e4m3_k2"])
def test_elementwise_grid_stride(dt, k, shape, scale):
    import ftar
    shifts = [0] * (k - 1) + [1]       # the last source misaligned against dst
    ve = 16 // ke.esize(dt)
    fold = fold_for(dt, "sum", k, STRIDE_N + ve, shape, scale, shifts=shifts)
    launch = api(dt, shape=shape, scale=scale)
    for off in (0, 1):
        srcs, dst = fold.pointers(off)
        launch(srcs, dst, STRIDE_N)
        bad = fold.verify(off, STRIDE_N)
        assert bad is None, (off, ftar.last_kernel(), bad)
        assert ke.geometry(ftar.last_kernel()).family == ("reduce_tree_elem_kernel" if shape else "reduce_elem_kernel")


# ---- the multi-segment copy -------------------------------------------------------------------------------
SEG_SIZES = [0, 1, 3, 15, 16, 17, 8191, 8192, 8193, 3 * 8192 + 4096 + 5]
ALIGN = [(0, 0), (5, 5), (15, 15), (3, 8), (0, 1)]             # (src mod 16, dst mod 16)
GAP = 64


def place(sizes, mod):
    """Windows of these sizes back to back, each at `mod` from a 16-byte boundary, >= GAP guard bytes between."""
    wins, cur = [], 0
    for b in sizes:
        lo = -(-cur // 16) * 16 + mod
        wins.append((lo, lo + b))
        cur = lo + b + GAP
    return wins, cur


def seg_sizes(nsegs, turn):
    """Unequal sizes with the largest among them and, from three segments on, a zero-byte one in the middle."""
    big = SEG_SIZES[-1]
    if nsegs == 1:
        return [SEG_SIZES[1 + 2 * turn % 9]]
    if nsegs == 2:
        return [SEG_SIZES[1 + (3 * turn) % 8], big]
    sizes = [SEG_SIZES[(i + turn) % len(SEG_SIZES)] for i in range(nsegs)]
    sizes[nsegs // 2] = 0
    sizes[-1] = big
    if nsegs >= len(SEG_SIZES) + 2:
        assert set(sizes) == set(SEG_SIZES)
    return sizes


class CopyArenas:
    def __init__(self, nbytes, seed):
        self.src, self.dst = ke.Arena(nbytes), ke.Arena(nbytes)
        self.src.upload(0, np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8))

    def verify(self, swins, dwins, what):
        import torch
        for i, ((slo, shi), (dlo, dhi)) in enumerate(zip(swins, dwins)):
            got, exp = self.dst.window(dlo, dhi), self.src.window(slo, shi)
            if not torch.equal(got, exp):
                bad = int(torch.nonzero(got != exp)[0])
                raise AssertionError((what, f"segment {i} of {shi - slo} bytes differs from byte {bad}"))
        assert ke.check_untouched(self.dst, windows=dwins) is None, (what, ke.check_untouched(self.dst, windows=dwins))
        assert ke.check_untouched(self.src) is None, (what, ke.check_untouched(self.src))
        for lo, hi in dwins:
            self.dst.restore(lo, hi)


@pytest.mark.parametrize("ms,md", ALIGN)
def test_multi_segment_copy(ms, md):
    """launch_gather through ftar_debug_gather: 1, 2, 3, 8 and FTAR_MAX_K segments of unequal sizes (a zero-byte
    one in the middle, 3 bytes at misalignment 5 or 15: head > n), both cache policies, with and without the
    release fence, and workgroup caps that make the stride loop turn on the largest segment.  Every destination
    segment equals its source; the 64-byte gaps, the guards and the sources are untouched."""
    import ftar
    turn = ALIGN.index((ms, md))
    total = place([max(SEG_SIZES)] * ke.MAX_K, 15)[1]
    arenas = CopyArenas(total, 77 + turn)
    for i, nsegs in enumerate([1, 2, 3, 8, ke.MAX_K]):
        i += turn                                      # every axis value meets every alignment pair
        nt, rel, cap = i % 2, (i // 2) % 2, (0, 1, 3)[i % 3]
        sizes = seg_sizes(nsegs, turn)
        swins, dwins = place(sizes, ms)[0], place(sizes, md)[0]
        what = dict(nsegs=nsegs, sizes=sizes if nsegs <= 8 else "all", nt=nt, release_system=rel, max_wg_per_seg=cap)
        ke.gather([arenas.src.ptr(lo) for lo, _ in swins], [arenas.dst.ptr(lo) for lo, _ in dwins], sizes,
                  nt=nt, max_wg_per_seg=cap, release_system=rel)
        arenas.verify(swins, dwins, what)
        assert ftar.last_kernel() == f"gather_kernel<{'true' if nt else 'false'}, {'true' if rel else 'false'}>", what
    # each cap on the largest size alone and with company, at this alignment
    for cap in (1, 3):
        for sizes in ([SEG_SIZES[-1]], [8193, 0, SEG_SIZES[-1], 3]):
            swins, dwins = place(sizes, ms)[0], place(sizes, md)[0]
            ke.gather([arenas.src.ptr(lo) for lo, _ in swins], [arenas.dst.ptr(lo) for lo, _ in dwins], sizes,
                      max_wg_per_seg=cap)
            arenas.verify(swins, dwins, dict(sizes=sizes, max_wg_per_seg=cap))


def test_multi_segment_copy_axes_meet_every_alignment():
    """The trimmed cross product above, counted: both cache policies, the fence on and off, every cap and every
    size under every alignment pair."""
    for turn in range(len(ALIGN)):
        seen = [(i % 2, (i // 2) % 2, (0, 1, 3)[i % 3]) for i in range(turn, turn + 5)]
        assert {s[0] for s in seen} == {0, 1} and {s[1] for s in seen} == {0, 1}
        assert {s[2] for s in seen} == {0, 1, 3}
        assert set(seg_sizes(ke.MAX_K, turn)) == set(SEG_SIZES)
        for nsegs in (3, 8, ke.MAX_K):
            sizes = seg_sizes(nsegs, turn)
            assert sizes[nsegs // 2] == 0 and max(SEG_SIZES) in sizes and len(set(sizes)) > 1


@pytest.mark.parametrize("ms,md", ALIGN)
def test_single_copy_takes_the_lds_copy_or_the_copy_kernel(ms, md):
    """launch_copy (ftar_reduce with k = 1 on u8): the LDS-staged copy when source and destination share their
    address mod 16, the multi-segment copy kernel otherwise; same sizes, same checks."""
    import ftar
    arenas = CopyArenas(max(SEG_SIZES) + 32, 99)
    for n in SEG_SIZES:
        swins, dwins = [(ms, ms + n)], [(md, md + n)]
        ftar.reduce([arenas.src.ptr(ms)], arenas.dst.ptr(md), n, "u8", "sum")
        arenas.verify(swins, dwins, dict(n=n))
        if n and ms == md:      # <the byte trait, K = 1, U = 1, W = 1, nt, progressive>
            name, targs = ke.template_args(ftar.last_kernel())
            assert name == "reduce_lds_kernel" and targs[1:] == ["1", "1", "1", "2", "true"], (n, ftar.last_kernel())
        elif n:
            assert ftar.last_kernel() == "gather_kernel<true, false>", n
