"""Write footprint and tile-edge sizes of the fp8 folds, on the helpers of tests/kernel_edges.py as they are
(Arena and check_untouched through Fold, geometry() of the launched kernel's name, edge_counts(16, wg_tile): 16
fp8 elements to a 16-byte vector).  Every launch writes into a guarded arena: the payload must equal the CPU
expectation of tests/f8_ref.py byte for byte (finite inputs: no NaN lane, whose payload would be open), every
byte outside [dst, dst + n) must still hold its filler, and the sources must be unchanged."""
import numpy as np
import pytest

import f8_ref as ref
import kernel_edges as ke

pytestmark = pytest.mark.gpu

VE = 16
QUARTER = 0.25


def api(dt, op="sum", shape=None, scale=None):
    def launch(srcs, dst, n):
        import ftar
        ftar.reduce(srcs, dst, n, dt, op, shape=list(shape) if shape else None, scale=scale)
    return launch


def hop(dt):
    """The ring's one-round fold, which only the engine asks for (round_each): ftar_debug_reduce_ex."""
    def launch(srcs, dst, n):
        ke.reduce_ex(srcs, dst, n, dt, "sum", round_each=True)
    return launch


def probe(launch, k):
    """The id of the kernel `launch` takes for co-aligned pointers and a count with vectors."""
    import ftar
    import torch
    rows = torch.zeros((k + 1, 66 * 16 + 32), dtype=torch.uint8, device="cuda")
    launch([rows[j].data_ptr() for j in range(k)], rows[k].data_ptr(), 65 * VE)
    torch.cuda.synchronize()
    return ftar.last_kernel()


CASES = {
    # name: (launcher, dtype, k, expectation(ins), the launched kernel's family, what its id names)
    "e4m3_sum_k2_lds": (api("f8e4m3"), "f8e4m3", 2, lambda i: ref.fold("f8e4m3", i),
                        "reduce_lds_kernel", ("reduce_lds_kernel<F8SumT<F8Fmt<false>", ", 2, ")),
    "e4m3_sum_k9_registers": (api("f8e4m3"), "f8e4m3", 9, lambda i: ref.fold("f8e4m3", i),
                               "reduce_vec_kernel", ("reduce_vec_kernel<F8SumT<F8Fmt<false>", ", 0, ")),
    "e4m3_hop_k3": (hop("f8e4m3"), "f8e4m3", 3, lambda i: ref.hop_fold("f8e4m3", i),
                    "reduce_lds_kernel", ("reduce_lds_kernel<F8SumHopT<F8Fmt<false>", ", 3, ")),
    "e4m3_nested_2x2": (api("f8e4m3", shape=(2, 2)), "f8e4m3", 4, lambda i: ref.nested("f8e4m3", i, (2, 2)),
                        "reduce_tree_lds_kernel", ("reduce_tree_lds_kernel<F8SumT<F8Fmt<false>", "StaticShape<2, 2>")),
    "e4m3_scaled_k2": (api("f8e4m3", scale=QUARTER), "f8e4m3", 2,
                       lambda i: ref.fold("f8e4m3", i, ref.scale_of(QUARTER)),
                       "reduce_lds_kernel", ("reduce_lds_scaled_kernel<F8SumT<F8Fmt<false>", ", 2, ")),
    "e5m2_max_k2": (api("f8e5m2", "max"), "f8e5m2", 2, lambda i: ref.minmax("f8e5m2", "max", i),
                    "reduce_lds_kernel", ("reduce_lds_kernel<F8MinMax<F8Fmt<true>, true>", ", 2, ")),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fp8_footprint_at_the_edges(case):
    import ftar
    launch, dt, k, expect, family, named = CASES[case]
    symbol = probe(launch, k)
    g = ke.geometry(symbol)
    assert g.family == family and symbol.startswith(named[0]) and all(x in symbol for x in named[1:]), symbol
    edges = ke.edge_counts(VE, g.wg_tile)
    ins = ref.finite_sources(dt, k, max(e.n for e in edges) + VE)
    want = expect(ins)
    assert not ref.nan_mask(dt, want).any() and not any(ref.nan_mask(dt, x).any() for x in ins)
    assert dt == "f8e4m3" or not ((want & 0x7F) == 0x7C).any()      # nor an inf
    fold = ke.Fold(ins, want)
    for e in edges:
        off = ke.head_offset(VE, e.head)
        srcs, dst = fold.pointers(off)
        launch(srcs, dst, e.n)
        bad = fold.verify(off, e.n)
        assert bad is None, (e, ftar.last_kernel(), bad)
        assert e.nvec < 1 or ftar.last_kernel() == symbol, "one kernel for every count with vectors"
