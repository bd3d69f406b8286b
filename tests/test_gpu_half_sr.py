"""GPU tests of ftar_cast_half_sr (f32 -> bf16 / f16 with stochastic rounding) and of half_compress_hook.  Every
comparison is bit for bit (NaN lanes as "NaN or not") with tests/half_sr_ref.py; every call runs between guard bytes
(kernel_edges.Arena), so each one also checks its write footprint: the n elements and, with amax, the one word."""
import ctypes

import numpy as np
import pytest

import amax_ref
import cast_ref
import half_sr_ref as hr
import kernel_edges
import sr_ref
from test_gpu_cast_sr import Bucket, _on_threads, group

pytestmark = pytest.mark.gpu
DSTS = ("bf16", "f16")
SEED, TOP, HALF, M64 = 0x0123456789ABCDEF, (1 << 32) - 1, 0x3F000000, (1 << 64) - 1
# past lane 0: inf, -0, the largest finite value, the smallest subnormal, -inf, a NaN
SPECIALS = {3: 0x7F800000, 5: 0x80000000, 6: 0x7F7FFFFF, 9: 0x00000001, 10: 0xFF800000, 12: 0x7FC00001}


def inputs(n, seed=1, specials=True):
    x = amax_ref.base_sources("f32", 2, max(n, 2), seed)[0][:n].copy()      # |x| < 1
    for at, bits in SPECIALS.items() if specials else ():
        x[at:at + 1] = bits
    return x


def run(dst, x, r=None, seed=SEED, offset=0, so=0, do=0, amax=False, words=None):
    """(stored bits, amax word or None, kernel) of one call; words: the bench library's hook in the generator's place."""
    import torch

    import ftar
    n = x.size
    sa, da = kernel_edges.Arena(4 * (n + so) + 16), kernel_edges.Arena(2 * (n + do) + 16)
    am, sd, aux = kernel_edges.Arena(64), kernel_edges.Arena(64), kernel_edges.Arena(4 * n + 16)
    sa.upload(4 * so, x)
    sd.upload(8, np.array([seed & M64], np.uint64))
    aux.upload(0, np.array([cast_ref.ONE if r is None else r], np.uint32))
    if words is None:
        ftar.cast_half_sr(sa.ptr(4 * so), da.ptr(2 * do), n, "f32", dst, sd.ptr(8), scale=None if r is None else aux.ptr(0),
                          offset=offset, amax=am.ptr(16) if amax else None)
    else:
        aux.upload(16, np.broadcast_to(np.asarray(words, np.uint32), (n,)))
        hook = ftar.bench_lib().ftar_bench_cast_half_sr_words
        hook.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 3
        assert hook(sa.ptr(4 * so), 6, da.ptr(2 * do), cast_ref.ID[dst], n, aux.ptr(0), aux.ptr(16), None) == 0
    torch.cuda.synchronize()
    for arena, win in ((sa, (0, 0)), (sd, (0, 0)), (aux, (0, 0)), (da, (2 * do, 2 * (do + n))), (am, (16, 20) if amax else (0, 0))):
        assert kernel_edges.check_untouched(arena, *win) is None
    word = int(am.window(16, 20).cpu().numpy().view(np.uint32)[0]) if amax else None
    return da.window(2 * do, 2 * (do + n)).cpu().numpy().view(np.uint16), word, ftar.last_kernel()


def check(dt, got, want, what=""):
    assert cast_ref.same_bits(dt, got, want), (what, cast_ref.first_diff(dt, got, want))


def tile(dst):
    """The elements one workgroup of half_vec_sr_kernel<Rd, BF, MODE, U, BS, LAYOUT> covers per pass."""
    name, a = kernel_edges.template_args(run(dst, inputs(4099))[2])
    assert name == "half_vec_sr_kernel", name
    return int(a[3]) * int(a[4]) * 8


@pytest.mark.parametrize("dst", DSTS)
def test_counts_heads_and_both_families_against_the_reference(dst):
    """(so, do) = (3, 7) is head 1, (1, 1) head 7, both with a tail; (1, 0) and (0, 1) run the element-wise kernel."""
    T = tile(dst)
    cases = [(n, 0, 0) for n in (0, 1, 7, 8, 9, T - 1, T, T + 1, 3 * T - 1)]
    cases += [(T + 11, 3, 7), (T + 11, 1, 1), (T + 11, 4, 8), (T + 11, 1, 0), (T + 11, 0, 1)]
    for i, (n, so, do) in enumerate(cases):
        x, r = inputs(n, seed=2), (None, HALF, cast_ref.THIRD)[i % 3]
        want = hr.sr_cast(dst, x, r, SEED, 11)
        got, _, k0 = run(dst, x, r, SEED, 11, so, do)
        got_a, word, k1 = run(dst, x, r, SEED, 11, so, do, amax=True)
        check(dst, got, want, (n, so, do))
        check(dst, got_a, want, (n, so, do, "amax"))
        assert amax_ref.matches(word, amax_ref.amax_bits(dst, want)), (n, so, do, hex(word))
        assert sorted(np.flatnonzero(cast_ref.nan_mask(dst, got))) == [p for p in (12,) if p < n]
        family = "half_elem_sr" if (so, do) in ((1, 0), (0, 1)) else "half_vec_sr"
        assert n == 0 or (k0.startswith(family + "_kernel<") and k1.startswith(family + "_amax_kernel<")), (k0, k1)


@pytest.mark.parametrize("low", (0x0001, 0x7FFF, 0x8000, 0xFFFF), ids=hex)
@pytest.mark.parametrize("dst", DSTS)
def test_every_f32_high_half_under_the_edge_words(dst, low):
    """Pins the narrowing: 0, 2^32 - 1, each input's threshold 2^32 - F and the word below it, in both families."""
    x = (np.arange(65536, dtype=np.uint32) << np.uint32(16)) | np.uint32(low)
    thr = ((np.uint64(1) << np.uint64(32)) - hr.frac32(dst, x).astype(np.uint64)) & np.uint64(TOP)
    for w in (0, TOP, thr.astype(np.uint32), ((thr - np.uint64(1)) & np.uint64(TOP)).astype(np.uint32)):
        for so, do in ((0, 0), (0, 1)):
            check(dst, run(dst, x, words=w, so=so, do=do)[0], hr.sr_cast_words(dst, x, None, w), (w, so, do))


@pytest.mark.parametrize("dst", DSTS)
def test_splits_and_offsets_across_2_32_and_at_2_63(dst):
    T = tile(dst)
    x = inputs(2 * T + 5, seed=5)
    for offset in (1000, (1 << 32) - T, 1 << 63, (1 << 64) - 5):
        whole = run(dst, x, HALF, SEED, offset)[0]
        check(dst, whole, hr.sr_cast(dst, x, HALF, SEED, offset), hex(offset))
        for a in (1, T - 3, T + 1):
            parts = np.concatenate([run(dst, x[:a], HALF, SEED, offset)[0], run(dst, x[a:], HALF, SEED, offset + a)[0]])
            assert parts.tobytes() == whole.tobytes(), (hex(offset), a)


@pytest.mark.parametrize("dst", DSTS)
def test_amax_sees_a_nan_and_an_inf(dst):
    x = inputs(4099, 7, specials=False)
    for bits, want in ((x[300], None), (0x7FC00000, amax_ref.NAN), (0xFF800000, 0x7F800000), (0x7F7FFFFF, 0x7F800000)):
        x[300] = bits      # the last: an overflow at the cast (bf16: under this seed's word)
        got, word, _ = run(dst, x, None, SEED, amax=True)
        ref = hr.sr_cast(dst, x, None, SEED)
        check(dst, got, ref)
        assert amax_ref.matches(word, amax_ref.amax_bits(dst, ref) if want is None else want), hex(word)


@pytest.mark.parametrize("dst", DSTS)
def test_a_captured_cast_follows_the_device_seed(dst):
    import torch

    import ftar
    n = 100_003
    x = inputs(n, seed=8)
    s = torch.from_numpy(x.view(np.float32).copy()).cuda()
    out = torch.empty(n, dtype=torch.int16, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        ftar.cast_half_sr(s, out, n, "f32", dst, seed, offset=123, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    for sv in (5, 6, -1, 5):
        seed.fill_(sv)
        g.replay()
        torch.cuda.synchronize()
        check(dst, out.cpu().numpy().view(np.uint16), hr.sr_cast(dst, x, None, sv & M64, 123), sv)


@pytest.mark.parametrize("rounding", ["stochastic", "nearest"])
@pytest.mark.parametrize("fmt", DSTS)
@pytest.mark.parametrize("P", [2, 4])
def test_half_compress_hook_over_threads(P, fmt, rounding):
    """Two buckets in a row, one-stage topology: each rank's own seed at the running offset, one averaged wire."""
    import torch

    import ftar.ddp
    base, g, offset, sr = 99, group(P), 0, rounding == "stochastic"
    states = [ftar.ddp.HalfCompressState(g[r], fmt=fmt, topo=str(P), rounding=rounding, seed=base) for r in range(P)]
    for b, n in enumerate((20_001, 4099)):
        ins = [x[:n] for x in amax_ref.base_sources("f32", P, 20_001, seed=9 + b)]
        wire = [hr.sr_cast(fmt, x, None, sr_ref.rank_seed(base, r), offset) if sr else cast_ref.rne16_bits(fmt, x)
                for r, x in enumerate(ins)]
        red = amax_ref.schedule(fmt, wire, str(P), "avg")
        ts = [torch.from_numpy(x.view(np.float32).copy()).cuda() for x in ins]
        _on_threads(P, lambda r: ftar.ddp.half_compress_hook(states[r], Bucket(ts[r])).wait())
        offset += n if sr else 0
        for r in range(P):
            check("f32", ts[r].cpu().numpy().view(np.uint32), cast_ref.widen_bits(fmt, red), (b, r))
            check(fmt, states[r]._wire[:n].view(torch.int16).cpu().numpy().view(np.uint16), red, (b, r))
            assert states[r].offset == offset and states[r].calls == b + 1 and float(states[r].found_inf()) == 0.0
            assert not sr or int(states[r].seed.cpu().numpy().view(np.uint64)[0]) == sr_ref.rank_seed(base, r)
