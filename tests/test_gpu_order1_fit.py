"""GPU parity of fitting an order-1 set: rc_histogram_pairs against numpy pair counts (exact
integers) and against rc_histogram_order1, rc_ideal_bits_order1 against numpy f64, and
fit_order1_set end to end on the K = 8 recovery data of test_order1_fit.py.

The ideal-bits tolerance (rtol 1e-12): the kernel adds a chunk of n_k symbols as 64 partial sums,
each in runs of 16 consecutive symbols at a stride of 1024, and a 6-step butterfly, so its
relative error is at most about (n_k / 64 + 22) * 2^-53, which stays below 1e-12 up to
n_k = 5.7e5.  The longest chunk here holds 70,000 symbols: (70000 / 64 + 22) * 2^-53 = 1.3e-13,
and numpy's pairwise sum of the reference is within about 20 * 2^-53.  So no length of this
file needs a cap below what the pair-count tests use."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from range_coder_rust_amd import model_build as mb  # noqa: E402
from range_coder_rust_amd.api import _ptr  # noqa: E402
from gpu_helpers import dev  # noqa: E402
import order1_fit_ref as R  # noqa: E402

# 0, 1, 2 and the 16-B load's edges; one full stride of a workgroup of 256, 512 and 1024 lanes
# x 16 symbols and its neighbours; one chunk of several strides
LENGTHS = [0, 1, 2, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 70000]
SMALL = [0, 1, 2, 15, 16, 17, 33, 100]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def layout(chunks, shift=0):
    """(syms, sym_off) on the device: the chunks back to back, the first one `shift` bytes past
    an allocation's (256-B aligned) start."""
    flat = np.concatenate([np.asarray(c, np.uint8) for c in chunks] + [np.zeros(0, np.uint8)])
    big = torch.zeros(len(flat) + shift + 64, dtype=torch.uint8, device="cuda")
    view = big[shift:shift + len(flat)]
    if len(flat):
        view.copy_(dev(flat))
    assert big.data_ptr() % 256 == 0
    off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64) + shift
    return big, dev(off)


def pairs_gpu(ctx, chunks, shift=0, **kw):
    syms, off = layout(chunks, shift)
    pair, first = mb.histogram_pairs(syms, off, ctx=ctx, **kw)
    torch.cuda.synchronize()
    return pair.cpu().numpy(), first.cpu().numpy()


def check_pairs(ctx, chunks, shift=0):
    pair, first = pairs_gpu(ctx, chunks, shift)
    want_pair, want_first = R.pair_counts_ref(chunks)
    assert np.array_equal(first, want_first)
    assert np.array_equal(pair, want_pair)
    return pair, first


def zipfish(rng, n):
    """Skewed bytes that still reach every context."""
    return np.minimum(rng.geometric(0.03, n) - 1, 255).astype(np.uint8) ^ \
        (rng.integers(0, 256, n) * (rng.random(n) < 0.2)).astype(np.uint8)


# ---- pair counts ----

def test_pairs_lengths(ctx):
    rng = np.random.default_rng(11)
    check_pairs(ctx, [zipfish(rng, n) for n in LENGTHS])


@pytest.mark.parametrize("shift", range(16))
def test_pairs_every_alignment(ctx, shift):
    rng = np.random.default_rng(100 + shift)
    check_pairs(ctx, [rng.integers(0, 256, n).astype(np.uint8) for n in SMALL + [4097]], shift)


def test_pairs_do_not_cross_chunk_boundaries(ctx):
    A, B = 200, 13
    rng = np.random.default_rng(12)
    chunks = []
    for n in (2, 3, 16, 17, 31, 32, 33, 500, 4096, 4097):
        s = rng.integers(0, 256, n).astype(np.uint8)
        s[0], s[-1] = B, A
        chunks.append(s)
    chunks[3][5:7] = (A, B)  # in-chunk occurrences
    chunks[7][15:17] = (A, B)
    pair, first = check_pairs(ctx, chunks)
    inside = sum(int(np.sum((c[:-1] == A) & (c[1:] == B))) for c in chunks)
    assert inside >= 2 and pair[A, B] == inside
    assert first[B] == len(chunks) and first.sum() == len(chunks)


def test_pairs_one_counter_past_2_to_16(ctx):
    pair, first = check_pairs(ctx, [np.full(70000, 77, np.uint8)])
    assert pair[77, 77] == 69999 and pair.sum() == 69999 and first[77] == 1


def test_pairs_slice_edges(ctx):
    edges = (0, 63, 64, 127, 128, 191, 192, 255)
    seq = np.array([x for p in edges for x in (p, 0, p, 255)], np.uint8)
    pair, _ = check_pairs(ctx, [seq, seq[::-1].copy(), np.tile(seq, 40)])
    for p in edges:
        assert pair[p, 0] >= 41 and pair[p, 255] >= 41


def test_pairs_more_chunks_than_workgroups(ctx):
    rng = np.random.default_rng(13)
    check_pairs(ctx, list(rng.integers(0, 256, (2100, 3)).astype(np.uint8)))


def test_pairs_accumulate(ctx):
    rng = np.random.default_rng(14)
    chunks = [zipfish(rng, n) for n in (5000, 0, 1, 333)]
    p0 = rng.integers(0, 1 << 40, (256, 256))
    f0 = rng.integers(0, 1 << 40, 256)
    pair, first = pairs_gpu(ctx, chunks, pair_hist=dev(p0), first_hist=dev(f0))
    want_pair, want_first = R.pair_counts_ref(chunks)
    assert np.array_equal(pair, p0 + want_pair) and np.array_equal(first, f0 + want_first)
    syms, off = layout(chunks)
    pair2, first2 = mb.histogram_pairs(syms, off, ctx=ctx)
    mb.histogram_pairs(syms, off, pair_hist=pair2, first_hist=first2, ctx=ctx)
    torch.cuda.synchronize()
    assert np.array_equal(pair2.cpu().numpy(), 2 * want_pair)
    assert np.array_equal(first2.cpu().numpy(), 2 * want_first)


def test_pairs_either_output_may_be_null(ctx):
    rng = np.random.default_rng(15)
    chunks = [zipfish(rng, n) for n in (4097, 0, 1, 2, 20000)]
    want_pair, want_first = R.pair_counts_ref(chunks)
    syms, off = layout(chunks, 3)
    pair = torch.zeros((256, 256), dtype=torch.int64, device="cuda")
    first = torch.zeros(256, dtype=torch.int64, device="cuda")
    ctx.bind_stream()
    call = ctx._lib.rc_histogram_pairs
    n = len(chunks)
    assert call(ctx.handle, _ptr(syms), _ptr(off), n, _ptr(pair), None) == N.RC_OK
    assert call(ctx.handle, _ptr(syms), _ptr(off), n, None, _ptr(first)) == N.RC_OK
    assert call(ctx.handle, _ptr(syms), _ptr(off), n, None, None) == N.RC_OK
    assert call(ctx.handle, None, None, n, None, None) == N.RC_OK  # both null: a no-op
    assert call(ctx.handle, None, _ptr(off), n, _ptr(pair), None) == N.RC_E_ARG
    assert call(ctx.handle, _ptr(syms), _ptr(off), (1 << 28) + 1, _ptr(pair), None) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(pair.cpu().numpy(), want_pair)
    assert np.array_equal(first.cpu().numpy(), want_first)


def test_pairs_pool_into_the_existing_kernels_rows(ctx):
    rng = np.random.default_rng(16)
    chunks = [zipfish(rng, n) for n in (9000, 17, 0, 1, 4096, 2500)]
    K = 11
    cmap = rng.integers(0, K, 256).astype(np.uint8)
    first_row = 4
    syms, off = layout(chunks, 5)
    pair, first = mb.histogram_pairs(syms, off, ctx=ctx)
    rows = mb.histogram_order1(syms, off, cmap, first_row, n_models=K, ctx=ctx)
    torch.cuda.synchronize()
    pair, first, rows = pair.cpu().numpy(), first.cpu().numpy(), rows.cpu().numpy()
    for j in range(K):
        want = pair[cmap == j].sum(axis=0) + (first if j == first_row else 0)
        assert np.array_equal(rows[j], want), j


# ---- ideal bits ----

def random_set(rng, K, n=256, total=1 << 16):
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        w = rng.pareto(1.2, n) + 0.01
        rows[j] += rng.multinomial(total - n, w / w.sum())
    return rows.astype(np.uint32), rng.integers(0, K, n).astype(np.uint8), int(rng.integers(0, K))


def bits_gpu(model, chunks, shift=0):
    syms, off = layout(chunks, shift)
    b = mb.ideal_bits_order1(model, syms, off)
    torch.cuda.synchronize()
    return b.cpu().numpy()


@pytest.mark.parametrize("K", [1, 8, 64])
def test_ideal_bits(ctx, K):
    rng = np.random.default_rng(20 + K)
    c, cmap, fr = random_set(rng, K)
    model = rc.Order1ModelSet(c, None, 1 << 16, ctx_map=cmap, first_row=fr, ctx=ctx)
    for shift, lens in [(0, LENGTHS)] + [(s, SMALL) for s in range(1, 16)]:
        chunks = [zipfish(rng, n) for n in lens]
        got = bits_gpu(model, chunks, shift)
        want = R.ideal_bits_ref(chunks, c, 1 << 16, cmap, fr)
        assert np.isfinite(got).all()
        for k, n in enumerate(lens):
            print(f"K={K} shift={shift} n={n}: rel err "
                  f"{abs(got[k] - want[k]) / max(want[k], 1e-300):.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert got[lens.index(0)] == 0.0
    model.close()


def test_ideal_bits_zero_frequency_under_the_right_context(ctx):
    c = np.full((2, 256), 256, np.uint32)
    c[1, 7], c[1, 8] = 0, 512  # row 1 cannot code symbol 7
    cmap = (np.arange(256) & 1).astype(np.uint8)  # an odd previous symbol picks row 1
    model = rc.Order1ModelSet(c, None, 1 << 16, ctx_map=cmap, first_row=0, ctx=ctx)
    base = np.full(40, 2, np.uint8)
    hit, miss, at0, tail = base.copy(), base.copy(), base.copy(), base.copy()
    hit[20:22] = (3, 7)    # 7 after an odd symbol: row 1, c = 0
    miss[20:22] = (4, 7)   # 7 after an even symbol: row 0
    at0[0] = 7             # 7 first in the chunk: first_row = 0
    tail[38:40] = (1, 7)   # in the symbol-wise tail of the chunk
    chunks = [miss, hit, at0, np.zeros(0, np.uint8), tail, miss]
    got = bits_gpu(model, chunks)
    want = R.ideal_bits_ref(chunks, c, 1 << 16, cmap, 0)
    assert list(np.isinf(got)) == [False, True, False, False, True, False]
    assert not np.isnan(got).any() and got[3] == 0.0 and (got[np.isinf(got)] > 0).all()
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=0)
    model.close()


def test_ideal_bits_symbol_past_the_alphabet(ctx):
    rng = np.random.default_rng(31)
    c, cmap, fr = random_set(rng, 3, n=100)
    model = rc.Order1ModelSet(c, None, 1 << 16, ctx_map=cmap, first_row=fr, ctx=ctx)
    chunks = [rng.integers(0, 100, n).astype(np.uint8) for n in (50, 50, 0, 4097, 17)]
    chunks[1][30] = 100
    chunks[3][4096] = 255
    got = bits_gpu(model, chunks, 9)
    want = R.ideal_bits_ref(chunks, c, 1 << 16, cmap, fr)
    assert list(np.isinf(got)) == [False, True, False, True, False]
    assert not np.isnan(got).any() and got[2] == 0.0
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=0)
    model.close()


def test_ideal_bits_takes_only_order1_sets(ctx):
    c = np.full(256, 256, np.uint32)
    static = rc.StaticModel(c, None, 1 << 16, ctx=ctx)
    mset = rc.StaticModelSet(np.stack([c, c]), None, 1 << 16, ctx=ctx)
    wide = rc.WideStaticModel(c, None, 1 << 16, ctx=ctx)
    o1 = rc.Order1ModelSet(np.stack([c, c]), None, 1 << 16, ctx_map=np.zeros(256, np.uint8),
                           ctx=ctx)
    syms, off = layout([np.zeros(10, np.uint8)])
    bits = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.bind_stream()
    call = ctx._lib.rc_ideal_bits_order1
    for m in (static, mset, wide):
        assert call(ctx.handle, m.handle, _ptr(syms), _ptr(off), 1, _ptr(bits)) == N.RC_E_ARG
    assert call(ctx.handle, None, _ptr(syms), _ptr(off), 1, _ptr(bits)) == N.RC_E_ARG
    assert call(ctx.handle, o1.handle, _ptr(syms), _ptr(off), 1, None) == N.RC_E_ARG
    assert call(ctx.handle, o1.handle, None, None, 0, None) == N.RC_OK
    assert call(ctx.handle, o1.handle, _ptr(syms), _ptr(off), 1, _ptr(bits)) == N.RC_OK
    torch.cuda.synchronize()
    assert float(bits[0]) == pytest.approx(80.0, rel=1e-12)  # 10 symbols at 8 bits
    for m in (static, mset, wide, o1):
        m.close()


# ---- end to end ----

def test_fit_order1_set_end_to_end(ctx):
    K, n, L = 8, 32, 2048
    chunks = R.markov_chunks(K, n, L)
    _, true_map, true_first = R.markov_source(K)
    syms, off = layout(chunks)
    fitted = mb.fit_order1_set(syms, off, n_models=K, ctx=ctx)
    true = mb.build_order1_set(syms, off, true_map, true_first, ctx=ctx)
    order0 = mb.build_model(syms, off, ctx=ctx)
    assert fitted.n_models == K and fitted.first_row == fitted.ctx_map[0]
    want_pair, want_first = R.pair_counts_ref(chunks)
    assert R.partition(want_pair, want_first, fitted.ctx_map, fitted.first_row) == \
        R.partition(want_pair, want_first, true_map, true_first)
    cap = rc.slot_capacity(L, 16.0)
    out_off = dev(np.arange(n + 1, dtype=np.int64) * cap)
    code_off = out_off[:-1].contiguous()

    def encode(fn, model):
        out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        out_len, flags = fn(model, syms, off, out, out_off)
        torch.cuda.synchronize()
        assert int(flags.abs().sum()) == 0
        h, ol = out.cpu().numpy(), out_len.cpu().numpy()
        return out, out_len, [bytes(h[k * cap:k * cap + int(ol[k])]) for k in range(n)]

    out, out_len, got = encode(rc.encode_batch_order1, fitted)
    _, _, want = encode(rc.encode_batch_order1, true)
    assert got == want  # the same table for every symbol, whatever the rows' numbers
    dec = torch.zeros_like(syms)
    fd = rc.decode_batch_order1(fitted, out, code_off, out_len, dec, off)
    torch.cuda.synchronize()
    assert int(fd.abs().sum()) == 0 and torch.equal(dec[:n * L], syms[:n * L])
    _, _, plain = encode(rc.encode_batch, order0)
    assert sum(map(len, got)) < sum(map(len, plain))
    # the batch's ideal bits under the fitted set: the class counts priced by the quantised rows
    bits = mb.ideal_bits_order1(fitted, syms, off)
    torch.cuda.synchronize()
    rows = np.concatenate([want_pair, want_first[None, :]])
    cls = np.concatenate([fitted.ctx_map.astype(np.int64), [fitted.first_row]])
    cost = 0.0
    for j in range(K):
        cnt = rows[cls == j].sum(axis=0).astype(np.float64)
        cost += float(np.sum(cnt * np.log2(fitted.total / fitted.c[j].astype(np.float64))))
    assert float(bits.sum()) == pytest.approx(cost, rel=1e-9)
    assert 8.0 * sum(map(len, got)) >= float(bits.sum())
    for m in (fitted, true, order0):
        m.close()
