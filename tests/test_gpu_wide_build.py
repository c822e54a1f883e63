"""GPU parity of wide model construction: rc_histogram_wide against numpy counts (exact
integers, every mode, every copy count of the counter layout, chunks at every 16-B load phase),
build_wide_model's table against the oracle quantiser with a round trip through the wide coders,
and rc_ideal_bits_wide against wide_build_ref.ideal_bits_ref.

The ideal-bits tolerance (rtol 1e-12): the chunks here hold at most 2000 symbols and the GPU adds
them as 64 partial sums and a butterfly, so its relative error is at most about
(2000 / 64 + 6 + 1) * 2^-53 < 50 * 2^-53 = 5.6e-15; the reference's bin-ordered sum of at most
4096 positive terms is within 4096 * 2^-53 = 4.5e-13.  Both are below 1e-12."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from range_coder_rust_amd.api import _ptr  # noqa: E402
from oracle import model_build as O  # noqa: E402
from gpu_helpers import dev  # noqa: E402
from wide_build_ref import hist_ref, ideal_bits_ref, zipf_counts  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def arena(values, shift=0):
    """An int16 tensor holding the uint16 `values`, its first symbol `shift` symbols past an
    allocation's (256-B aligned) start: the shift sets the phase of the kernels' 16-B loads."""
    v = np.ascontiguousarray(values, np.uint16).view(np.int16)
    big = torch.zeros(len(v) + shift + 64, dtype=torch.int16, device="cuda")
    view = big[shift:shift + len(v)]
    view.copy_(dev(v))
    assert view.data_ptr() % 16 == (2 * shift) % 16
    return view


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def ragged_lens(rng, n, lo, hi):
    lens = rng.integers(lo, hi + 1, n)
    lens[rng.random(n) < 0.1] = 0  # empty chunks
    return lens


def zipf_draw(rng, n, tot):
    c, _, total = zipf_counts(n)
    return rng.choice(n, tot, p=c.astype(np.float64) / total).astype(np.uint16)


def shared_bank_bins(n_bins):
    """Two bins whose counters share LDS banks: counter word = bin * copies + copy and an LDS
    atomic has 32 banks, so bins 32 / copies apart do (with 32 copies any two bins do)."""
    copies = int(N.load().rc_histogram_wide_copies_(n_bins))
    a = min(5, n_bins - 1)
    return a, min(a + max(1, 32 // copies), n_bins - 1)


def draw(rng, kind, n_bins, tot):
    if kind == "uniform":
        return rng.integers(0, n_bins, tot).astype(np.uint16)
    if kind == "zipf":
        return zipf_draw(rng, n_bins, tot)
    if kind == "constant":  # one bin takes every symbol
        return np.full(tot, n_bins // 3, np.uint16)
    if kind == "last":
        return np.full(tot, n_bins - 1, np.uint16)
    a, b = shared_bank_bins(n_bins)
    return np.where(rng.random(tot) < 0.5, a, b).astype(np.uint16)


def rows_ref(data, off, n_bins):
    """(rows int64[n, n_bins], batch int64[n_bins], out-of-range count) with numpy."""
    n = len(off) - 1
    s = np.asarray(data[off[0]:off[-1]], np.int64)
    chunk = np.repeat(np.arange(n), np.diff(off))
    ok = s < n_bins
    rows = np.bincount(chunk[ok] * n_bins + s[ok], minlength=n * n_bins).reshape(n, n_bins)
    batch, stray = hist_ref(s, n_bins)
    assert (rows.sum(0) == batch).all() and stray == int((~ok).sum())
    return rows, batch, stray


def check_hist(data, off, n_bins, shift):
    """Rows and batch together, batch only (rows NULL) and rows only (hist NULL)."""
    rows, batch, stray = rows_ref(data, off, n_bins)
    syms, doff = arena(data, shift), dev(off)
    hist, ch, oob = rc.histogram_wide(syms, doff, n_bins, per_chunk=True)
    assert ch.shape == rows.shape
    assert (ch.cpu().numpy() == rows).all()
    assert (hist.cpu().numpy() == batch).all() and int(oob) == stray
    hist, ch, oob = rc.histogram_wide(syms, doff, n_bins)
    assert ch is None and (hist.cpu().numpy() == batch).all() and int(oob) == stray
    hist, ch, oob = rc.histogram_wide(syms, doff, n_bins, per_chunk=True, batch=False)
    assert hist is None and (ch.cpu().numpy() == rows).all() and int(oob) == stray


@pytest.mark.parametrize("shift", [0, 1, 3, 7])
@pytest.mark.parametrize("kind", ["uniform", "zipf", "constant", "last", "pair"])
@pytest.mark.parametrize("n_bins", [1, 255, 256, 257, 1000, 4095, 4096])
def test_histogram_matches_numpy(ctx, n_bins, kind, shift):
    rng = np.random.default_rng(n_bins * 100 + shift * 10 + len(kind))
    lens = ragged_lens(rng, 300, 0, 5000)
    check_hist(draw(rng, kind, n_bins, int(lens.sum())), offsets(lens), n_bins, shift)


@pytest.mark.parametrize("shift", [0, 3, 7])
def test_histogram_chunks_shorter_than_a_head(ctx, shift):
    rng = np.random.default_rng(shift)
    lens = rng.integers(1, 10, 300)
    check_hist(draw(rng, "zipf", 1000, int(lens.sum())), offsets(lens), 1000, shift)


def test_histogram_out_of_range_symbols(ctx):
    """Symbols >= n_bins (the first one past the bins, the last wide symbol, the first value
    past every wide alphabet, 65535) are counted in oob and move no bin."""
    rng = np.random.default_rng(11)
    lens = ragged_lens(rng, 300, 0, 5000)
    data = draw(rng, "zipf", 1000, int(lens.sum()))
    where = rng.random(len(data)) < 0.05
    data[where] = rng.choice(np.array([1000, 4095, 4096, 65535], np.uint16), int(where.sum()))
    off = offsets(lens)
    rows, batch, stray = rows_ref(data, off, 1000)
    assert stray == int(where.sum()) > 0
    check_hist(data, off, 1000, 3)
    # oob_dev = NULL is accepted, and the bins are the same
    syms, doff = arena(data, 1), dev(off)
    hist = torch.zeros(1000, dtype=torch.int64, device="cuda")
    ctx.bind_stream()
    assert ctx._lib.rc_histogram_wide(ctx.handle, _ptr(syms), _ptr(doff), len(lens), 1000, None,
                                      _ptr(hist), None) == N.RC_OK
    assert (hist.cpu().numpy() == batch).all()
    # with every result NULL the call does nothing
    assert ctx._lib.rc_histogram_wide(ctx.handle, _ptr(syms), _ptr(doff), len(lens), 1000, None,
                                      None, None) == N.RC_OK


def test_histogram_accumulates(ctx):
    rng = np.random.default_rng(12)
    lens = ragged_lens(rng, 300, 0, 5000)
    data = draw(rng, "uniform", 1200, int(lens.sum()))  # a sixth of it out of range
    syms, doff = arena(data), dev(offsets(lens))
    hist, _, oob = rc.histogram_wide(syms, doff, 1000)
    first, first_oob = hist.clone(), oob.clone()
    assert int(first_oob) > 0
    ctx.bind_stream()
    assert ctx._lib.rc_histogram_wide(ctx.handle, _ptr(syms), _ptr(doff), len(lens), 1000, None,
                                      _ptr(hist), _ptr(oob)) == N.RC_OK
    torch.cuda.synchronize()
    assert torch.equal(hist, 2 * first) and int(oob) == 2 * int(first_oob)


@pytest.mark.parametrize("n_bins", [256, 4096])
def test_histogram_one_long_constant_chunk(ctx, n_bins):
    """The counters are plain u32 words that are flushed into the u64 results before 2^32
    symbols have been counted since the last flush, and read out on no other schedule: that
    boundary cannot be reached in a few seconds.  Instead: one chunk of 5 Mi symbols of one
    value (every count into one bin's copies), between two short chunks."""
    lens = np.array([3, 5 << 20, 11], np.int64)
    data = np.full(int(lens.sum()), n_bins - 2, np.uint16)
    data[:3] = [0, 1, n_bins - 1]
    check_hist(data, offsets(lens), n_bins, 5)


def test_histogram_argument_errors(ctx):
    syms = torch.zeros(64, dtype=torch.int16, device="cuda")
    off = dev(np.array([0, 32], np.int64))
    hist = torch.zeros(4096, dtype=torch.int64, device="cuda")
    call = ctx._lib.rc_histogram_wide
    ctx.bind_stream()
    assert call(ctx.handle, _ptr(syms), _ptr(off), 1, 0, None, _ptr(hist), None) == N.RC_E_ARG
    assert call(ctx.handle, _ptr(syms), _ptr(off), 1, 4097, None, _ptr(hist), None) == N.RC_E_ARG
    odd = ctypes.c_void_p(syms.data_ptr() + 1)
    assert call(ctx.handle, odd, _ptr(off), 1, 256, None, _ptr(hist), None) == N.RC_E_ARG
    assert call(ctx.handle, None, _ptr(off), 1, 256, None, _ptr(hist), None) == N.RC_E_ARG
    assert call(ctx.handle, _ptr(syms), None, 1, 256, None, _ptr(hist), None) == N.RC_E_ARG
    assert call(ctx.handle, None, None, 0, 256, None, _ptr(hist), None) == N.RC_OK
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0
    with pytest.raises(ValueError):
        rc.histogram_wide(syms, off, 4097)


# ------------------------------------------------------------------------ build_wide_model
@pytest.mark.parametrize("T,all_symbols", [(1 << 16, True), (4096, False)])
@pytest.mark.parametrize("n", [300, 4096])
def test_build_wide_model_table_and_round_trip(ctx, n, T, all_symbols):
    rng = np.random.default_rng(n + T)
    lens = rng.integers(100, 3001, 64)
    data, off = zipf_draw(rng, n, int(lens.sum())), offsets(lens)
    m = rc.build_wide_model(arena(data, 3), dev(off), n, target_total=T, all_symbols=all_symbols)
    want = O.quantize_counts(np.bincount(data, minlength=n), T,
                             O.Q_ALL_SYMBOLS if all_symbols else 0)
    assert m.n_symbols == n
    assert list(m.c) == want[0] and list(m.cum) == want[1] and m.total == want[2]
    chunks = [data[off[k]:off[k + 1]] for k in range(len(lens))]
    codes = rc.encode_chunks_wide(m, chunks)
    dec = rc.decode_chunks_wide(m, codes, [len(x) for x in chunks])
    assert all((np.asarray(d) == x).all() for d, x in zip(dec, chunks))


def test_build_wide_model_refuses_stray_symbols(ctx):
    data = np.arange(600, dtype=np.uint16) % 300
    data[[17, 400]] = [300, 65535]
    with pytest.raises(ValueError, match="2 symbols >= 300"):
        rc.build_wide_model(arena(data), dev(np.array([0, 600], np.int64)), 300)


# ------------------------------------------------------------------------------ ideal bits
@pytest.fixture(scope="module", params=[4096, 300])
def wide_table(request, ctx):
    c, cum, total = zipf_counts(request.param)
    return c, total, rc.WideStaticModel(c, cum, total, ctx=ctx)


@pytest.mark.parametrize("n", [1, 255, 256, 1000])
def test_ideal_bits_matches_reference(wide_table, n):
    c, total, model = wide_table
    rng = np.random.default_rng(n + len(c))
    lens = ragged_lens(rng, n, 0, 2000)
    data, off = zipf_draw(rng, len(c), int(lens.sum())), offsets(lens)
    bits = rc.ideal_bits_wide(model, arena(data, n % 8), dev(off)).cpu().numpy()
    want = ideal_bits_ref([data[off[k]:off[k + 1]] for k in range(n)], c, total)
    assert bits.shape == (n,) and np.isfinite(want).all()
    np.testing.assert_allclose(bits, want, rtol=1e-12, atol=0)
    assert (bits[lens == 0] == 0.0).all()  # exactly


def test_ideal_bits_inf_chunks_have_finite_neighbours(ctx):
    c, _, _ = zipf_counts(300)
    c[0] += c[7]
    c[7] = 0
    model = rc.WideStaticModel(c, ctx=ctx)
    ok = np.arange(40, dtype=np.uint16) + 8
    chunks = [ok, np.append(ok, 7), ok[:9], np.append(ok, 300), ok[:1],
              np.insert(ok, 3, 65535), ok]
    chunks = [np.asarray(x, np.uint16) for x in chunks]
    off = offsets([len(x) for x in chunks])
    bits = rc.ideal_bits_wide(model, arena(np.concatenate(chunks), 1), dev(off)).cpu().numpy()
    want = ideal_bits_ref(chunks, c, model.total)
    assert [math.isinf(x) for x in want] == [False, True, False, True, False, True, False]
    assert (np.isinf(bits) == np.isinf(want)).all() and (bits[np.isinf(bits)] > 0).all()
    fin = np.isfinite(want)
    np.testing.assert_allclose(bits[fin], want[fin], rtol=1e-12, atol=0)


def test_ideal_bits_takes_wide_models_only(ctx):
    c, cum, total = zipf_counts(256)
    syms = torch.zeros(64, dtype=torch.int16, device="cuda")
    off = dev(np.array([0, 32], np.int64))
    bits = torch.zeros(1, dtype=torch.float64, device="cuda")
    call = ctx._lib.rc_ideal_bits_wide
    ctx.bind_stream()
    static = rc.StaticModel(c, cum, total, ctx=ctx)
    mset = rc.StaticModelSet.from_counts(np.stack([c, c[::-1]]).astype(np.uint64), ctx=ctx)
    for other in (static, mset):
        assert call(ctx.handle, other.handle, _ptr(syms), _ptr(off), 1, _ptr(bits)) == N.RC_E_ARG
    wide = rc.WideStaticModel(c, cum, total, ctx=ctx)
    odd = ctypes.c_void_p(syms.data_ptr() + 1)
    assert call(ctx.handle, wide.handle, odd, _ptr(off), 1, _ptr(bits)) == N.RC_E_ARG
    assert call(ctx.handle, wide.handle, None, _ptr(off), 1, _ptr(bits)) == N.RC_E_ARG
    assert call(ctx.handle, wide.handle, None, None, 0, None) == N.RC_OK
    assert call(ctx.handle, wide.handle, _ptr(syms), _ptr(off), 1, _ptr(bits)) == N.RC_OK
    torch.cuda.synchronize()
    assert float(bits[0]) == pytest.approx(32 * math.log2(total / int(c[0])), rel=1e-12)


def test_code_length_vs_ideal_wide(ctx):
    """The entropy report for a wide model: coded bytes against the ideal code length of the
    same table, 256 chunks of 16 Ki symbols drawn from the table on the device; the bound is the
    one test_code_length_vs_ideal uses for the same arithmetic."""
    n, L = 256, 16384
    c, cum, total = zipf_counts(4096)
    m = rc.WideStaticModel(c, cum, total, ctx=ctx)
    g = torch.Generator(device="cuda").manual_seed(7)
    r = torch.randint(0, total, (n * L,), device="cuda", generator=g)
    ends = torch.from_numpy(np.cumsum(c.astype(np.int64))).to("cuda")
    sym64 = torch.searchsorted(ends, r, right=True)  # s with cum[s] <= r < cum[s] + c[s]
    syms = sym64.to(torch.int16)
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    hist, _, oob = rc.histogram_wide(syms, off, 4096)
    assert torch.equal(hist, torch.bincount(sym64, minlength=4096)) and int(oob) == 0
    ideal = rc.ideal_bits_wide(m, syms, off)
    cap = rc.slot_capacity(L, m.max_bits_per_symbol() + 1)
    out = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    out_len, fl = rc.encode_batch_wide(m, syms, off, out,
                                       torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap)
    assert int(fl.abs().sum()) == 0
    over = (out_len.double() * 8 - ideal).cpu().numpy()
    assert (over > 0).all() and (over < 64 + 0.01 * L).all()
