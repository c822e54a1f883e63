"""Every batch entry point on arenas whose offsets pass 2^32 (tests/high_arena.py).

The chunks are the small ones of the family tests, and the expected bytes come from the same
oracles: where a chunk lies changes nothing about them.  What is new is where the chunks lie: a
few KiB either side of byte 2^32 of a sentinel-filled arena of 4 GiB (8 GiB where the element
index passes 2^32 too).  A kernel that narrows an offset, or the byte address it scales it to,
to 32 bits then reads sentinels instead of the chunk, or writes where untouched() counts it;
test_high_arena_layout.py checks on the host that every layout used here has that property.

Every test allocates its arenas itself and frees them before it returns."""
import gc
import inspect

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N, synth  # noqa: E402
from range_coder_rust_amd import container as CT, model_build as MB  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import dev  # noqa: E402
import container2_ref  # noqa: E402
import direct_table_models  # noqa: E402
import high_arena as H  # noqa: E402
import indexed_ref  # noqa: E402
import lag_ref  # noqa: E402
import order1_ref  # noqa: E402
import periodic_ref  # noqa: E402
import rows_ref as RR  # noqa: E402
import wide_build_ref  # noqa: E402
import wide_ref  # noqa: E402
from test_gpu_rows import as_row, dtab, fresh, ref_decode, ref_encode  # noqa: E402
from test_gpu_wide16 import zipf  # noqa: E402
from test_gpu_wide16_fine import sparse_table  # noqa: E402

SENT = 0xEE
SENT16 = 0xEEEE
MAX = 1 << 25  # RC_MAX_CHUNK_SYMBOLS


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


@pytest.fixture(autouse=True)
def memory_cap():
    """Every test stays a small tenant: its peak lies under high_arena.MEM_CAP, and it leaves
    nothing allocated."""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    gc.collect()
    torch.cuda.empty_cache()
    assert peak <= H.MEM_CAP, f"peak {peak / 2 ** 30:.2f} GiB"


def free():
    """Return what the caller has just dropped (del) to the device."""
    gc.collect()
    torch.cuda.empty_cache()


def draw(rng, c, L, dtype):
    """L symbols of a table: half by frequency, half evenly over the occupied symbols."""
    c = np.asarray(c, np.float64)
    occ = np.flatnonzero(c)
    s = rng.choice(len(c), size=L, p=c / c.sum())
    even = rng.random(L) < 0.5
    s[even] = occ[rng.integers(0, len(occ), int(even.sum()))]
    return s.astype(dtype)


def sym_arena(name, which, chunks, dtype, fill=True):
    """(arena, off) of a case's symbol arena: the chunks at the case's layout, sentinels
    everywhere else.  fill=False leaves the chunks' ranges sentinels too (decoder output)."""
    eb = 2 if dtype == torch.int16 else 1
    off = H.case_layout(name, which, [len(c) for c in chunks])
    place = H.CASES[name]["place" if which == "enc" else "dec_place"]
    t = H.arena(H.place_elems(place, off[-1]), dtype, SENT16 if eb == 2 else SENT)
    if fill:
        H.put(t, off[0], np.concatenate(chunks))
    return t, off


def first_above(off, elem_bytes, boundary, lens, need=1):
    """The last chunk of at least `need` symbols that begins above the boundary."""
    ks = [k for k in range(len(lens)) if off[k] * elem_bytes > boundary and lens[k] >= need]
    assert ks
    return ks[-1]


def coder_case(name, enc, dec, chunks, exp, wide=False, side=None, too_long=False):
    """One family at one placement, both directions.

    enc(syms, sym_off, out, out_off, *side) -> (out_len, flags);
    dec(code, code_off, code_len, syms_out, sym_off, *side) -> flags.
    chunks: one symbol array per chunk; exp: the oracle's (flags, bytes) per chunk; side: None,
    or one uint8 array per chunk that lives in a second arena indexed like the symbols.
    One slot above the boundary is a byte short (RC_F_CAPACITY with the exact length), one
    stream above the boundary is cut to 7 bytes (RC_F_TRUNCATED).  too_long: a last chunk claims
    2^25 + 1 symbols from the end of the real ones on; it is flagged and nothing of it is read
    or written."""
    case = H.CASES[name]
    eb, boundary, _ = H.PLACEMENTS[case["place"]]
    dtype, sent = (torch.int16, SENT16) if wide else (torch.uint8, SENT)
    n = len(chunks)
    lens = [len(c) for c in chunks]
    assert all(f == 0 for f, _ in exp)
    flat = np.concatenate(chunks)

    def with_long(off):
        return np.concatenate([off, [off[-1] + MAX + 1]]) if too_long else off

    # ---- encode
    syms, off = sym_arena(name, "enc", chunks, dtype)
    side_t = ()
    if side is not None:
        side_t = (H.arena(syms.numel(), torch.uint8, SENT),)
        H.put(side_t[0], off[0], np.concatenate(side))
    caps = np.array([len(b) + (0, 5, 16)[k % 3] for k, (_, b) in enumerate(exp)], np.int64)
    short = first_above(off, eb, boundary, [len(b) for _, b in exp], need=9)
    caps[short] = len(exp[short][1]) - 1
    if too_long:
        caps = np.concatenate([caps, [2048]])
    out_off, caps = H.slot_layout(caps, mode=case["slots"])
    out = H.arena(H.place_elems("u8", out_off[-1]), torch.uint8, SENT)
    out_len, flags = enc(syms, dev(with_long(off)), out, dev(out_off), *side_t)
    torch.cuda.synchronize()
    fl, ol = flags.cpu().numpy(), out_len.cpu().numpy()
    h = H.window(out, out_off[0], out_off[-1])
    rel = out_off - out_off[0]
    for k, (f, b) in enumerate(exp):
        if k == short:
            assert (int(fl[k]), int(ol[k])) == (N.F_CAPACITY, len(b)), (name, k, fl[k], ol[k])
            continue
        assert (int(fl[k]), int(ol[k])) == (0, len(b)), (name, k, lens[k], fl[k], ol[k], len(b))
        assert bytes(h[rel[k]:rel[k] + len(b)]) == b, (name, k, lens[k])
    if too_long:
        assert (int(fl[n]), int(ol[n])) == (N.F_TOO_LONG, 0)
        assert (h[rel[n]:] == SENT).all()  # the flagged chunk's slot
    assert H.untouched(out, [(out_off[0], out_off[-1])], SENT) == 0, name
    assert H.untouched(syms, [(off[0], off[-1])], sent) == 0, name
    assert np.array_equal(H.window(syms, off[0], off[-1]), flat), name
    del out, syms, h  # (the decode's arenas are of the same sizes and take their place)

    # ---- decode, from the oracle's bytes
    codes = [b for _, b in exp] + ([bytes([SENT]) * 64] if too_long else [])
    code_len = np.array([len(b) for b in codes], np.int64)
    code_off = H.code_layout(code_len, seed=case["seed"])
    code = H.arena(H.place_elems("u8", int((code_off + code_len).max())), torch.uint8, SENT)
    for k, b in enumerate(codes):
        H.put(code, code_off[k], np.frombuffer(b, np.uint8))
    dec_out, doff = sym_arena(name, "dec", chunks, dtype, fill=False)
    if side is not None:
        side_t[0].fill_(SENT)
        H.put(side_t[0], doff[0], np.concatenate(side))
    cut = [k for k in range(n) if doff[k] * eb > boundary and code_off[k] > H.BOUNDARY
           and lens[k] >= 1][-1]
    code_len[cut] = 7
    fd = dec(code, dev(code_off), dev(code_len), dec_out, dev(with_long(doff)), *side_t)
    torch.cuda.synchronize()
    fd = fd.cpu().numpy()
    got = H.window(dec_out, doff[0], doff[-1])
    drel = doff - doff[0]
    for k, s in enumerate(chunks):
        if k == cut:
            assert int(fd[k]) == N.F_TRUNCATED, (name, k, fd[k])
            continue
        assert int(fd[k]) == 0, (name, k, lens[k], fd[k])
        assert np.array_equal(got[drel[k]:drel[k + 1]], s), (name, k, lens[k])
    if too_long:
        assert int(fd[n]) == N.F_TOO_LONG
    assert H.untouched(dec_out, [(doff[0], doff[-1])], sent) == 0, name
    del code, dec_out, side_t, got
    free()


# ------------------------------------------------------------------- 1. 8-bit static coders
def static_tables():
    out = {"static_zipf": synth.zipf_table(), "static_uniform": synth.uniform_table()}
    c = direct_table_models._zipf(1 << 20)  # a total above 2^16: the wide route
    out["static_total_2p20"] = (c, direct_table_models.cum_of(c), 1 << 20)
    out["static_direct_table"] = direct_table_models.models()["sparse"]
    return out


def static_case(name, table, too_long=False):
    c, cum, total = table
    c, cum = np.asarray(c, np.uint32), np.asarray(cum, np.uint32)
    m = rc.StaticModel(c, cum, int(total))
    rng = np.random.default_rng(H.CASES[name]["seed"])
    chunks = [draw(rng, c, int(L), np.uint8) for L in H.case_lens(name)]
    exp = [cpu.encode(c, cum, int(total), s)[:2] for s in chunks]
    coder_case(name, lambda *a: rc.encode_batch(m, *a), lambda *a: rc.decode_batch(m, *a),
               chunks, exp, too_long=too_long)
    m.close()


@pytest.mark.parametrize("name", ["static_zipf", "static_uniform", "static_total_2p20",
                                  "static_direct_table"])
def test_static_coders(ctx, name):
    static_case(name, static_tables()[name])


# ------------------------------------------------------------------- 2. adaptive coders
@pytest.mark.parametrize("n_alpha", [256, 128])
def test_adaptive_coders(ctx, n_alpha):
    name = f"adaptive_{n_alpha}"
    p = rc.ADAPTIVE_DEFAULTS
    m = rc.AdaptiveModel(n_alpha, **p)
    rng = np.random.default_rng(H.CASES[name]["seed"])
    w = 1.0 / np.arange(1, n_alpha + 1) ** 1.1
    chunks = [draw(rng, w, int(L), np.uint8) for L in H.case_lens(name)]
    exp = [cpu.encode_adaptive(n_alpha, p["increment"], p["limit"], p["period"], s)[:2]
           for s in chunks]
    coder_case(name, lambda *a: rc.encode_batch(m, *a), lambda *a: rc.decode_batch(m, *a),
               chunks, exp)
    m.close()


# ------------------------------------------------------------------- 3. indexed sets
def test_indexed_set(ctx):
    name, K = "indexed_k8", 8
    rng = np.random.default_rng(H.CASES[name]["seed"])
    c, cum = indexed_ref.tables(order1_ref.markov_rows(rng, K, 256, 65536))
    ms = rc.StaticModelSet(c, cum, 65536)
    chunks = [draw(rng, c[0], int(L), np.uint8) for L in H.case_lens(name)]
    idx = [rng.integers(0, K, len(s)).astype(np.uint8) for s in chunks]
    exp = [indexed_ref.encode_ref(c, cum, 65536, s, x) for s, x in zip(chunks, idx)]

    def enc(syms, sym_off, out, out_off, idx_t):
        return rc.encode_batch_indexed(ms, syms, idx_t, sym_off, out, out_off)

    def dec(code, code_off, code_len, syms_out, sym_off, idx_t):
        return rc.decode_batch_indexed(ms, code, code_off, code_len, idx_t, syms_out, sym_off)

    coder_case(name, enc, dec, chunks, exp, side=idx)
    ms.close()


# ------------------------------------------------------------------- 4. order-1 sets
def order1_case(name, P, D, too_long=False):
    K = 8
    rng = np.random.default_rng(H.CASES[name]["seed"])
    c, cum = indexed_ref.tables(order1_ref.markov_rows(rng, K, 256, 65536))
    cm = rng.integers(0, K, (P, 256)).astype(np.uint8)
    first_row = 3
    o1 = rc.Order1ModelSet(c, cum, 65536, ctx_map=cm if P > 1 else cm[0], first_row=first_row,
                           period=P, lag=D)
    chunks = [draw(rng, c[int(rng.integers(0, K))], int(L), np.uint8)
              for L in H.case_lens(name)]
    if D > 1:
        exp = [lag_ref.encode_ref(c, cum, 65536, cm, first_row, s, D) for s in chunks]
    elif P > 1:
        exp = [periodic_ref.encode_ref(c, cum, 65536, cm, first_row, s) for s in chunks]
    else:
        exp = [order1_ref.encode_ref(c, cum, 65536, cm[0], first_row, s) for s in chunks]
    coder_case(name, lambda *a: rc.encode_batch_order1(o1, *a),
               lambda *a: rc.decode_batch_order1(o1, *a), chunks, exp, too_long=too_long)
    o1.close()


@pytest.mark.parametrize("name,P,D", [("order1", 1, 1), ("order1_periodic_p4", 4, 1),
                                      ("order1_lagged_p4_d4", 4, 4)])
def test_order1_sets(ctx, name, P, D):
    order1_case(name, P, D)


# ------------------------------------------------------------------- 5. wide coders
def wide_models():
    """name -> (class, frequencies, encode call, decode call)"""
    w16 = (rc.encode_batch_wide16, rc.decode_batch_wide16)
    return {"wide_1024": (rc.WideStaticModel, zipf(1024, 65536), rc.encode_batch_wide,
                          rc.decode_batch_wide),
            "wide16_65536": (rc.Wide16StaticModel, np.ones(65536, np.int64), *w16),
            "wide16_fine_2p20": (rc.Wide16FineModel, sparse_table(), *w16)}


def wide_case(name, model, too_long=False):
    cls, f, enc, dec = wide_models()[model]
    c, cum, total = wide_ref.table(f)
    m = cls(c, cum, total)
    rng = np.random.default_rng(H.CASES[name]["seed"])
    chunks = [draw(rng, c, int(L), np.uint16) for L in H.case_lens(name)]
    if len(c) == 65536 and c[65535]:
        max(chunks, key=len)[-1] = 65535
    exp = [wide_ref.encode_ref(c, cum, total, s) for s in chunks]
    coder_case(name, lambda *a: enc(m, *a), lambda *a: dec(m, *a), chunks, exp, wide=True,
               too_long=too_long)
    m.close()


@pytest.mark.parametrize("name,model", [("wide_1024", "wide_1024"),
                                        ("wide16_65536", "wide16_65536"),
                                        ("wide16_fine_2p20", "wide16_fine_2p20"),
                                        ("wide16_65536_index", "wide16_65536")])
def test_wide_coders(ctx, name, model):
    wide_case(name, model)


# ------------------------------------------------------------------- 6. chunk sets
def chunk_set_case(name, too_long=False):
    K = 8
    rng = np.random.default_rng(H.CASES[name]["seed"])
    c, cum = indexed_ref.tables(order1_ref.markov_rows(rng, K, 256, 65536))
    cs = rc.ChunkModelSet(c, cum, 65536)
    lens = H.case_lens(name)
    cls = rng.integers(0, K, len(lens) + 1).astype(np.uint8)
    chunks = [draw(rng, c[r], int(L), np.uint8) for r, L in zip(cls, lens)]
    exp = [cpu.encode(c[r], cum[r], 65536, s)[:2] for r, s in zip(cls, chunks)]
    cls_t = dev(cls)
    coder_case(name, lambda *a: rc.api.encode_batch_chunk_set(cs, cls_t, *a),
               lambda *a: rc.api.decode_batch_chunk_set(cs, cls_t, *a), chunks, exp,
               too_long=too_long)
    cs.close()


def test_chunk_set(ctx):
    chunk_set_case("chunk_set_k8")


# ------------------------------------------------------------------- too-long chunks
@pytest.mark.parametrize("name", ["too_long_wide16", "too_long_wide16_fine",
                                  "too_long_chunk_set", "too_long_periodic", "too_long_lagged"])
def test_too_long_chunk_above_the_boundary_is_flagged_untouched(ctx, name):
    """test_gpu_limits.py's check for the families it does not reach, with the flagged chunk
    (its out_len, flag and slot) behind chunks that lie above the boundary."""
    if name == "too_long_wide16":
        wide_case(name, "wide16_65536", too_long=True)
    elif name == "too_long_wide16_fine":
        wide_case(name, "wide16_fine_2p20", too_long=True)
    elif name == "too_long_chunk_set":
        chunk_set_case(name, too_long=True)
    elif name == "too_long_periodic":
        order1_case(name, 4, 1, too_long=True)
    else:
        order1_case(name, 4, 4, too_long=True)


# ------------------------------------------------------------------- 8. model building
def data_arena(name, chunks, dtype):
    """(arena, sym_off tensor, sym_off) of a read-only case: the chunks at the case's layout"""
    t, off = sym_arena(name, "enc", chunks, dtype)
    return t, dev(off), off


def unchanged(name, t, off, chunks, sent):
    assert H.untouched(t, [(off[0], off[-1])], sent) == 0, name
    assert np.array_equal(H.window(t, off[0], off[-1]), np.concatenate(chunks)), name


@pytest.mark.parametrize("name", ["histograms_u8", "histograms_u8_exact"])
def test_histograms_8_bit(ctx, name):
    """rc_histogram (batch and per-chunk rows), rc_histogram_order1, rc_histogram_pairs and its
    periodic and lagged variants: exact against numpy on the chunks around the boundary.  The
    sentinels are symbol 0xEE, so a chunk read from a truncated address counts there."""
    rng = np.random.default_rng(H.CASES[name]["seed"])
    chunks = [rng.integers(0, 200, int(L)).astype(np.uint8) for L in H.case_lens(name)]
    flat = np.concatenate(chunks)
    syms, off_t, off = data_arena(name, chunks, torch.uint8)
    hist, rows = MB.histogram(syms, off_t, per_chunk=True)
    h1, none = MB.histogram(syms, off_t)
    assert none is None
    K = 8
    cm = rng.integers(0, K, 256).astype(np.uint8)
    ho1 = MB.histogram_order1(syms, off_t, cm, 5, n_models=K)
    pair, first = MB.histogram_pairs(syms, off_t)
    pair_p, first_p = MB.histogram_pairs_periodic(syms, off_t, 4)
    pair_l, first_l = MB.histogram_pairs_periodic(syms, off_t, 4, lag=4)
    torch.cuda.synchronize()
    want = np.bincount(flat, minlength=256)
    assert np.array_equal(hist.cpu().numpy(), want) and np.array_equal(h1.cpu().numpy(), want)
    rows = rows.cpu().numpy()
    for k, s in enumerate(chunks):
        assert np.array_equal(rows[k], np.bincount(s, minlength=256)), (name, k, len(s))
    want_o1 = np.zeros((K, 256), np.int64)
    for s in chunks:
        np.add.at(want_o1, (order1_ref.derive_idx(cm, 5, s, 256).astype(np.int64),
                            s.astype(np.int64)), 1)
    assert np.array_equal(ho1.cpu().numpy(), want_o1)
    for (gp, gf), (P, D) in (((pair, first), (1, 1)), ((pair_p, first_p), (4, 1)),
                             ((pair_l, first_l), (4, 4))):
        wp, wf = (periodic_ref.pairs(chunks, P) if D == 1 else lag_ref.pairs(chunks, P, D))
        assert np.array_equal(gp.cpu().numpy().reshape(P, 256, 256), wp), (name, P, D)
        assert np.array_equal(gf.cpu().numpy(), wf), (name, P, D)
    unchanged(name, syms, off, chunks, SENT)
    del syms
    free()


def test_histograms_16_bit(ctx):
    """rc_histogram_wide (n = 1024, with and without per-chunk rows), histogram16 and
    rc_ideal_bits_wide.  The sentinels are symbol 0xEEEE: out of range for the 1024 bins (oob
    counts them), a bin of its own for histogram16, and +inf for the ideal bits."""
    name = "histograms_u16"
    rng = np.random.default_rng(H.CASES[name]["seed"])
    c, cum, total = wide_ref.table(zipf(1024, 65536))
    chunks = [draw(rng, c, int(L), np.uint16) for L in H.case_lens(name)]
    flat = np.concatenate(chunks)
    syms, off_t, off = data_arena(name, chunks, torch.int16)
    hist, rows, oob = MB.histogram_wide(syms, off_t, 1024, per_chunk=True)
    h1, none, oob1 = MB.histogram_wide(syms, off_t, 1024)
    h16 = MB.histogram16(syms, off_t)
    m = rc.WideStaticModel(c, cum, total)
    bits = MB.ideal_bits_wide(m, syms, off_t)
    torch.cuda.synchronize()
    want = np.bincount(flat, minlength=1024)
    assert none is None and int(oob) == 0 and int(oob1) == 0
    assert np.array_equal(hist.cpu().numpy(), want) and np.array_equal(h1.cpu().numpy(), want)
    rows = rows.cpu().numpy()
    for k, s in enumerate(chunks):
        assert np.array_equal(rows[k], np.bincount(s, minlength=1024)), (k, len(s))
    assert np.array_equal(h16.cpu().numpy(), np.bincount(flat, minlength=65536))
    # the tolerance test_gpu_wide_build.py states for chunks of at most 2000 symbols
    np.testing.assert_allclose(bits.cpu().numpy(), wide_build_ref.ideal_bits_ref(chunks, c, total),
                               rtol=1e-12, atol=0)
    unchanged(name, syms, off, chunks, SENT16)
    m.close()
    del syms
    free()


def test_ideal_bits_order1(ctx):
    """rc_ideal_bits_order1 at period 1 and with a period and a lag, within the 1e-12 relative
    that test_gpu_periodic.py and test_gpu_lag.py state, against their f64 reference."""
    name, K = "ideal_bits_order1", 8
    rng = np.random.default_rng(H.CASES[name]["seed"])
    c, cum = indexed_ref.tables(order1_ref.markov_rows(rng, K, 256, 65536, 1.0))
    chunks = [rng.integers(0, 256, int(L)).astype(np.uint8) for L in H.case_lens(name)]
    syms, off_t, off = data_arena(name, chunks, torch.uint8)
    for P, D in ((1, 1), (4, 4)):
        cm = rng.integers(0, K, (P, 256)).astype(np.uint8)
        o1 = rc.Order1ModelSet(c, cum, 65536, ctx_map=cm if P > 1 else cm[0], first_row=1,
                               period=P, lag=D)
        got = MB.ideal_bits_order1(o1, syms, off_t).cpu().numpy()
        want = np.array([lag_ref.ideal_bits(c, 65536, cm, 1, s, D) for s in chunks])
        assert np.isfinite(want).all() and np.isfinite(got).all()
        zero = want == 0
        assert (got[zero] == 0).all()
        err = np.abs(got[~zero] - want[~zero]) / want[~zero]
        print(f"ideal bits order-1, P={P} D={D}: relative error {err.max():.3g}")
        assert err.max() <= 1e-12
        o1.close()
    unchanged(name, syms, off, chunks, SENT)
    del syms
    free()


def rows_launch(n_chunks, n_real, seed, dtype, hi):
    """sym_off of a launch of n_chunks chunks, all empty but the last n_real, over a small
    arena: (arena, sym_off tensor, the real chunks)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 300, n_real)
    lens[:3] = (0, 1, 300)
    chunks = [rng.integers(0, hi, int(L)).astype(np.uint16 if dtype == torch.int16 else np.uint8)
              for L in lens]
    base = 37
    real_off = base + np.concatenate([[0], np.cumsum(lens)])
    off = torch.full((n_chunks + 1,), base, dtype=torch.int64, device="cuda")
    off[n_chunks - n_real:] = torch.from_numpy(real_off).cuda()
    t = H.arena(H.arena_elems(real_off[-1], 2 if dtype == torch.int16 else 1), dtype, SENT)
    H.put(t, base, np.concatenate(chunks))
    return t, off, chunks


def check_rows(rows, chunks, n_chunks, n_real, bins, seed):
    """the real chunks' rows, and the rows of a sample of the empty ones: the first ones (where
    a row offset taken mod 2^32 would put the real chunks' counts), the last before the real
    ones, and random ones"""
    first_real = n_chunks - n_real
    for j, s in enumerate(chunks):
        got = rows[first_real + j].cpu().numpy()
        assert np.array_equal(got, np.bincount(s, minlength=bins)), (j, len(s))
    rng = np.random.default_rng(seed)
    sample = np.concatenate([np.arange(1024), np.arange(first_real - 1024, first_real),
                             rng.integers(1024, first_real - 1024, H.ROWS_SAMPLE - 2048)])
    assert int(rows[torch.from_numpy(sample).cuda()].abs().sum()) == 0


def test_per_chunk_rows_past_4_gib(ctx):
    """rc_histogram's per-chunk rows (1 KiB each) pass byte 2^32 at chunk 2^22: one launch of
    2^22 + 64 chunks, all empty (sym_off repeats one value) but the last 64."""
    n, r = H.ROWS_CHUNKS, H.ROWS_REAL
    syms, off, chunks = rows_launch(n, r, 31, torch.uint8, 256)
    hist, rows = MB.histogram(syms, off, per_chunk=True)
    torch.cuda.synchronize()
    assert rows.shape == (n, 256) and rows.numel() * 4 > H.BOUNDARY
    assert np.array_equal(hist.cpu().numpy(), np.bincount(np.concatenate(chunks), minlength=256))
    check_rows(rows, chunks, n, r, 256, 32)
    del rows, syms, off
    free()


def test_per_chunk_rows_wide_past_4_gib(ctx):
    """rc_histogram_wide's per-chunk rows at n = 1024 (4 KiB each) pass byte 2^32 at chunk
    2^20: one launch of 2^20 + 64 chunks, all empty but the last 64."""
    n, r = (1 << 20) + 64, H.ROWS_REAL
    syms, off, chunks = rows_launch(n, r, 33, torch.int16, 1024)
    hist, rows, oob = MB.histogram_wide(syms, off, 1024, per_chunk=True)
    torch.cuda.synchronize()
    assert rows.shape == (n, 1024) and rows.numel() * 4 > H.BOUNDARY and int(oob) == 0
    assert np.array_equal(hist.cpu().numpy(), np.bincount(np.concatenate(chunks), minlength=1024))
    check_rows(rows, chunks, n, r, 1024, 34)
    del rows, syms, off
    free()


# ------------------------------------------------------------------- 9. checksum_batch
@pytest.mark.parametrize("name", ["checksum_u8", "checksum_u16", "checksum_u16_index"])
def test_checksum_batch(ctx, name):
    """8-bit and 16-bit data; the 16-bit kernel scales the element offset to bytes itself (b *
    sym_bytes), at the placement where the byte offset passes 2^32 and at the one where the
    element index does."""
    wide = name != "checksum_u8"
    rng = np.random.default_rng(H.CASES[name]["seed"])
    chunks = [rng.integers(0, 65536 if wide else 256, int(L)).astype(np.uint16 if wide
                                                                     else np.uint8)
              for L in H.case_lens(name)]
    data, off_t, off = data_arena(name, chunks, torch.int16 if wide else torch.uint8)
    sums = CT.checksum_batch(data, off_t).cpu().numpy().view(np.uint32)
    kind = container2_ref.KIND_WIDE if wide else container2_ref.KIND_STATIC
    want = [container2_ref.checksum(container2_ref.sym_bytes(s, kind)) for s in chunks]
    assert sums.tolist() == want
    unchanged(name, data, off, chunks, SENT16 if wide else SENT)
    del data
    free()


# ------------------------------------------------------------------- 7. resumable streams
def stream_slots(name, lens, off, elem_bytes, boundary):
    """(out_off, caps, short): slots of RC_STREAM_MAX_BYTES and a little more, one of a stream
    above the boundary a byte short of it (RC_F_CAPACITY, nothing changed)"""
    caps = np.array([N.stream_max_bytes(int(L), True) + (0, 5, 16)[k % 3]
                     for k, L in enumerate(lens)], np.int64)
    short = first_above(off, elem_bytes, boundary, lens, need=1)
    caps[short] = N.stream_max_bytes(int(lens[short]), True) - 1
    out_off, caps = H.slot_layout(caps, mode=H.CASES[name]["slots"])
    return out_off, caps, short


def check_stream_encode(name, out, out_off, out_len, flags, states, exp, short):
    """exp: (flags, bytes, final state row) per stream"""
    torch.cuda.synchronize()
    fl, ol = flags.cpu().numpy(), out_len.cpu().numpy()
    st = states.cpu().numpy().view(np.uint64)
    h = H.window(out, out_off[0], out_off[-1])
    rel = out_off - out_off[0]
    for k, (f, b, row) in enumerate(exp):
        if k == short:
            assert (int(fl[k]), int(ol[k])) == (N.F_CAPACITY, 0), (name, k, fl[k], ol[k])
            assert st[k].tolist() == fresh(1)[0].tolist(), (name, k)
            continue
        assert (int(fl[k]), int(ol[k])) == (f, len(b)) and f == 0, (name, k, fl[k], ol[k])
        assert bytes(h[rel[k]:rel[k] + len(b)]) == b, (name, k)
        assert st[k].tolist() == row.tolist(), (name, k)
    assert H.untouched(out, [(out_off[0], out_off[-1])], SENT) == 0, name


def stream_code_arena(name, codes, doff, lens):
    """(code arena, code_off, code_len, cut): the oracle's streams at code_layout's offsets; one
    stream above the boundary cut to 7 bytes (RC_F_TRUNCATED at Decoder::new, state untouched)"""
    code_len = np.array([len(b) for b in codes], np.int64)
    code_off = H.code_layout(code_len, seed=H.CASES[name]["seed"])
    code = H.arena(H.place_elems("u8", int((code_off + code_len).max())), torch.uint8, SENT)
    for k, b in enumerate(codes):
        H.put(code, code_off[k], np.frombuffer(b, np.uint8))
    cut = [k for k in range(len(codes)) if code_off[k] > H.BOUNDARY and lens[k] >= 1][-1]
    code_len[cut] = 7
    return code, code_off, code_len, cut


def check_stream_decode(name, dec_out, doff, flags, states, chunks, rows, cut):
    """rows: the final state row of every stream"""
    torch.cuda.synchronize()
    fd = flags.cpu().numpy()
    st = states.cpu().numpy().view(np.uint64)
    got = H.window(dec_out, doff[0], doff[-1])
    drel = doff - doff[0]
    for k, s in enumerate(chunks):
        if k == cut:
            assert int(fd[k]) == N.F_TRUNCATED, (name, k, fd[k])
            assert (got[drel[k]:drel[k + 1]] == SENT).all(), (name, k)
            continue
        assert int(fd[k]) == 0, (name, k, len(s), fd[k])
        assert np.array_equal(got[drel[k]:drel[k + 1]], s), (name, k, len(s))
        assert st[k].tolist() == rows[k].tolist(), (name, k)
    assert H.untouched(dec_out, [(doff[0], doff[-1])], SENT) == 0, name


def test_stream_batch(ctx):
    """rc_stream_encode with the (c, cum, total) triples at the 12-byte placement (element
    2^32 // 12: byte 2^32 falls inside a triple) and the slots high; rc_stream_decode with the
    code and the decoded symbols high."""
    name = "stream_triples"
    case = H.CASES[name]
    rng = np.random.default_rng(case["seed"])
    c, cum, total = (np.asarray(a, np.uint32) if i < 2 else int(a)
                     for i, a in enumerate(synth.zipf_table()))
    lens = H.case_lens(name)
    n = len(lens)
    chunks = [draw(rng, c, int(L), np.uint8) for L in lens]
    trips = [np.stack([c[s], cum[s], np.full(len(s), total, np.uint32)], axis=1).astype(np.uint32)
             for s in chunks]
    exp = []
    for t in trips:
        st = cpu.Stream.fresh()
        f, b, _ = cpu.stream_encode(st, t, finish=True)
        exp.append((f, b, as_row(st)))
    off = H.case_layout(name, "enc")
    S32 = 0xEEEEEEEE
    tri = H.arena(3 * H.place_elems("triples", off[-1]), torch.int32, S32)
    flat = np.concatenate(trips).reshape(-1)
    H.put(tri, 3 * off[0], flat)
    out_off, caps, short = stream_slots(name, lens, off, 12, H.BOUNDARY)
    out = H.arena(H.place_elems("u8", out_off[-1]), torch.uint8, SENT)
    states = rc.stream_states(n)
    out_len, flags = rc.stream_encode_batch(ctx, states, tri, dev(off), out, dev(out_off),
                                            finish=True)
    check_stream_encode(name, out, out_off, out_len, flags, states, exp, short)
    assert H.untouched(tri, [(3 * off[0], 3 * off[-1])], S32) == 0
    assert np.array_equal(H.window(tri, 3 * off[0], 3 * off[-1]), flat)
    del tri, out
    # decode
    eb, boundary, _ = H.PLACEMENTS["u8"]
    doff = H.layout(lens, eb, boundary, mode=case["dec"])
    dec_out = H.arena(H.place_elems("u8", doff[-1]), torch.uint8, SENT)
    code, code_off, code_len, cut = stream_code_arena(name, [b for _, b, _ in exp], doff, lens)
    rows = []
    for s, (_, b, _) in zip(chunks, exp):
        st = cpu.Stream.fresh()
        f, got = cpu.stream_decode(st, c, cum, total, b, len(s))
        assert f == 0 and np.array_equal(got, s)
        rows.append(as_row(st))
    states = rc.stream_states(n)
    fd = rc.stream_decode_batch(ctx, dev(c.view(np.int32)), dev(cum.view(np.int32)), total, states,
                                code, dev(code_off), dev(code_len), dec_out, dev(doff))
    check_stream_decode(name, dec_out, doff, fd, states, chunks, rows, cut)
    del code, dec_out
    free()


def test_stream_rows(ctx):
    """rc_stream_encode_rows and rc_stream_decode_rows with row_of (4 bytes per symbol) at
    element 2^30, where its byte offset passes 2^32, through the wave-per-stream and the
    lane-per-stream decoder, chosen as test_gpu_rows_lane.py chooses them."""
    name = "stream_rows"
    case = H.CASES[name]
    rng = np.random.default_rng(case["seed"])
    tab = RR.mixed_table(64, 164)
    T = dtab(tab)
    lens = H.case_lens(name)
    n = len(lens)
    rows = [rng.integers(0, RR.N_ROWS, int(L)).astype(np.uint32) for L in lens]
    chunks = [RR.live_symbols(tab[0], r, rng) for r in rows]
    exp = [(f, b, row) for f, b, _, row in (ref_encode(tab, r, s, True)
                                            for r, s in zip(rows, chunks))]
    eb, boundary, _ = H.PLACEMENTS["row_of"]
    S32 = 0xEEEEEEEE

    def arenas(off, with_syms):
        row_of = H.arena(H.place_elems("row_of", off[-1]), torch.int32, S32)
        H.put(row_of, off[0], np.concatenate(rows))
        syms = H.arena(row_of.numel(), torch.uint8, SENT)  # indexed like row_of: 1 GiB
        if with_syms:
            H.put(syms, off[0], np.concatenate(chunks))
        return row_of, syms

    off = H.case_layout(name, "enc")
    row_of, syms = arenas(off, True)
    out_off, caps, short = stream_slots(name, lens, off, 4, boundary)
    out = H.arena(H.place_elems("u8", out_off[-1]), torch.uint8, SENT)
    states = rc.stream_states(n)
    out_len, flags = rc.stream_encode_rows_batch(ctx, *T, row_of, syms, states, dev(off), out,
                                                 dev(out_off), finish=True)
    check_stream_encode(name, out, out_off, out_len, flags, states, exp, short)
    for t, s, flat in ((row_of, S32, np.concatenate(rows)), (syms, SENT, np.concatenate(chunks))):
        assert H.untouched(t, [(off[0], off[-1])], s) == 0
        assert np.array_equal(H.window(t, off[0], off[-1]), flat)
    del row_of, syms, out
    # decode, once per kernel
    doff = H.case_layout(name, "dec")
    row_of, dec_out = arenas(doff, False)
    code, code_off, code_len, cut = stream_code_arena(name, [b for _, b, _ in exp], doff, lens)
    want = [ref_decode(tab, r, b)[2] for r, (_, b, _) in zip(rows, exp)]
    made = []
    try:
        for which in (1, 2):  # wave per stream, lane per stream
            c2 = rc.Context(0)
            made.append(c2)
            assert c2._lib.rc_rows_decoder_(c2.handle, which) == N.RC_OK
            dec_out.fill_(SENT)
            states = rc.stream_states(n)
            fd = rc.stream_decode_rows_batch(c2, *T, row_of, states, code, dev(code_off),
                                             dev(code_len), dec_out, dev(doff))
            check_stream_decode(name, dec_out, doff, fd, states, chunks, want, cut)
    finally:
        torch.cuda.synchronize()
        for c2 in made:
            c2.close()
    assert H.untouched(row_of, [(doff[0], doff[-1])], S32) == 0
    del row_of, dec_out, code
    free()


# ------------------------------------------------------------------- 10. containers
@pytest.mark.parametrize("name", ["container_rcb1", "container_rcb2_checksums"])
def test_container_payload_past_4_gib(ctx, name):
    """pack() from encoder slots above the boundary.  Chunk 0 is a filler: 16 symbols and a
    code_len of 2^32 + 4103 bytes of whatever its slot holds (its own short stream, then
    sentinels), so every later chunk's payload lies past 2^32 inside the container; what chunk
    0 decodes to is not compared."""
    rcb2 = name != "container_rcb1"
    c, cum, total = synth.zipf_table()
    c, cum, total = np.asarray(c, np.uint32), np.asarray(cum, np.uint32), int(total)
    m = rc.StaticModel(c, cum, total)
    rng = np.random.default_rng(H.CASES[name]["seed"])
    lens = np.concatenate([[16], H.case_lens(name)])
    n = len(lens)
    chunks = [draw(rng, c, int(L), np.uint8) for L in lens]
    exp = [cpu.encode(c, cum, total, s)[:2] for s in chunks]
    assert all(f == 0 for f, _ in exp)
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    syms = dev(np.concatenate(chunks + [np.zeros(16, np.uint8)]))
    caps = [len(b) + (0, 5, 16)[k % 3] for k, (_, b) in enumerate(exp)]
    slot_off = H.filler_layout(caps)
    slots = H.arena(H.arena_elems(slot_off[-1], 1), torch.uint8, SENT)
    out_len, flags = rc.encode_batch(m, syms, dev(sym_off), slots, dev(slot_off))
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0
    code_len = out_len.cpu().numpy().astype(np.int64)
    assert code_len.tolist() == [len(b) for _, b in exp]
    code_len[0] = H.FILLER_BYTES
    sums = CT.checksum_batch(syms, dev(sym_off)) if rcb2 else None
    blob = CT.pack(m, slots, dev(slot_off), dev(code_len), dev(sym_off), sums=sums, rcb2=rcb2)
    assert H.untouched(slots, [(slot_off[0], slot_off[-1])], SENT) == 0
    del slots
    free()
    inf = CT.info(blob)
    assert isinstance(inf, N.Container2Info) == rcb2
    padded = (code_len + 15) // 16 * 16
    assert inf.payload_bytes == int(padded.sum()) and inf.n_chunks == n
    assert inf.container_bytes == inf.payload_off + int(padded.sum()) == blob.numel()
    want_off = inf.payload_off + np.concatenate([[0], np.cumsum(padded)[:-1]])
    assert (want_off[1:] > H.BOUNDARY).all()
    code_off, clen, soff = CT.offsets(blob, inf)
    assert code_off.cpu().numpy().tolist() == want_off.tolist()
    assert clen.cpu().numpy().tolist() == code_len.tolist()
    assert soff.cpu().numpy().tolist() == sym_off.tolist()
    for k in range(1, n):  # the streams, and their zero padding to 16 bytes
        got = H.window(blob, want_off[k], want_off[k] + padded[k])
        assert bytes(got[:code_len[k]]) == exp[k][1], (name, k)
        assert not got[code_len[k]:].any(), (name, k)
    head = H.window(blob, want_off[0], want_off[0] + 4096)
    assert bytes(head[:len(exp[0][1])]) == exp[0][1] and (head[2048:] == SENT).all()
    if rcb2:
        stored = H.window(blob, inf.sum_off, inf.sum_off + 4 * n).view(np.uint32)
        assert stored.tolist() == [container2_ref.checksum(s.tobytes()) for s in chunks]
    dec = torch.full((int(sym_off[-1]) + 16,), SENT, dtype=torch.uint8, device="cuda")
    fd = rc.decode_batch(m, blob, code_off[1:], clen[1:], dec, soff[1:])
    torch.cuda.synchronize()
    assert int(fd.abs().sum()) == 0
    d = dec.cpu().numpy()
    assert np.array_equal(d[16:sym_off[-1]], np.concatenate(chunks[1:]))
    assert (d[:16] == SENT).all() and (d[sym_off[-1]:] == SENT).all()
    m.close()
    del blob, dec
    free()


# ------------------------------------------------------------------- coverage
# Every public call of rc.api, rc.model_build and rc.container that takes a sym_off: the test
# here that runs it on a high arena, or the reason it runs on none.
COVERED = {
    "api.encode_batch": "test_static_coders, test_adaptive_coders",
    "api.decode_batch": "test_static_coders, test_adaptive_coders",
    "api.encode_batch_indexed": "test_indexed_set",
    "api.decode_batch_indexed": "test_indexed_set",
    "api.encode_batch_order1": "test_order1_sets",
    "api.decode_batch_order1": "test_order1_sets",
    "api.encode_batch_wide": "test_wide_coders",
    "api.decode_batch_wide": "test_wide_coders",
    "api.encode_batch_wide16": "test_wide_coders",
    "api.decode_batch_wide16": "test_wide_coders",
    "api.encode_batch_chunk_set": "test_chunk_set",
    "api.decode_batch_chunk_set": "test_chunk_set",
    "api.stream_encode_batch": "test_stream_batch",
    "api.stream_decode_batch": "test_stream_batch",
    "api.stream_encode_rows_batch": "test_stream_rows",
    "api.stream_decode_rows_batch": "test_stream_rows",
    "model_build.histogram": "test_histograms_8_bit, test_per_chunk_rows_past_4_gib",
    "model_build.histogram_order1": "test_histograms_8_bit",
    "model_build.histogram_pairs": "test_histograms_8_bit",
    "model_build.histogram_pairs_periodic": "test_histograms_8_bit",
    "model_build.histogram_wide": "test_histograms_16_bit, test_per_chunk_rows_wide_past_4_gib",
    "model_build.histogram16": "test_histograms_16_bit",
    "model_build.ideal_bits_wide": "test_histograms_16_bit",
    "model_build.ideal_bits_order1": "test_ideal_bits_order1",
    "container.checksum_batch": "test_checksum_batch",
    "container.pack": "test_container_payload_past_4_gib",
}
HOST = "host-resident arrays: 4 GiB of host memory and its PCIe time do not fit a test"
EXCLUDED = {
    "api.encode_host": HOST,
    "api.decode_host": HOST,
    "api.encode_host_multi": HOST + "; several devices",
    "api.decode_host_multi": HOST + "; several devices",
    "model_build.build_model": "histogram (covered), then the table is made on the host",
    "model_build.build_order1_set": "histogram_order1 or histogram_pairs_periodic (covered), "
                                    "then the rows are made on the host",
    "model_build.fit_order1_set": "histogram_pairs, histogram_pairs_periodic and "
                                  "histogram_order1 (covered); the clustering takes no offsets",
    "model_build.build_wide_model": "histogram_wide (covered), then the table is made on the host",
    "model_build.build_wide16_model": "histogram16 (covered), then the table is made on the host",
    "model_build.fit_chunk_set": "histogram with per-chunk rows (covered); the costs and the "
                                 "sums by class take rows, no offsets",
    "container.verify": "checksum_batch's kernel with an expected sum per chunk; its offsets "
                        "are taken the same way (covered there)",
}


def test_every_call_with_offsets_has_a_case():
    """A family added later fails here until it has a high-offset case, or a written reason."""
    found = set()
    for mod in (rc.api, MB, CT):
        short = mod.__name__.rsplit(".", 1)[1]
        for fname, fn in vars(mod).items():
            if fname.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != mod.__name__:
                continue
            if "sym_off" in inspect.signature(fn).parameters:
                found.add(f"{short}.{fname}")
    assert not set(COVERED) & set(EXCLUDED)
    assert found == set(COVERED) | set(EXCLUDED), (sorted(found - set(COVERED) - set(EXCLUDED)),
                                                   sorted((set(COVERED) | set(EXCLUDED)) - found))
    here = globals()
    for tests in COVERED.values():
        for t in tests.split(", "):
            assert callable(here.get(t)), t
    assert all(len(r) > 20 for r in EXCLUDED.values())
