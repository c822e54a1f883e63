"""The indexed batch coders (rc_encode_batch_indexed / rc_decode_batch_indexed: a static model
set and one model index per symbol) through the C ABI, against the CPU oracle (indexed_ref.py)
and against the single-table coders: ragged and misaligned arenas, sentinel bytes around the
slots, every set shape, the rare paths, flags, bad streams, the kind checks and the C++ example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N, synth  # noqa: E402
from gpu_helpers import dev  # noqa: E402
from indexed_ref import decode_ref, encode_ref, tables  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xEE


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


# ---------------------------------------------------------------- arenas through the C ABI
def _shifted(t, off):
    """A tensor holding t's values whose first byte sits `off` bytes past a 256-B aligned
    allocation (torch allocations are at least 256-B aligned)."""
    big = torch.full((t.numel() + off + 64,), SENT, dtype=torch.uint8, device="cuda")
    v = big[off:off + t.numel()]
    v.copy_(t)
    return v, big


def run_encode(mset, chunks, caps, misalign=False, seed=0):
    """chunks: (symbols, indexes) pairs at contiguous ragged offsets.  misalign: symbols,
    indexes and slots start at independent random byte offsets (so idx is in general not
    congruent to syms mod 16); otherwise every base is 16-B aligned."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(s) for s, _ in chunks], np.int64)
    pre = int(rng.integers(0, 16)) if misalign else 0
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + pre
    cat = lambda j: np.concatenate([rng.integers(0, 256, pre).astype(np.uint8)] +  # noqa: E731
                                   [np.asarray(c[j], np.uint8) for c in chunks] +
                                   [np.zeros(1, np.uint8)])
    bs, bi, bo = (int(x) for x in rng.integers(0, 16, 3)) if misalign else (0, 0, 0)
    syms, _ks = _shifted(dev(cat(0)), bs)
    idx, _ki = _shifted(dev(cat(1)), bi)
    caps = np.asarray(caps, np.int64)
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + bo
    out = torch.full((int(out_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = rc.encode_batch_indexed(mset, syms, idx, dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    # nothing is written outside the slots (bytes past out_len inside a slot are unspecified)
    assert (h[:bo] == SENT).all() and (h[out_off[-1]:] == SENT).all()
    return h, out_off, out_len.cpu().numpy(), flags.cpu().numpy()


def run_decode(mset, codes, idxs, misalign=False, seed=0):
    """codes at random gaps, indexes and decoded symbols at independent random byte offsets."""
    rng = np.random.default_rng(seed)
    n = len(codes)
    clen = np.array([len(c) for c in codes], np.int64)
    gaps = rng.integers(0, 16, n) if misalign else (-clen) % 16
    coff = np.zeros(n, np.int64)
    parts, pos = [], 0
    for k, c in enumerate(codes):
        parts.append(np.frombuffer(bytes(c), np.uint8))
        coff[k] = pos
        pos += len(c)
        parts.append(rng.integers(0, 256, int(gaps[k])).astype(np.uint8))
        pos += int(gaps[k])
    parts.append(np.zeros(16, np.uint8))
    counts = np.array([len(x) for x in idxs], np.int64)
    pre = int(rng.integers(0, 16)) if misalign else 0
    sym_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) + pre
    icat = np.concatenate([rng.integers(0, 256, pre).astype(np.uint8)] +
                          [np.asarray(x, np.uint8) for x in idxs] + [np.zeros(1, np.uint8)])
    bc, bi, bs = (int(x) for x in rng.integers(0, 16, 3)) if misalign else (0, 0, 0)
    code, _kc = _shifted(dev(np.concatenate(parts)), bc)
    idx, _ki = _shifted(dev(icat), bi)
    big = torch.full((int(sym_off[-1]) + bs + 64,), SENT, dtype=torch.uint8, device="cuda")
    syms = big[bs:bs + len(icat)]  # (as long as the index tensor, which the wrapper requires)
    flags = rc.decode_batch_indexed(mset, code, dev(coff), dev(clen), idx, syms, dev(sym_off))
    torch.cuda.synchronize()
    s = syms.cpu().numpy()
    b = big.cpu().numpy()
    # nothing is written outside the chunks' symbol ranges
    assert (b[:bs + sym_off[0]] == SENT).all() and (b[bs + sym_off[-1]:] == SENT).all()
    return [s[sym_off[k]:sym_off[k + 1]] for k in range(n)], flags.cpu().numpy()


def check_round_trip(mset, c, cum, total, chunks, misalign, seed, slack=64):
    """Encode and decode `chunks`; bytes, lengths and flags equal the oracle's, and decode
    returns the symbols."""
    bits = mset.max_bits_per_symbol() + 1
    caps = [rc.slot_capacity(len(s), bits) + slack for s, _ in chunks]
    h, out_off, ol, fl = run_encode(mset, chunks, caps, misalign, seed)
    codes = []
    for k, (s, x) in enumerate(chunks):
        f, b = encode_ref(c, cum, total, s, x)
        assert (int(fl[k]), int(ol[k])) == (f, len(b)), (k, len(s), fl[k], ol[k], f, len(b))
        assert bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, (k, len(s))
        codes.append(b)
    dec, fd = run_decode(mset, codes, [x for _, x in chunks], misalign, seed + 1)
    for k, (s, _) in enumerate(chunks):
        assert fd[k] == 0 and np.array_equal(dec[k], np.asarray(s, np.uint8)), (k, len(s))
    return codes


def draw(rng, c, L, idx=None):
    """L symbols, each from the row its (independently drawn) index picks."""
    K, n = c.shape
    idx = rng.integers(0, K, L).astype(np.uint8) if idx is None else idx
    s = np.zeros(L, np.uint8)
    for j in range(K):
        w = np.flatnonzero(idx == j)
        if len(w):
            s[w] = rng.choice(n, len(w), p=c[j] / c[j].sum())
    return s, idx


# ---------------------------------------------------------------- 1. parity
def parity_rows():
    """K = 8, 256 symbols, total 65536: shifted Zipf tables, one row with a block of
    zero-frequency symbols (never drawn: their probability is 0), one spike."""
    zc, _, zt = synth.zipf_table()
    assert zt == 65536 and len(zc) == 256
    rows = [np.roll(np.asarray(zc, np.int64), 32 * j) for j in range(8)]
    z = rows[6]
    big = int(np.argmax(z))
    blk = [i for i in range(100, 140) if i != big]
    z[big] += int(z[blk].sum())
    z[blk] = 0
    spike = np.ones(256, np.int64)
    spike[17] = 65536 - 255
    rows[7] = spike
    return tables(rows)


@pytest.fixture(scope="module")
def parity_set(ctx):
    c, cum = parity_rows()
    return rc.StaticModelSet(c, cum, 65536), c, cum


@pytest.mark.parametrize("misalign", [False, True])
def test_parity_with_the_oracle(parity_set, misalign):
    mset, c, cum = parity_set
    rng = np.random.default_rng(11 + misalign)
    lens = [0, 1, 7, 63, 64, 65, 127, 640, 4099]
    # 200 chunks: one partly filled workgroup, three full waves and a ragged one (more than one
    # workgroup: test_many_short_chunks_fill_several_workgroups)
    chunks = [draw(rng, c, lens[k % len(lens)]) for k in range(200)]
    check_round_trip(mset, c, cum, 65536, chunks, misalign, seed=100 + misalign)


def test_many_short_chunks_fill_several_workgroups(ctx):
    """K = 64: 1,700 short chunks are more than any plan's workgroup holds (a launch this small
    runs 256-lane workgroups so that more CUs take part: seven of them, the last partly filled),
    all checked against the oracle.  Full-size workgroups: the 2^18-chunk case of
    test_one_table_sets_match_the_static_coders."""
    rng = np.random.default_rng(64)
    n, total = 256, 65536
    rows = np.ones((64, n), np.int64)
    for j in range(64):
        w = rng.pareto(1.2, n) + 0.01
        rows[j] += rng.multinomial(total - n, w / w.sum())
    c, cum = tables(rows)
    mset = rc.StaticModelSet(c, cum, total)
    plan = (ctypes.c_uint32 * 8)()
    assert N.load().rc_model_set_plan_(64, total, plan) == N.RC_OK
    assert 1700 > 3 * plan[0] and 1700 > 2 * plan[4]  # (encoder / decoder lanes per workgroup)
    cuts = np.cumsum(rng.integers(0, 81, 1700))[:-1]
    s, x = draw(rng, c, int(cuts[-1]) + 40)
    chunks = list(zip(np.split(s, cuts), np.split(x, cuts)))
    check_round_trip(mset, c, cum, total, chunks, misalign=True, seed=640)


# ---------------------------------------------------------------- 2. shapes of the set
@pytest.mark.parametrize("total", [256, 257, 40000, 65535])
@pytest.mark.parametrize("K", [1, 64])
def test_set_shapes(ctx, K, total):
    rng = np.random.default_rng(K * 100003 + total)
    n = 100
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        w = rng.pareto(1.0, n) + 0.01
        rows[j] += rng.multinomial(total - n, w / w.sum())
    c, cum = tables(rows)
    mset = rc.StaticModelSet(c, cum, total)
    lens = [int(x) for x in rng.integers(0, 2001, 18)] + [0, 2000]
    chunks = [draw(rng, c, L) for L in lens]
    check_round_trip(mset, c, cum, total, chunks, misalign=bool(K == 64), seed=total)


# ---------------------------------------------------------------- 3. the existing coders
@pytest.mark.parametrize("n,L", [(4096, 4096), (1 << 18, 64)])
def test_one_table_sets_match_the_static_coders(ctx, n, L):
    """No oracle: a K = 1 set, and a K = 16 set whose rows are all that table (random
    indexes), produce the slots, lengths and flags of rc_encode_batch on the StaticModel of the
    row, and decode back.  4,096 chunks of 4 KiB are sixteen 256-lane workgroups; 2^18 chunks of
    64 symbols give every CU a workgroup of the plan's full size (1,024 and 768 lanes)."""
    c, cum, total = synth.zipf_table()
    m = rc.StaticModel(c, cum, total)
    syms = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    synth.fill(ctx, 0x1D5EED, synth.inverse_cdf(c), syms, L, n)
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    cap = rc.slot_capacity(L, 8.0)
    out_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap
    want = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    want_len, want_fl = rc.encode_batch(m, syms, sym_off, want, out_off)
    torch.cuda.synchronize()
    assert int(want_fl.abs().sum()) == 0
    valid = torch.arange(cap, device="cuda")[None, :] < want_len[:, None]
    g = torch.Generator(device="cuda").manual_seed(5)
    for K in (1, 16):
        mset = rc.StaticModelSet(np.tile(np.asarray(c, np.uint32), (K, 1)), None, total)
        idx = torch.randint(0, K, (n * L,), dtype=torch.uint8, device="cuda", generator=g)
        out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        out_len, fl = rc.encode_batch_indexed(mset, syms, idx, sym_off, out, out_off)
        torch.cuda.synchronize()
        assert torch.equal(out_len, want_len) and torch.equal(fl, want_fl), K
        assert torch.equal(out.view(n, cap) * valid, want.view(n, cap) * valid), K
        dec = torch.zeros_like(syms)
        fd = rc.decode_batch_indexed(mset, out, out_off[:-1].contiguous(), out_len, idx, dec,
                                     sym_off)
        torch.cuda.synchronize()
        assert int(fd.abs().sum()) == 0 and torch.equal(dec, syms), K


# ---------------------------------------------------------------- 4. rare path
@pytest.mark.parametrize("misalign", [False, True])
def test_rare_heavy_rows(ctx, misalign):
    """Alternating between a row whose coded symbols are nearly all c = 1 of 65536 (2-3 bytes
    settle per symbol and range_reduction_expansion runs often) and a spike row."""
    total = 65536
    a = np.ones(256, np.int64)
    a[0] = 2000
    a[1] = total - 2000 - 254
    b = np.ones(256, np.int64)
    b[200] = total - 255
    c, cum = tables([a, b])
    mset = rc.StaticModelSet(c, cum, total)
    rng = np.random.default_rng(40 + misalign)
    chunks = []
    for L in [64, 640, 4096, 4099, 1000, 127, 0]:
        idx = (np.arange(L) & 1).astype(np.uint8)
        s = rng.integers(2, 256, L)
        s[rng.random(L) < 0.05] = 0
        spike = (idx == 1) & (rng.random(L) < 0.7)
        s[spike] = 200
        chunks.append((s.astype(np.uint8), idx))
    check_round_trip(mset, c, cum, total, chunks, misalign, seed=400 + misalign)


# ---------------------------------------------------------------- 5. flags
def _flag_set():
    rng = np.random.default_rng(77)
    n, K, total = 200, 4, 40000
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        rows[j] += rng.multinomial(total - n, np.ones(n) / n)
    rows[2, 0] += rows[2, 50]
    rows[2, 50] = 0  # the zero-frequency symbol of row 2
    return tables(rows), total


def test_encode_flags(ctx):
    (c, cum), total = _flag_set()
    K, n = c.shape
    mset = rc.StaticModelSet(c, cum, total)
    rng = np.random.default_rng(78)
    chunks = []
    for k in range(70):  # chunks 0..63 share a wave
        idx = rng.integers(0, K, 300).astype(np.uint8)
        s, idx = draw(rng, c, 300, idx)
        chunks.append([s, idx])

    def put(k, pos, sym=None, row=None):
        if row is not None:
            chunks[k][1][pos] = row
        if sym is not None:
            chunks[k][0][pos] = sym

    put(3, 100, sym=50, row=2)              # ZERO_FREQ
    put(10, 200, sym=n)                     # BAD_SYMBOL (symbol >= n_symbols)
    put(11, 0, sym=255)
    put(20, 150, row=K)                     # BAD_MODEL (index >= K)
    put(21, 299, row=255)
    put(30, 50, sym=50, row=2)              # the first error wins, whatever its kind
    put(30, 200, row=K)
    put(31, 50, row=K + 3)
    put(31, 200, sym=n + 1)
    put(32, 7, sym=n)
    put(32, 8, sym=50, row=2)
    put(33, 120, sym=n, row=K)              # at one symbol the model is looked up first
    exp = [encode_ref(c, cum, total, s, x) for s, x in chunks]
    assert [exp[k][0] for k in (3, 10, 11, 20, 21, 30, 31, 32, 33)] == [
        N.F_ZERO_FREQ, N.F_BAD_SYMBOL, N.F_BAD_SYMBOL, N.F_BAD_MODEL, N.F_BAD_MODEL,
        N.F_ZERO_FREQ, N.F_BAD_MODEL, N.F_BAD_SYMBOL, N.F_BAD_MODEL]
    caps = [rc.slot_capacity(300, 16.0)] * 70
    caps[40] = len(exp[40][1]) - 1          # a slot one byte short
    for mis in (False, True):
        h, out_off, ol, fl = run_encode(mset, chunks, caps, mis, seed=5 + mis)
        for k, (f, b) in enumerate(exp):
            if k == 40:
                assert (int(fl[k]), int(ol[k])) == (N.F_CAPACITY, len(b))  # the exact length
                continue
            assert int(fl[k]) == f, (k, fl[k], f)
            if f == 0:  # the neighbours of the flagged chunks stay clean and bit-exact
                assert int(ol[k]) == len(b) and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, k


def test_decode_flags(ctx):
    (c, cum), total = _flag_set()
    K, n = c.shape
    mset = rc.StaticModelSet(c, cum, total)
    rng = np.random.default_rng(79)
    chunks = [draw(rng, c, 300) for _ in range(70)]
    codes = [encode_ref(c, cum, total, s, x)[1] for s, x in chunks]
    idxs = [x.copy() for _, x in chunks]
    idxs[5][299] = K                        # BAD_MODEL at the last symbol,
    idxs[6][0] = 255                        # at the first,
    idxs[7][123] = K + 1                    # and inside a 16-symbol phase
    codes[8] = codes[8][:40]                # an earlier error of another kind wins
    idxs[8][250] = K
    idxs[9][10] = K                         # and a later one does not
    codes[9] = codes[9][:len(codes[9]) - 3]
    exp = [decode_ref(c, cum, total, codes[k], idxs[k]) for k in range(70)]
    assert [exp[k][0] for k in (5, 6, 7, 8, 9)] == [N.F_BAD_MODEL] * 3 + [N.F_TRUNCATED,
                                                                           N.F_BAD_MODEL]
    for mis in (False, True):
        dec, fd = run_decode(mset, codes, idxs, mis, seed=9 + mis)
        for k, (f, s) in enumerate(exp):
            assert int(fd[k]) == f, (k, fd[k], f)
            if f == 0:
                assert np.array_equal(dec[k], chunks[k][0]), k


def test_too_long_chunk_is_flagged_untouched(parity_set):
    mset, c, cum = parity_set
    MAX = N.MAX_CHUNK_SYMBOLS
    rng = np.random.default_rng(7)
    s, x = draw(rng, c, 300)
    # chunk 2 claims MAX + 1 symbols starting inside 300-byte symbol and index buffers
    sym_off = np.array([0, 100, 200, 200 + MAX + 1], np.int64)
    cap = 2048
    out_off = np.arange(4, dtype=np.int64) * cap
    out = torch.full((3 * cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = rc.encode_batch_indexed(mset, dev(s), dev(x), dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    fl, ol, h = flags.cpu().numpy(), out_len.cpu().numpy(), out.cpu().numpy()
    assert fl.tolist() == [0, 0, N.F_TOO_LONG] and ol[2] == 0
    assert (h[2 * cap:] == SENT).all()  # the flagged slot and everything after it untouched
    for k in range(2):
        f, b = encode_ref(c, cum, 65536, s[sym_off[k]:sym_off[k + 1]], x[sym_off[k]:sym_off[k + 1]])
        assert f == 0 and len(b) == ol[k] and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b
    code_len = ol.astype(np.int64).copy()
    code_len[2] = 64
    dec = torch.full((300 + 64,), SENT, dtype=torch.uint8, device="cuda")
    xpad = np.concatenate([x, np.zeros(64, np.uint8)])
    fd = rc.decode_batch_indexed(mset, out, dev(out_off[:3].copy()), dev(code_len), dev(xpad),
                                 dec, dev(sym_off))
    torch.cuda.synchronize()
    d = dec.cpu().numpy()
    assert fd.cpu().numpy().tolist() == [0, 0, N.F_TOO_LONG]
    assert np.array_equal(d[:200], s[:200]) and (d[200:] == SENT).all()


# ---------------------------------------------------------------- 6. bad streams
def test_bad_streams(parity_set):
    """Garbage and truncated streams decoded with random indexes: flags equal the oracle's and,
    where the flag is 0, so do the symbols."""
    mset, c, cum = parity_set
    rng = np.random.default_rng(60)
    codes, idxs = [], []
    for k in range(64):
        codes.append(rng.integers(0, 256, int(rng.integers(8, 401))).astype(np.uint8).tobytes())
        idxs.append(rng.integers(0, 8, 300).astype(np.uint8))
    for cut in range(1, 9):
        s, x = draw(rng, c, 300)
        f, b = encode_ref(c, cum, 65536, s, x)
        assert f == 0
        codes.append(b[:len(b) - cut])
        idxs.append(x)
    exp = [decode_ref(c, cum, 65536, codes[k], idxs[k]) for k in range(len(codes))]
    assert any(f for f, _ in exp)
    for mis in (False, True):
        dec, fd = run_decode(mset, codes, idxs, mis, seed=61 + mis)
        for k, (f, s) in enumerate(exp):
            assert int(fd[k]) == f, (k, len(codes[k]), fd[k], f)
            if f == 0:
                assert np.array_equal(dec[k], s), k


# ---------------------------------------------------------------- 7. kinds do not mix
def test_kinds_do_not_mix(ctx, parity_set):
    mset, c, cum = parity_set
    lib = ctx._lib
    m = rc.StaticModel(c[0], cum[0], 65536)
    am = rc.AdaptiveModel(256, **rc.ADAPTIVE_DEFAULTS)
    syms = torch.zeros(256, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(256, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 128, 256], dtype=torch.int64, device="cuda")
    out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    out_off = torch.tensor([0, 2048, 4096], dtype=torch.int64, device="cuda")
    ol = torch.zeros(2, dtype=torch.int64, device="cuda")
    fl = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    h = mset.handle
    assert lib.rc_encode_batch(ctx.handle, h, p(syms), p(off), 2, p(out), p(out_off), p(ol),
                               p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch(ctx.handle, h, p(out), p(out_off), p(ol), p(syms), p(off), 2,
                               p(fl)) == N.RC_E_ARG
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    n_out = ctypes.c_uint64()
    assert lib.rc_container_pack(ctx.handle, h, p(out), p(out_off), p(ol), p(off), 2, p(dst),
                                 8192, ctypes.byref(n_out)) == N.RC_E_ARG
    hs = np.zeros(256, np.uint8)
    ho = np.array([0, 128, 256], np.uint64)
    with pytest.raises(N.RCError) as e:
        rc.encode_host(mset, hs, ho, np.array([0, 2048, 4096], np.uint64))
    assert e.value.code == N.RC_E_ARG
    with pytest.raises(N.RCError) as e:
        rc.encode_host_multi([mset], hs, ho, np.array([0, 2048, 4096], np.uint64))
    assert e.value.code == N.RC_E_ARG
    for other in (m, am):
        assert lib.rc_encode_batch_indexed(ctx.handle, other.handle, p(syms), p(idx), p(off), 2,
                                           p(out), p(out_off), p(ol), p(fl)) == N.RC_E_ARG
        assert lib.rc_decode_batch_indexed(ctx.handle, other.handle, p(out), p(out_off), p(ol),
                                           p(idx), p(syms), p(off), 2, p(fl)) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()  # nothing was launched


# ---------------------------------------------------------------- the Python mirror
def test_chunk_helpers_round_trip_and_raise(parity_set):
    mset, c, cum = parity_set
    rng = np.random.default_rng(90)
    chunks = [draw(rng, c, L) for L in (0, 5, 1000, 64)]
    codes = rc.encode_chunks_indexed(mset, chunks)
    for (s, x), b in zip(chunks, codes):
        assert encode_ref(c, cum, 65536, s, x) == (0, b)
    back = rc.decode_chunks_indexed(mset, [(b, x) for b, (_, x) in zip(codes, chunks)])
    for (s, _), d in zip(chunks, back):
        assert np.array_equal(s, d)
    s, x = draw(rng, c, 100)
    x[40] = 8
    with pytest.raises(rc.BadModelError):
        rc.encode_chunks_indexed(mset, [(s, x)])
    x1000 = chunks[2][1].copy()
    x1000[40] = 8
    with pytest.raises(rc.BadModelError):
        rc.decode_chunks_indexed(mset, [(codes[2], x1000)])
    s2, x2 = draw(rng, c, 100, np.full(100, 6, np.uint8))
    s2[3] = 120  # a zero-frequency symbol of row 6
    with pytest.raises(rc.ZeroFrequencyError):
        rc.encode_chunks_indexed(mset, [(s2, x2)])
    with pytest.raises(rc.TruncatedStreamError):
        rc.decode_chunks_indexed(mset, [(codes[2][:20], chunks[2][1])])
    with pytest.raises(ValueError):
        rc.encode_chunks_indexed(mset, [(s, x[:50])])


# ---------------------------------------------------------------- 8. the C++ example
def test_cpp_model_set_impl(ctx):
    """examples/model_set_impl: two FreqTables alternating per symbol through rc::ModelSet,
    against the per-call rc::Encoder / rc::Decoder given the same tables."""
    exe = os.path.join(ROOT, "examples", "model_set_impl")
    assert os.path.exists(exe), "examples/model_set_impl not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test passed" in r.stdout
