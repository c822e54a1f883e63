"""The wide batch coders (rc_encode_batch_wide / rc_decode_batch_wide: 16-bit symbols against
one static table of up to 4096 symbols) through the C ABI, byte-exact against the CPU oracles
(wide_ref.py) and against the single-table coders: ragged arenas at aligned and odd symbol
offsets, guard bytes around the slots and the decoded symbols, every table shape, several
workgroups, flags, bad streams, the kind checks, the Python helpers and the C++ example."""
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
from wide_ref import decode_ref, encode_ref, literal_table, table  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xEE
SENT16 = np.uint16(0xEEEE).view(np.int16)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


# ---------------------------------------------------------------- arenas through the C ABI
def _sym_arena(values, shift):
    """An int16 tensor holding the uint16 `values`, its first symbol `shift` symbols past a
    256-B aligned allocation (odd shift: 2-B aligned only), guard symbols on both sides."""
    v = np.ascontiguousarray(values, np.uint16).view(np.int16)
    big = torch.full((len(v) + shift + 64,), int(SENT16), dtype=torch.int16, device="cuda")
    view = big[shift:shift + len(v)]
    view.copy_(dev(v))
    return view, big


def run_encode(model, chunks, caps, shift=0, seed=0):
    """chunks: uint16 arrays at contiguous ragged offsets.  shift: symbols between an aligned
    base and the first symbol; with a shift the slots start at a random byte offset too."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(s) for s in chunks], np.int64)
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cat = np.concatenate([np.asarray(s, np.uint16) for s in chunks] + [np.zeros(1, np.uint16)])
    syms, _keep = _sym_arena(cat, shift)
    bo = int(rng.integers(1, 16)) if shift else 0
    caps = np.asarray(caps, np.int64)
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + bo
    out = torch.full((int(out_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = rc.encode_batch_wide(model, syms, dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    # nothing is written outside the slots (bytes past out_len inside a slot are unspecified)
    assert (h[:bo] == SENT).all() and (h[out_off[-1]:] == SENT).all()
    return h, out_off, out_len.cpu().numpy(), flags.cpu().numpy()


def run_decode(model, codes, counts, shift=0, seed=0):
    """codes at random gaps (with a shift) and decoded symbols `shift` symbols past an aligned
    base, after `shift` guard symbols that belong to no chunk."""
    rng = np.random.default_rng(seed)
    n = len(codes)
    clen = np.array([len(c) for c in codes], np.int64)
    gaps = rng.integers(0, 16, n) if shift else (-clen) % 16
    coff = np.zeros(n, np.int64)
    parts, pos = [], int(rng.integers(0, 16)) if shift else 0
    parts.append(rng.integers(0, 256, pos).astype(np.uint8))
    for k, c in enumerate(codes):
        parts.append(np.frombuffer(bytes(c), np.uint8))
        coff[k] = pos
        pos += len(c)
        parts.append(rng.integers(0, 256, int(gaps[k])).astype(np.uint8))
        pos += int(gaps[k])
    parts.append(np.zeros(16, np.uint8))
    counts = np.asarray(counts, np.int64)
    sym_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) + shift
    big = torch.full((int(sym_off[-1]) + shift + 64,), int(SENT16), dtype=torch.int16,
                     device="cuda")
    syms = big[shift:]
    flags = rc.decode_batch_wide(model, dev(np.concatenate(parts)), dev(coff), dev(clen), syms,
                                 dev(sym_off))
    torch.cuda.synchronize()
    s = syms.cpu().numpy().view(np.uint16)
    b = big.cpu().numpy()
    # nothing is written outside the chunks' symbol ranges
    assert (b[:shift + sym_off[0]] == SENT16).all() and (b[shift + sym_off[-1]:] == SENT16).all()
    return [s[sym_off[k]:sym_off[k + 1]] for k in range(n)], flags.cpu().numpy()


def check_round_trip(model, c, cum, total, chunks, shift, seed, slack=64):
    """Encode and decode `chunks`; bytes, lengths and flags equal the oracle's, and the GPU
    decoder returns the symbols from those bytes."""
    bits = model.max_bits_per_symbol() + 1
    caps = [rc.slot_capacity(len(s), bits) + slack for s in chunks]
    h, out_off, ol, fl = run_encode(model, chunks, caps, shift, seed)
    codes = []
    for k, s in enumerate(chunks):
        f, b = encode_ref(c, cum, total, s)
        assert (int(fl[k]), int(ol[k])) == (f, len(b)), (k, len(s), fl[k], ol[k], f, len(b))
        assert bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, (k, len(s))
        codes.append(b)
    dec, fd = run_decode(model, codes, [len(s) for s in chunks], shift, seed + 1)
    for k, s in enumerate(chunks):
        assert fd[k] == 0 and np.array_equal(dec[k], np.asarray(s, np.uint16)), (k, len(s))
    return codes


def draw(rng, c, L):
    p = np.asarray(c, np.float64)
    return rng.choice(len(c), size=L, p=p / p.sum()).astype(np.uint16)


def spread(rng, live, total):
    """`live` frequencies >= 1 summing to total, unevenly."""
    w = rng.random(live) ** 3 + 1e-9
    return 1 + rng.multinomial(total - live, w / w.sum())


# ---------------------------------------------------------------- 1. parity
PARITY_LENS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 500, 2000]


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("n,total", [(1, 256), (2, 65536), (255, 40000), (256, 65536),
                                     (257, 65535), (1000, 65536), (4096, 65536)])
def test_parity_with_the_oracle(ctx, n, total, shift):
    rng = np.random.default_rng(n * 3 + shift)
    c, cum, t = table(spread(rng, n, total))
    assert t == total
    model = rc.WideStaticModel(c, cum, total)
    lens = PARITY_LENS + [int(x) for x in rng.integers(0, 300, 40 - len(PARITY_LENS))]
    order = rng.permutation(len(lens))
    chunks = [draw(rng, c, lens[i]) for i in order]
    assert len(chunks) == 40
    check_round_trip(model, c, cum, total, chunks, shift, seed=n + shift)


# ---------------------------------------------------------------- 2. table shapes
def sparse_table(rng, n, total):
    """Runs of more than 300 zero-frequency symbols, in front, inside and behind."""
    c = np.zeros(n, np.int64)
    if n == 4096:
        blocks = [(400, 440), (800, 860), (1200, 1201), (2000, 2050), (3700, 3740)]
    else:
        blocks = [(310, 340), (660, 680)]
    live = np.concatenate([np.arange(a, b) for a, b in blocks])
    assert len(live) <= total
    c[live] = spread(rng, len(live), total)
    return c


def shapes(rng, n, total):
    out = {}
    if total >= n:
        u = np.full(n, total // n, np.int64)
        u[: total - int(u.sum())] += 1
        out["uniform"] = u
        z = 1.0 / np.arange(1, n + 1) ** 1.2
        zc = 1 + np.floor(z / z.sum() * (total - n)).astype(np.int64)
        zc[0] += total - int(zc.sum())
        out["zipf"] = zc[rng.permutation(n)] if n < 4096 else zc
        s = np.ones(n, np.int64)
        s[n // 3] = total - (n - 1)
        out["spike"] = s
    out["sparse"] = sparse_table(rng, n, total)
    return out


@pytest.mark.parametrize("total", [65536, 65535, 40000, 4096, 256])
@pytest.mark.parametrize("n", [4096, 1000])
def test_table_shapes(ctx, n, total):
    rng = np.random.default_rng(n + total)
    tabs = shapes(rng, n, total)
    assert ("uniform" in tabs) == (total >= n)  # total 256: zero frequencies, n > total
    for name, freq in tabs.items():
        c, cum, t = table(freq)
        assert t == total, name
        if name == "sparse":
            z = np.flatnonzero(c)
            assert z[0] > 300 and n - 1 - z[-1] > 300 and np.diff(z).max() > 300
        model = rc.WideStaticModel(c, cum, total)
        chunks = [draw(rng, c, int(L)) for L in rng.integers(250, 351, 64)]
        check_round_trip(model, c, cum, total, chunks, shift=3 if name == "spike" else 0,
                         seed=total % 1000)


# ---------------------------------------------------------------- 3. workgroups
@pytest.fixture(scope="module")
def table_1000():
    rng = np.random.default_rng(1000)
    return table(spread(rng, 1000, 65536))


@pytest.mark.parametrize("n_chunks", [1091, 3])
def test_workgroups(ctx, table_1000, n_chunks):
    """1,091 chunks: more than one workgroup, a ragged last wave and dead lanes; 3 chunks: the
    small-launch path."""
    c, cum, total = table_1000
    model = rc.WideStaticModel(c, cum, total)
    rng = np.random.default_rng(n_chunks)
    chunks = [draw(rng, c, 64) for _ in range(n_chunks)]
    check_round_trip(model, c, cum, total, chunks, shift=0, seed=3)


# ---------------------------------------------------------------- 4. encode flags
def _flag_table():
    rng = np.random.default_rng(77)
    n, total = 1000, 40000
    f = spread(rng, n, total)
    f[0] += f[500]
    f[500] = 0  # the zero-frequency symbol
    return table(f)


def test_encode_flags(ctx):
    c, cum, total = _flag_table()
    n = len(c)
    model = rc.WideStaticModel(c, cum, total)
    rng = np.random.default_rng(78)
    chunks = [draw(rng, c, 300) for _ in range(70)]  # chunks 0..63 share a wave
    chunks[3][100] = 500                     # ZERO_FREQ
    chunks[10][0] = n                        # BAD_SYMBOL at n_symbols: head,
    chunks[11][150] = n                      # body
    chunks[12][299] = n                      # and tail of a chunk
    chunks[13][0] = 65535                    # and at the largest 16-bit value
    chunks[14][150] = 65535
    chunks[15][299] = 65535
    chunks[16][151] = 4096
    chunks[30][50] = 500                     # the first error wins, whatever its kind
    chunks[30][200] = n
    chunks[31][50] = 65535
    chunks[31][200] = 500
    chunks[32][7] = n
    chunks[32][8] = 500
    exp = [encode_ref(c, cum, total, s) for s in chunks]
    assert [exp[k][0] for k in (3, 10, 11, 12, 13, 14, 15, 16, 30, 31, 32)] == [
        N.F_ZERO_FREQ] + [N.F_BAD_SYMBOL] * 7 + [N.F_ZERO_FREQ, N.F_BAD_SYMBOL, N.F_BAD_SYMBOL]
    caps = [rc.slot_capacity(300, 16.0)] * 70
    caps[40] = len(exp[40][1]) - 1           # a slot one byte short
    for shift in (0, 7):
        h, out_off, ol, fl = run_encode(model, chunks, caps, shift, seed=5 + shift)
        for k, (f, b) in enumerate(exp):
            if k == 40:
                assert (int(fl[k]), int(ol[k])) == (N.F_CAPACITY, len(b))  # the exact length
                continue
            assert int(fl[k]) == f, (k, fl[k], f)
            if f == 0:  # the neighbours of the flagged chunks stay clean and bit-exact
                assert int(ol[k]) == len(b) and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, k
        # a retry with the reported length succeeds
        h, out_off, ol, fl = run_encode(model, [chunks[40]], [int(ol[40])], shift, seed=6)
        assert int(fl[0]) == 0 and bytes(h[out_off[0]:out_off[0] + ol[0]]) == exp[40][1]


def test_too_long_chunk_is_flagged_untouched(ctx, table_1000):
    c, cum, total = table_1000
    model = rc.WideStaticModel(c, cum, total)
    MAX = N.MAX_CHUNK_SYMBOLS
    s = draw(np.random.default_rng(7), c, 300)
    # chunk 2 claims MAX + 1 symbols starting inside a 300-symbol buffer
    sym_off = np.array([0, 100, 200, 200 + MAX + 1], np.int64)
    cap = 2048
    out_off = np.arange(4, dtype=np.int64) * cap
    out = torch.full((3 * cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    syms, _keep = _sym_arena(s, 0)
    out_len, flags = rc.encode_batch_wide(model, syms, dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    fl, ol, h = flags.cpu().numpy(), out_len.cpu().numpy(), out.cpu().numpy()
    assert fl.tolist() == [0, 0, N.F_TOO_LONG] and ol[2] == 0
    assert (h[2 * cap:] == SENT).all()  # the flagged slot and everything after it untouched
    for k in range(2):
        f, b = encode_ref(c, cum, total, s[sym_off[k]:sym_off[k + 1]])
        assert f == 0 and len(b) == ol[k] and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b
    code_len = ol.astype(np.int64).copy()
    code_len[2] = 64
    dec = torch.full((300 + 64,), int(SENT16), dtype=torch.int16, device="cuda")
    fd = rc.decode_batch_wide(model, out, dev(out_off[:3].copy()), dev(code_len), dec,
                              dev(sym_off))
    torch.cuda.synchronize()
    d = dec.cpu().numpy()
    assert fd.cpu().numpy().tolist() == [0, 0, N.F_TOO_LONG]
    assert np.array_equal(d[:200].view(np.uint16), s[:200]) and (d[200:] == SENT16).all()


# ---------------------------------------------------------------- 5. bad streams
def test_bad_streams(ctx):
    """Truncated and garbage streams over the sparse table: flags and the symbols before the
    first error equal the reference's, its choice of n_symbols - 1 when rfreq >= total
    included (there the last symbol has c == 0: CORRUPT)."""
    rng = np.random.default_rng(60)
    n, total = 4096, 65536
    c, cum, _ = table(sparse_table(rng, n, total))
    lit = literal_table(c)
    model = rc.WideStaticModel(c, cum, total)
    codes, counts = [], []
    s = draw(rng, c, 120)
    f, good = encode_ref(c, cum, total, s)
    assert f == 0 and len(good) > 40
    for cut in list(range(13)) + [20, 33, len(good) - 9, len(good) - 1, len(good)]:
        codes.append(good[:cut])
        counts.append(120)
    for k in range(64):
        codes.append(rng.integers(0, 256, int(rng.integers(8, 300))).astype(np.uint8).tobytes())
        counts.append(int(rng.integers(1, 201)))
    for k in range(16):  # a valid stream with one byte changed
        bad = bytearray(good)
        bad[8 + 5 * k] ^= 0x5A
        codes.append(bytes(bad))
        counts.append(120)
    exp = [decode_ref(c, cum, total, codes[k], counts[k], lit) for k in range(len(codes))]
    for cut in range(8):
        assert exp[cut][0] == N.F_TRUNCATED  # clen < 8
    assert {0, N.F_TRUNCATED, N.F_CORRUPT} <= {f for f, _ in exp[18:18 + 64]}
    assert {f for f, _ in exp} <= {0, N.F_TRUNCATED, N.F_CORRUPT}
    for shift in (0, 9):
        dec, fd = run_decode(model, codes, counts, shift, seed=61 + shift)
        for k, (f, want) in enumerate(exp):
            assert int(fd[k]) == f, (k, len(codes[k]), fd[k], f)
            assert np.array_equal(dec[k][:len(want)], want), (k, f)
            if f == 0:
                assert len(want) == counts[k]


# ---------------------------------------------------------------- 6. the existing coders
@pytest.mark.parametrize("n,L", [(4096, 4096), (1 << 18, 64)])
def test_one_byte_alphabets_agree_with_the_static_coders(ctx, n, L):
    """No oracle: at n_symbols = 256 the wide coders produce, on the widened symbols, the slots,
    lengths and flags of rc_encode_batch on the StaticModel of the same table, and decode back.
    4,096 chunks are small workgroups; 2^18 chunks give every CU one of the plan's full size."""
    c, cum, total = synth.zipf_table()
    m = rc.StaticModel(c, cum, total)
    w = rc.WideStaticModel(c, cum, total)
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
    syms16 = syms.to(torch.int16)
    out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    out_len, fl = rc.encode_batch_wide(w, syms16, sym_off, out, out_off)
    torch.cuda.synchronize()
    assert torch.equal(out_len, want_len) and torch.equal(fl, want_fl)
    assert torch.equal(out.view(n, cap) * valid, want.view(n, cap) * valid)
    dec = torch.full_like(syms16, int(SENT16))
    fd = rc.decode_batch_wide(w, out, out_off[:-1].contiguous(), out_len, dec, sym_off)
    torch.cuda.synchronize()
    assert int(fd.abs().sum()) == 0 and torch.equal(dec, syms16)


# ---------------------------------------------------------------- 7. kinds do not mix
def test_kinds_do_not_mix(ctx, table_1000):
    c, cum, total = table_1000
    w = rc.WideStaticModel(c, cum, total)
    lib = ctx._lib
    zc, zcum, zt = synth.zipf_table()
    m = rc.StaticModel(zc, zcum, zt)
    am = rc.AdaptiveModel(256, **rc.ADAPTIVE_DEFAULTS)
    ms = rc.StaticModelSet(np.tile(np.asarray(zc, np.uint32), (2, 1)), None, zt)
    syms = torch.zeros(512, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 128, 256], dtype=torch.int64, device="cuda")
    out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    out_off = torch.tensor([0, 2048, 4096], dtype=torch.int64, device="cuda")
    ol = torch.zeros(2, dtype=torch.int64, device="cuda")
    fl = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    h = w.handle
    # a wide model to every other entry point that takes a model
    assert lib.rc_encode_batch(ctx.handle, h, p(syms), p(off), 2, p(out), p(out_off), p(ol),
                               p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch(ctx.handle, h, p(out), p(out_off), p(ol), p(syms), p(off), 2,
                               p(fl)) == N.RC_E_ARG
    assert lib.rc_encode_batch_indexed(ctx.handle, h, p(syms), p(syms), p(off), 2, p(out),
                                       p(out_off), p(ol), p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch_indexed(ctx.handle, h, p(out), p(out_off), p(ol), p(syms), p(syms),
                                       p(off), 2, p(fl)) == N.RC_E_ARG
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    n_out = ctypes.c_uint64()
    assert lib.rc_container_pack(ctx.handle, h, p(out), p(out_off), p(ol), p(off), 2, p(dst),
                                 8192, ctypes.byref(n_out)) == N.RC_E_ARG
    hs = np.zeros(256, np.uint8)
    ho = np.array([0, 128, 256], np.uint64)
    oo = np.array([0, 2048, 4096], np.uint64)
    with pytest.raises(N.RCError) as e:
        rc.encode_host(w, hs, ho, oo)
    assert e.value.code == N.RC_E_ARG
    with pytest.raises(N.RCError) as e:
        rc.decode_host(w, np.zeros(64, np.uint8), np.array([0, 32], np.uint64),
                       np.array([32, 32], np.uint64), ho)
    assert e.value.code == N.RC_E_ARG
    with pytest.raises(N.RCError) as e:
        rc.encode_host_multi([w], hs, ho, oo)
    assert e.value.code == N.RC_E_ARG
    # every other model to the wide calls
    for other in (m, am, ms):
        assert lib.rc_encode_batch_wide(ctx.handle, other.handle, p(syms), p(off), 2, p(out),
                                        p(out_off), p(ol), p(fl)) == N.RC_E_ARG
        assert lib.rc_decode_batch_wide(ctx.handle, other.handle, p(out), p(out_off), p(ol),
                                        p(syms), p(off), 2, p(fl)) == N.RC_E_ARG
    # 16-bit symbols at an odd address
    odd = ctypes.c_void_p(syms.data_ptr() + 1)
    assert lib.rc_encode_batch_wide(ctx.handle, h, odd, p(off), 2, p(out), p(out_off), p(ol),
                                    p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch_wide(ctx.handle, h, p(out), p(out_off), p(ol), odd, p(off), 2,
                                    p(fl)) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()  # nothing was launched
    # the Python mirror takes 16-bit tensors only
    with pytest.raises(TypeError):
        rc.encode_batch_wide(w, syms, off, out, out_off)
    with pytest.raises(TypeError):
        rc.decode_batch_wide(w, out, out_off[:2].contiguous(), ol, syms, off)
    with pytest.raises(TypeError):
        rc.encode_batch_wide(w, syms.to(torch.int32), off, out, out_off)


# ---------------------------------------------------------------- 8. the Python mirror
def test_chunk_helpers_round_trip_and_raise(ctx):
    c, cum, total = _flag_table()
    model = rc.WideStaticModel(c, cum, total)
    rng = np.random.default_rng(90)
    chunks = [draw(rng, c, L) for L in (0, 5, 1000, 64)]
    codes = rc.encode_chunks_wide(model, chunks)
    for s, b in zip(chunks, codes):
        assert encode_ref(c, cum, total, s) == (0, b)
    back = rc.decode_chunks_wide(model, codes, [len(s) for s in chunks])
    for s, d in zip(chunks, back):
        assert d.dtype == np.uint16 and np.array_equal(s, d)
    assert rc.encode_chunks_wide(model, [[int(x) for x in chunks[1]]]) == [codes[1]]
    s = draw(rng, c, 100)
    s[40] = 1000
    with pytest.raises(rc.BadSymbolError):
        rc.encode_chunks_wide(model, [s])
    with pytest.raises(rc.BadSymbolError):
        rc.encode_chunks_wide(model, [[1, 2, 70000]])
    s[40] = 500
    with pytest.raises(rc.ZeroFrequencyError):
        rc.encode_chunks_wide(model, [s])
    with pytest.raises(rc.TruncatedStreamError):
        rc.decode_chunks_wide(model, [codes[2][:20]], [1000])
    # uint16 tensors, where this torch has them, are the native form
    if hasattr(torch, "uint16"):
        t = dev(chunks[2].view(np.int16)).view(torch.uint16)
        out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        off = torch.tensor([0, 1000], dtype=torch.int64, device="cuda")
        ol, fl = rc.encode_batch_wide(model, t, off, out,
                                      torch.tensor([0, 4096], dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        assert int(fl[0]) == 0 and bytes(out.cpu().numpy()[:int(ol[0])]) == codes[2]


# ---------------------------------------------------------------- 9. the C++ example
def test_cpp_wide_impl(ctx):
    """examples/wide_impl: sample_impl with a FreqTable of 1000 symbols through rc::WideModel,
    against the per-call rc::Encoder given the same table."""
    exe = os.path.join(ROOT, "examples", "wide_impl")
    assert os.path.exists(exe), "examples/wide_impl not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test passed" in r.stdout
