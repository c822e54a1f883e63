"""The order-1 batch coders (rc_encode_batch_order1 / rc_decode_batch_order1: the previous symbol
of the chunk picks the row of a static model set) through the C ABI, against the CPU oracle
(order1_ref.py) and against the existing coders: ragged and misaligned arenas, sentinel bytes
around the slots and the decoded range, every tile seam, every set shape, the rare paths, flags,
bad streams, the kind checks, rc_histogram_order1, the Python helpers and the C++ example."""
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
from order1_ref import (decode_ref, derive_idx, draw_markov, encode_ref, markov_rows,  # noqa: E402
                        tables)

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


def sym_arena(chunks, misalign, rng, head=None):
    """Symbols of `chunks` at contiguous ragged offsets; misalign: a random number of bytes in
    front and a random base offset (head: that number of bytes in front, base aligned)."""
    lens = np.array([len(s) for s in chunks], np.int64)
    pre = int(rng.integers(0, 16)) if misalign else 0
    bs = int(rng.integers(0, 16)) if misalign else 0
    if head is not None:
        pre, bs = head, 0
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + pre
    cat = np.concatenate([rng.integers(0, 256, pre).astype(np.uint8)] +
                         [np.asarray(s, np.uint8) for s in chunks] + [np.zeros(1, np.uint8)])
    syms, keep = _shifted(dev(cat), bs)
    return syms, keep, sym_off


def run_encode(o1, chunks, caps, misalign=False, seed=0, head=None):
    rng = np.random.default_rng(seed)
    syms, _ks, sym_off = sym_arena(chunks, misalign, rng, head)
    bo = int(rng.integers(0, 16)) if misalign else 0
    caps = np.asarray(caps, np.int64)
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + bo
    out = torch.full((int(out_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = rc.encode_batch_order1(o1, syms, dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    # nothing is written outside the slots (bytes past out_len inside a slot are unspecified)
    assert (h[:bo] == SENT).all() and (h[out_off[-1]:] == SENT).all()
    return h, out_off, out_len.cpu().numpy(), flags.cpu().numpy()


def run_decode(o1, codes, counts, misalign=False, seed=0, head=None):
    """codes at random gaps, decoded symbols at a random byte offset."""
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
    counts = np.asarray(counts, np.int64)
    pre = int(rng.integers(0, 16)) if misalign else 0
    bc, bs = (int(x) for x in rng.integers(0, 16, 2)) if misalign else (0, 0)
    if head is not None:
        pre, bs = head, 0
    sym_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) + pre
    code, _kc = _shifted(dev(np.concatenate(parts)), bc)
    big = torch.full((int(sym_off[-1]) + bs + 64,), SENT, dtype=torch.uint8, device="cuda")
    syms = big[bs:]
    flags = rc.decode_batch_order1(o1, code, dev(coff), dev(clen), syms, dev(sym_off))
    torch.cuda.synchronize()
    s = syms.cpu().numpy()
    b = big.cpu().numpy()
    # nothing is written outside the chunks' symbol ranges
    assert (b[:bs + sym_off[0]] == SENT).all() and (b[bs + sym_off[-1]:] == SENT).all()
    return [s[sym_off[k]:sym_off[k + 1]] for k in range(n)], flags.cpu().numpy()


def check_round_trip(o1, c, cum, chunks, misalign, seed, slack=64, head=None):
    """Encode and decode `chunks`; bytes, lengths and flags equal the oracle's, and decode
    returns the symbols with flags 0."""
    bits = o1.max_bits_per_symbol() + 1
    caps = [rc.slot_capacity(len(s), bits) + slack for s in chunks]
    h, out_off, ol, fl = run_encode(o1, chunks, caps, misalign, seed, head)
    codes = []
    for k, s in enumerate(chunks):
        f, b = encode_ref(c, cum, o1.total, o1.ctx_map, o1.first_row, s)
        assert (int(fl[k]), int(ol[k])) == (f, len(b)), (k, len(s), fl[k], ol[k], f, len(b))
        assert bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, (k, len(s))
        codes.append(b)
    dec, fd = run_decode(o1, codes, [len(s) for s in chunks], misalign, seed + 1, head)
    for k, s in enumerate(chunks):
        assert fd[k] == 0 and np.array_equal(dec[k], np.asarray(s, np.uint8)), (k, len(s))
    return codes


# ---------------------------------------------------------------- 1. parity
def parity_rows():
    """K = 8, 256 symbols, total 65536: shifted Zipf tables, one row with a block of
    zero-frequency symbols (never drawn: their probability is 0), one spike (the rows of the
    indexed tests' parity_rows)."""
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


PARITY_LENS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 640, 4099]


@pytest.fixture(scope="module")
def parity(ctx):
    """The parity set (map s -> s >> 5, first_row 7) and 200 chunks of its Markov chain."""
    c, cum = parity_rows()
    ctx_map = (np.arange(256) >> 5).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, 65536, ctx_map=ctx_map, first_row=7)
    rng = np.random.default_rng(11)
    chunks = [draw_markov(rng, c, ctx_map, 7, PARITY_LENS[k % len(PARITY_LENS)])
              for k in range(200)]
    return o1, c, cum, chunks


@pytest.mark.parametrize("misalign", [False, True])
def test_parity_with_the_oracle(parity, misalign):
    o1, c, cum, chunks = parity
    check_round_trip(o1, c, cum, chunks, misalign, seed=100 + misalign)


# ---------------------------------------------------------------- 2. the tile seams
def test_tile_seams(ctx):
    """Two rows with disjoint supports: row 0 gives c > 0 to even symbols only, row 1 to odd
    ones; the map sends a symbol to the row that allows the other parity, so a valid chunk
    alternates parity and a previous symbol taken from the wrong place at any seam (chunk start,
    byte-wise head into the first tile, tile to tile, byte-wise tail) is RC_F_ZERO_FREQ or wrong
    bytes.  One launch per head misalignment 0..15, one chunk per length 14..34 in each; the
    chunks before a chunk shift its start, so the lengths sweep further alignments."""
    n, total = 64, 4096
    rng = np.random.default_rng(22)
    rows = np.zeros((2, n), np.int64)
    for j in range(2):
        w = rng.random(n // 2) + 0.05
        rows[j, j::2] = 1 + rng.multinomial(total - n // 2, w / w.sum())
    c, cum = tables(rows)
    ctx_map = ((np.arange(n) + 1) & 1).astype(np.uint8)  # even symbol -> row 1 (odd next)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=ctx_map, first_row=0)
    chunks = [draw_markov(rng, c, ctx_map, 0, L) for L in range(14, 35)]
    for s in chunks:
        assert ((s.astype(np.int64) + np.arange(len(s))) % 2 == 0).all()  # parities alternate
    # longer chunks as well: several 64-symbol tiles after each head
    chunks += [draw_markov(rng, c, ctx_map, 0, L) for L in (63, 64, 65, 128, 129, 200)]
    for head in range(16):
        check_round_trip(o1, c, cum, chunks, False, seed=220 + head, head=head)


# ---------------------------------------------------------------- 3. shapes of the set
@pytest.mark.parametrize("total", [256, 257, 40000, 65535])
@pytest.mark.parametrize("K", [1, 64])
def test_set_shapes(ctx, K, total):
    rng = np.random.default_rng(K * 100003 + total)
    n = 100
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    ctx_map = rng.integers(0, K, n).astype(np.uint8)
    first = int(rng.integers(0, K))
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=ctx_map, first_row=first)
    lens = [int(x) for x in rng.integers(0, 2001, 18)] + [0, 2000]
    chunks = [draw_markov(rng, c, ctx_map, first, L) for L in lens]
    check_round_trip(o1, c, cum, chunks, misalign=bool(K == 64), seed=total)


# ---------------------------------------------------------------- 4. the existing coders
@pytest.mark.parametrize("n,L", [(4096, 4096), (1 << 18, 64)])
def test_matches_the_static_and_the_indexed_coders(ctx, n, L):
    """No oracle: a K = 1 order-1 set produces the slots, lengths and flags of rc_encode_batch on
    the StaticModel of its row; a K = 16 set with a random map those of rc_encode_batch_indexed
    fed the index stream derived on the GPU by a gather; both decode back.  4,096 chunks of 4 KiB
    are sixteen 256-lane workgroups; 2^18 chunks of 64 symbols give every CU a workgroup of the
    plan's full size."""
    c, cum, total = synth.zipf_table()
    syms = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    synth.fill(ctx, 0x01D5EED, synth.inverse_cdf(c), syms, L, n)
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    # (a rotated row gives the data's frequent symbols small counts: up to log2(65536 / min c))
    cap = rc.slot_capacity(L, float(np.log2(total / min(c))))
    out_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap
    rng = np.random.default_rng(5)
    for K in (1, 16):
        rows = np.tile(np.asarray(c, np.uint32), (K, 1))
        if K == 1:
            ctx_map, first = np.zeros(256, np.uint8), 0
            m = rc.StaticModel(c, cum, total)
            want = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
            want_len, want_fl = rc.encode_batch(m, syms, sym_off, want, out_off)
        else:
            # rows that differ: each a rotation of the table (every c > 0, so no flags)
            rows = np.stack([np.roll(rows[0], 16 * j) for j in range(K)])
            ctx_map, first = rng.integers(0, K, 256).astype(np.uint8), 5
            mset = rc.StaticModelSet(rows, None, total)
            idx = dev(ctx_map)[syms.long()].view(n, L).roll(1, dims=1)
            idx[:, 0] = first
            idx = idx.reshape(-1).contiguous()
            want = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
            want_len, want_fl = rc.encode_batch_indexed(mset, syms, idx, sym_off, want, out_off)
        torch.cuda.synchronize()
        assert int(want_fl.abs().sum()) == 0
        valid = torch.arange(cap, device="cuda")[None, :] < want_len[:, None]
        o1 = rc.Order1ModelSet(rows, None, total, ctx_map=ctx_map, first_row=first)
        out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        out_len, fl = rc.encode_batch_order1(o1, syms, sym_off, out, out_off)
        torch.cuda.synchronize()
        assert torch.equal(out_len, want_len) and torch.equal(fl, want_fl), K
        assert torch.equal(out.view(n, cap) * valid, want.view(n, cap) * valid), K
        dec = torch.zeros_like(syms)
        fd = rc.decode_batch_order1(o1, out, out_off[:-1].contiguous(), out_len, dec, sym_off)
        torch.cuda.synchronize()
        assert int(fd.abs().sum()) == 0 and torch.equal(dec, syms), K


# ---------------------------------------------------------------- 5. many short chunks
def test_many_short_chunks_fill_several_workgroups(ctx):
    """K = 64: 1,700 chunks of 0..80 symbols are more than any plan's workgroup holds, all checked
    against the oracle, misaligned."""
    rng = np.random.default_rng(64)
    n, total = 256, 65536
    c, cum = tables(markov_rows(rng, 64, n, total))
    ctx_map = rng.integers(0, 64, n).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=ctx_map, first_row=33)
    plan = (ctypes.c_uint32 * 8)()
    assert N.load().rc_model_order1_plan_(64, total, plan) == N.RC_OK
    assert 1700 > 3 * plan[0] and 1700 > 2 * plan[4]  # (encoder / decoder lanes per workgroup)
    lens = rng.integers(0, 81, 1700)
    chunks = [draw_markov(rng, c, ctx_map, 33, int(L)) for L in lens]
    check_round_trip(o1, c, cum, chunks, misalign=True, seed=640)


# ---------------------------------------------------------------- 6. rare path
@pytest.mark.parametrize("misalign", [False, True])
def test_rare_heavy_rows(ctx, misalign):
    """The two rows of the indexed tests' rare-path case (nearly every coded symbol c = 1 of
    65536, so 2-3 bytes settle per symbol and range_reduction_expansion runs often; and a spike
    row), with a map that alternates them: symbols below 128 pick row 1, the others row 0."""
    total = 65536
    a = np.ones(256, np.int64)
    a[0] = 2000
    a[1] = total - 2000 - 254
    b = np.ones(256, np.int64)
    b[200] = total - 255
    c, cum = tables([a, b])
    ctx_map = (np.arange(256) < 128).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=ctx_map, first_row=0)
    rng = np.random.default_rng(40 + misalign)
    chunks = []
    for L in [64, 640, 4096, 4099, 1000, 127, 0]:
        s = rng.integers(2, 256, L)
        s[rng.random(L) < 0.05] = 0
        s[rng.random(L) < 0.3] = 200
        chunks.append(s.astype(np.uint8))
    rows_used = np.concatenate([derive_idx(ctx_map, 0, s, 256) for s in chunks])
    assert 0.2 < rows_used.mean() < 0.8  # both rows in use, switching often
    check_round_trip(o1, c, cum, chunks, misalign, seed=400 + misalign)


# ---------------------------------------------------------------- 7. flags
def _flag_set():
    """n = 200 symbols, K = 4, total 40000; symbol 50 has c = 0 in row 2 only.  Map: s -> s & 3,
    so symbol 50 is refused after a symbol with s & 3 == 2 and passes after any other."""
    rng = np.random.default_rng(77)
    n, K, total = 200, 4, 40000
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        rows[j] += rng.multinomial(total - n, np.ones(n) / n)
    rows[2, 0] += rows[2, 50]
    rows[2, 50] = 0
    return tables(rows), total, (np.arange(n) & 3).astype(np.uint8)


def test_encode_flags(ctx):
    (c, cum), total, ctx_map = _flag_set()
    K, n = c.shape
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=ctx_map, first_row=1)
    rng = np.random.default_rng(78)
    chunks = [draw_markov(rng, c, ctx_map, 1, 300) for _ in range(70)]  # 0..63 share a wave

    def put(k, pos, *syms):
        chunks[k][pos:pos + len(syms)] = syms

    put(3, 100, 6, 50, 9)       # ZERO_FREQ: 50 after a symbol of class 2
    put(4, 100, 7, 50, 9)       # the same symbol passes under another context
    put(5, 0, 50)               # and as a chunk's first symbol (first_row 1)
    put(10, 200, n)             # BAD_SYMBOL (symbol >= n_symbols) at 200,
    put(11, 0, 255)             # at 0
    put(12, 299, n + 5)         # and at 299
    put(30, 50, 2, 50)          # two errors in one chunk: the first wins
    put(30, 200, n)
    put(31, 50, n + 1)
    put(31, 200, 2, 50)
    put(32, 7, n, 50)           # after a bad symbol (row 0 follows: 50 would pass there)
    exp = [encode_ref(c, cum, total, ctx_map, 1, s) for s in chunks]
    assert [exp[k][0] for k in (3, 4, 5, 10, 11, 12, 30, 31, 32)] == [
        N.F_ZERO_FREQ, 0, 0, N.F_BAD_SYMBOL, N.F_BAD_SYMBOL, N.F_BAD_SYMBOL, N.F_ZERO_FREQ,
        N.F_BAD_SYMBOL, N.F_BAD_SYMBOL]
    caps = [rc.slot_capacity(300, 16.0)] * 70
    caps[40] = len(exp[40][1]) - 1          # a slot one byte short
    for mis in (False, True):
        h, out_off, ol, fl = run_encode(o1, chunks, caps, mis, seed=5 + mis)
        for k, (f, b) in enumerate(exp):
            if k == 40:
                assert (int(fl[k]), int(ol[k])) == (N.F_CAPACITY, len(b))  # the exact length
                continue
            assert int(fl[k]) == f, (k, fl[k], f)
            if f == 0:  # the neighbours of the flagged chunks stay clean and bit-exact
                assert int(ol[k]) == len(b) and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, k


def test_bad_streams_and_decode_flags(parity):
    """Garbage and truncated streams, a 7-byte stream and an empty chunk over a 7-byte code: the
    flags equal the reference's and, where the flag is 0, so do the symbols."""
    o1, c, cum, _ = parity
    rng = np.random.default_rng(60)
    codes, counts = [], []
    for k in range(64):
        codes.append(rng.integers(0, 256, int(rng.integers(8, 401))).astype(np.uint8).tobytes())
        counts.append(300)
    for cut in range(1, 9):
        s = draw_markov(rng, c, o1.ctx_map, 7, 300)
        f, b = encode_ref(c, cum, 65536, o1.ctx_map, 7, s)
        assert f == 0
        codes.append(b[:len(b) - cut])
        counts.append(300)
    codes += [bytes(7), bytes(7)]
    counts += [10, 0]
    exp = [decode_ref(c, cum, 65536, o1.ctx_map, 7, codes[k], counts[k])
           for k in range(len(codes))]
    # the reference alone: garbage that is refused and garbage that decodes to something
    assert any(f for f, _ in exp[:64]) and any(f == 0 for f, _ in exp[:64])
    assert any(f == N.F_TRUNCATED for f, _ in exp[64:72])
    assert [f for f, _ in exp[72:]] == [N.F_TRUNCATED, N.F_TRUNCATED]
    for mis in (False, True):
        dec, fd = run_decode(o1, codes, counts, mis, seed=61 + mis)
        for k, (f, s) in enumerate(exp):
            assert int(fd[k]) == f, (k, len(codes[k]), fd[k], f)
            if f == 0:
                assert np.array_equal(dec[k], s), k


def test_too_long_chunk_is_flagged_untouched(parity):
    o1, c, cum, _ = parity
    MAX = N.MAX_CHUNK_SYMBOLS
    rng = np.random.default_rng(7)
    s = draw_markov(rng, c, o1.ctx_map, 7, 300)
    # chunk 2 claims MAX + 1 symbols starting inside a 300-byte symbol buffer
    sym_off = np.array([0, 100, 200, 200 + MAX + 1], np.int64)
    cap = 2048
    out_off = np.arange(4, dtype=np.int64) * cap
    out = torch.full((3 * cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = rc.encode_batch_order1(o1, dev(s), dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    fl, ol, h = flags.cpu().numpy(), out_len.cpu().numpy(), out.cpu().numpy()
    assert fl.tolist() == [0, 0, N.F_TOO_LONG] and ol[2] == 0
    assert (h[2 * cap:] == SENT).all()  # the flagged slot and everything after it untouched
    for k in range(2):
        f, b = encode_ref(c, cum, 65536, o1.ctx_map, 7, s[sym_off[k]:sym_off[k + 1]])
        assert f == 0 and len(b) == ol[k] and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b
    code_len = ol.astype(np.int64).copy()
    code_len[2] = 64
    dec = torch.full((300 + 64,), SENT, dtype=torch.uint8, device="cuda")
    fd = rc.decode_batch_order1(o1, out, dev(out_off[:3].copy()), dev(code_len), dec,
                                dev(sym_off))
    torch.cuda.synchronize()
    d = dec.cpu().numpy()
    assert fd.cpu().numpy().tolist() == [0, 0, N.F_TOO_LONG]
    assert np.array_equal(d[:200], s[:200]) and (d[200:] == SENT).all()


# ---------------------------------------------------------------- 10. kinds do not mix
def test_kinds_do_not_mix(ctx, parity):
    o1, c, cum, _ = parity
    lib = ctx._lib
    m = rc.StaticModel(c[0], cum[0], 65536)
    am = rc.AdaptiveModel(256, **rc.ADAPTIVE_DEFAULTS)
    mset = rc.StaticModelSet(c, cum, 65536)
    wide = rc.WideStaticModel(c[0], cum[0], 65536)
    syms = torch.zeros(256, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(256, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 128, 256], dtype=torch.int64, device="cuda")
    off16 = torch.tensor([0, 64, 128], dtype=torch.int64, device="cuda")
    out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    out_off = torch.tensor([0, 2048, 4096], dtype=torch.int64, device="cuda")
    ol = torch.zeros(2, dtype=torch.int64, device="cuda")
    fl = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    h = o1.handle
    # an order-1 set in every other entry point that takes a model
    assert lib.rc_encode_batch(ctx.handle, h, p(syms), p(off), 2, p(out), p(out_off), p(ol),
                               p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch(ctx.handle, h, p(out), p(out_off), p(ol), p(syms), p(off), 2,
                               p(fl)) == N.RC_E_ARG
    assert lib.rc_encode_batch_indexed(ctx.handle, h, p(syms), p(idx), p(off), 2, p(out),
                                       p(out_off), p(ol), p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch_indexed(ctx.handle, h, p(out), p(out_off), p(ol), p(idx), p(syms),
                                       p(off), 2, p(fl)) == N.RC_E_ARG
    assert lib.rc_encode_batch_wide(ctx.handle, h, p(syms), p(off16), 2, p(out), p(out_off),
                                    p(ol), p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch_wide(ctx.handle, h, p(out), p(out_off), p(ol), p(syms), p(off16),
                                    2, p(fl)) == N.RC_E_ARG
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    n_out = ctypes.c_uint64()
    assert lib.rc_container_pack(ctx.handle, h, p(out), p(out_off), p(ol), p(off), 2, p(dst),
                                 8192, ctypes.byref(n_out)) == N.RC_E_ARG
    hs = np.zeros(256, np.uint8)
    ho = np.array([0, 128, 256], np.uint64)
    with pytest.raises(N.RCError) as e:
        rc.encode_host(o1, hs, ho, np.array([0, 2048, 4096], np.uint64))
    assert e.value.code == N.RC_E_ARG
    with pytest.raises(N.RCError) as e:
        rc.encode_host_multi([o1], hs, ho, np.array([0, 2048, 4096], np.uint64))
    assert e.value.code == N.RC_E_ARG
    # and every other kind of model in the order-1 calls
    for other in (m, am, mset, wide):
        assert lib.rc_encode_batch_order1(ctx.handle, other.handle, p(syms), p(off), 2, p(out),
                                          p(out_off), p(ol), p(fl)) == N.RC_E_ARG
        assert lib.rc_decode_batch_order1(ctx.handle, other.handle, p(out), p(out_off), p(ol),
                                          p(syms), p(off), 2, p(fl)) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()  # nothing was launched
    assert int(syms.abs().sum()) == 0


# ---------------------------------------------------------------- 11. model construction
def _hist_ref(chunks, ctx_map256, first_row, K):
    want = np.zeros((K, 256), np.int64)
    for s in chunks:
        np.add.at(want, (derive_idx(ctx_map256, first_row, s, 256).astype(np.int64),
                         np.asarray(s, np.int64)), 1)
    return want


def test_histogram_order1_on_a_ragged_arena(parity):
    o1, c, cum, chunks = parity
    rng = np.random.default_rng(110)
    syms, _ks, sym_off = sym_arena(chunks, True, rng)
    assert min(len(s) for s in chunks) == 0 and 1 in [len(s) for s in chunks]
    want = _hist_ref(chunks, o1.ctx_map, 7, 8)
    base = rng.integers(0, 1000, (8, 256)).astype(np.int64)  # counts are ADDED into hist
    hist = dev(base.copy())
    got = rc.histogram_order1(syms, dev(sym_off), o1.ctx_map, 7, n_models=8, hist=hist)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.array_equal(g - base, want)
    assert int((g - base).sum()) == sum(len(s) for s in chunks)
    with pytest.raises(ValueError):
        rc.histogram_order1(syms, dev(sym_off), o1.ctx_map, 8, n_models=8)  # first_row = K
    with pytest.raises(ValueError):
        rc.histogram_order1(syms, dev(sym_off), o1.ctx_map, 0, n_models=7)  # a map entry = K


def test_histogram_order1_on_a_large_arena(ctx):
    n, L, K = 1 << 12, 4096, 64
    c, _, _ = synth.zipf_table()
    syms = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    synth.fill(ctx, 0x0B1D5EED, synth.inverse_cdf(c), syms, L, n)
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    ctx_map = np.random.default_rng(111).integers(0, K, 256).astype(np.uint8)
    got = rc.histogram_order1(syms, sym_off, ctx_map, 9, n_models=K)
    torch.cuda.synchronize()
    h = syms.cpu().numpy().reshape(n, L).astype(np.int64)
    idx = ctx_map[np.roll(h, 1, axis=1)].astype(np.int64)
    idx[:, 0] = 9
    want = np.bincount((idx * 256 + h).ravel(), minlength=K * 256).reshape(K, 256)
    assert np.array_equal(got.cpu().numpy(), want) and int(want.sum()) == n * L


def test_build_order1_set_round_trips_and_beats_order_0(ctx):
    """A 4-state source whose rows are far apart (each row keeps 7/8 of its mass on its own 16
    symbols): the order-1 set built from the data codes it in well under the bytes of the order-0
    model built from the same data.  The inequality is checked on the CPU reference first, so a
    failure on the GPU means the contexts are wired the wrong way round, not a weak source."""
    rng = np.random.default_rng(120)
    K, n, total = 4, 64, 65536
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        rows[j, 16 * j:16 * j + 16] += (total - n) * 7 // 8 // 16
        rows[j, 0] += total - rows[j].sum()
    c, _ = tables(rows)
    ctx_map = ((np.arange(n) >> 2) & 3).astype(np.uint8)  # the next state: bits 2..3
    chunks = [draw_markov(rng, c, ctx_map, 0, 3000) for _ in range(8)]
    # the CPU reference: order-1 rows from exact pair counts against one order-0 table
    cnt1 = _hist_ref(chunks, ctx_map, 0, K)[:, :n]
    q1 = [rc.quantize_counts(r, total, all_symbols=True) for r in cnt1]
    c1, cum1 = tables([q[0] for q in q1])
    q0 = rc.quantize_counts(cnt1.sum(axis=0), total, all_symbols=True)
    c0, cum0 = tables([q0[0]])
    ref1 = sum(len(encode_ref(c1, cum1, total, ctx_map, 0, s)[1]) for s in chunks)
    ref0 = sum(len(encode_ref(c0, cum0, total, np.zeros(n, np.uint8), 0, s)[1]) for s in chunks)
    assert ref1 < 0.8 * ref0, (ref1, ref0)
    # the GPU: the same set from rc_histogram_order1, the same bytes, a round trip
    syms, _ks, sym_off = sym_arena(chunks, False, rng)
    o1 = rc.build_order1_set(syms, dev(sym_off), ctx_map, 0, total, n_symbols=n)
    assert np.array_equal(o1.c, c1) and o1.n_models == K
    codes = rc.encode_chunks_order1(o1, chunks)
    assert sum(len(b) for b in codes) == ref1
    back = rc.decode_chunks_order1(o1, codes, [len(s) for s in chunks])
    assert all(np.array_equal(a, b) for a, b in zip(back, chunks))
    m0 = rc.build_model(syms, dev(sym_off), total, n_symbols=n)
    size0 = sum(len(b) for b in rc.encode_chunks(m0, chunks))
    assert size0 == ref0 and sum(len(b) for b in codes) < 0.8 * size0


# ---------------------------------------------------------------- 12. the mirrors
def test_chunk_helpers_round_trip_and_raise(parity):
    o1, c, cum, _ = parity
    rng = np.random.default_rng(90)
    chunks = [draw_markov(rng, c, o1.ctx_map, 7, L) for L in (0, 5, 1000, 64)]
    codes = rc.encode_chunks_order1(o1, chunks)
    for s, b in zip(chunks, codes):
        assert encode_ref(c, cum, 65536, o1.ctx_map, 7, s) == (0, b)
    back = rc.decode_chunks_order1(o1, codes, [len(s) for s in chunks])
    for s, d in zip(chunks, back):
        assert np.array_equal(s, d)
    s = chunks[2].copy()
    s[40:42] = (6 * 32, 120)  # a zero-frequency symbol of row 6, after a symbol of class 6
    with pytest.raises(rc.ZeroFrequencyError):
        rc.encode_chunks_order1(o1, [s])
    (c4, cum4), total4, map4 = _flag_set()
    small = rc.Order1ModelSet(c4, cum4, total4, ctx_map=map4, first_row=0)
    with pytest.raises(rc.BadSymbolError):
        rc.encode_chunks_order1(small, [np.array([1, 2, 250, 3], np.uint8)])
    with pytest.raises(rc.TruncatedStreamError):
        rc.decode_chunks_order1(o1, [codes[2][:20]], [1000])


def test_cpp_order1_impl(ctx):
    """examples/order1_impl: FreqTables by previous-byte class through rc::Order1Set, against the
    per-call rc::Encoder / rc::Decoder given the same tables."""
    exe = os.path.join(ROOT, "examples", "order1_impl")
    assert os.path.exists(exe), "examples/order1_impl not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test passed" in r.stdout
