"""Periodic order-1 sets on the GPU (rc_model_create_order1_set_periodic: the position in a record
joins the context) through rc_encode_batch_order1 / rc_decode_batch_order1, against the CPU
oracle (periodic_ref.py) and against the period-1 coders: byte parity with per-lane heads of
every length, the decoder against the oracle's stream decoder on sound and bad streams, encoder
errors judged with the phase, identity with the existing sets, rc_histogram_pairs_periodic,
rc_ideal_bits_order1, the refusals and the fit."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from gpu_helpers import dev  # noqa: E402
from order1_ref import markov_rows  # noqa: E402
import periodic_ref as ref  # noqa: E402

SENT = 0xEE
tables = ref.tables


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------- arenas
def layout(lens, rng, gap=4):
    """Offsets of chunks of `lens` symbols with 0 .. gap - 1 stray bytes before each."""
    lens = np.asarray(lens, np.int64)
    gaps = rng.integers(0, gap, len(lens))
    start = np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))
    return start.astype(np.int64), int(start[-1] + lens[-1]) if len(lens) else 0


def arena(chunks, start, size, fill):
    """A 64-B aligned device buffer of `size` bytes holding chunk k at start[k], `fill` elsewhere."""
    h = np.full(size + 64, fill, np.uint8)
    for s, o in zip(chunks, start):
        h[o:o + len(s)] = s
    t = dev(h)
    assert t.data_ptr() % 64 == 0
    return t


def run_encode(o1, chunks, rng, pre=None, bits=17.0):
    """Encode `chunks` laid out back to back (ragged, so the starts sweep the residues mod 64)
    behind `pre` stray bytes (default: a random number).  Returns (host slots, out_off, out_len,
    flags)."""
    lens = np.array([len(s) for s in chunks], np.int64)
    pre = int(rng.integers(0, 64)) if pre is None else pre
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + pre
    syms = arena(chunks, sym_off[:-1], int(sym_off[-1]), 0)
    caps = np.array([rc.slot_capacity(int(n), bits) + 16 for n in lens], np.int64)
    bo = int(rng.integers(0, 16))
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + bo
    out = torch.full((int(out_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = rc.encode_batch_order1(o1, syms, dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    # nothing is written outside the slots
    assert (h[:bo] == SENT).all() and (h[out_off[-1]:] == SENT).all()
    return h, out_off, out_len.cpu().numpy(), flags.cpu().numpy()


def run_decode(o1, codes, counts, rng, pre=None):
    """Decode `codes` (at random gaps) into symbol ranges laid back to back behind `pre` stray
    bytes (default: a random number).  Returns (symbols per chunk, flags)."""
    n = len(codes)
    clen = np.array([len(c) for c in codes], np.int64)
    cstart, csize = layout(clen, rng, 16)
    code = arena([np.frombuffer(bytes(c), np.uint8) for c in codes], cstart, csize + 64, 0x5A)
    counts = np.asarray(counts, np.int64)
    pre = int(rng.integers(0, 64)) if pre is None else pre
    sym_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) + pre
    big = torch.full((int(sym_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 64 == 0
    flags = rc.decode_batch_order1(o1, code, dev(cstart), dev(clen), big, dev(sym_off))
    torch.cuda.synchronize()
    b = big.cpu().numpy()
    # nothing is written outside the chunks' symbol ranges
    assert (b[:sym_off[0]] == SENT).all() and (b[sym_off[-1]:] == SENT).all()
    return [b[sym_off[k]:sym_off[k + 1]] for k in range(n)], flags.cpu().numpy()


# ---------------------------------------------------------------- 1. byte parity
def parity_lens(P):
    return [0, 1, P - 1, P, P + 1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 300]


def parity_maps(rng, P, K, n):
    """A purely positional map (the row depends on the phase alone) and one drawn per (phase,
    previous symbol)."""
    pos = np.repeat(((np.arange(P) * 5 + 1) % K)[:, None], n, axis=1).astype(np.uint8)
    return {"positional": pos, "random": rng.integers(0, K, (P, n)).astype(np.uint8)}


PARITY_CASES = [(P, K, total, 256) for P in (2, 4, 8) for K in sorted({1, P, 8, 16, 64})
                for total in (65536, 40000)] + [(4, 4, 40000, 100)]
N_PARITY = 600


def parity_layout(P, K, total, n, which):
    """The chunk lengths of one parity launch and the stray bytes in front of the symbols and
    of the decoded symbols: a function of the case alone, so that what the layout covers can be
    checked without a device."""
    lay = np.random.default_rng([P, K, total, n, which])
    lens = lay.choice(parity_lens(P), N_PARITY)
    return lens, int(lay.integers(0, 64)), int(lay.integers(0, 64))


def check_layout(P, lens, pre):
    """Chunk starts on every residue mod 64, so byte-wise heads of 0 .. 63 symbols all occur;
    neighbouring lanes of the first wave mostly differ in head and in length; every length of
    the list occurs."""
    res = (pre + np.concatenate([[0], np.cumsum(lens)[:-1]])) % 64
    assert len(set(res.tolist())) == 64
    assert (np.diff(res[:64]) != 0).sum() >= 40 and (np.diff(lens[:64]) != 0).sum() >= 40
    assert set(lens.tolist()) == set(parity_lens(P))


@pytest.mark.parametrize("P,K,total,n", PARITY_CASES)
def test_parity_with_the_oracle(ctx, P, K, total, n):
    """One launch of 600 chunks per map: more than two 256-lane workgroups with a partly dead
    last wave, lengths around every seam, symbol starts (encoder heads) and output starts
    (decoder heads) on every residue mod 64, neighbouring lanes differing in head and length.
    Code bytes, lengths and flags equal the oracle's; decoding returns the symbols."""
    rng = np.random.default_rng([P, K, total, n])
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    first = int(rng.integers(0, K))
    for which, (kind, cm) in enumerate(parity_maps(rng, P, K, n).items()):
        o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=first, period=P)
        lens, pre_enc, pre_dec = parity_layout(P, K, total, n, which)
        check_layout(P, lens, pre_enc)
        check_layout(P, lens, pre_dec)
        chunks = [ref.draw_markov(rng, c, cm, first, int(L)) for L in lens]
        h, out_off, ol, fl = run_encode(o1, chunks, rng, pre_enc)
        codes = []
        for k, s in enumerate(chunks):
            f, b = ref.encode_ref(c, cum, total, cm, first, s)
            assert f == 0
            assert (int(fl[k]), int(ol[k])) == (0, len(b)), (kind, k, len(s), fl[k], ol[k], len(b))
            assert bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, (kind, k, len(s))
            codes.append(b)
        dec, fd = run_decode(o1, codes, [len(s) for s in chunks], rng, pre_dec)
        for k, s in enumerate(chunks):
            assert fd[k] == 0 and np.array_equal(dec[k], s), (kind, k, len(s))
        o1.close()


def test_parity_cases_cover_the_plans():
    """The cases reach both encoder layouts, both divisions, the 768-lane decoder and the
    512-lane encoder (no device needed, but the cases are this file's)."""
    seen = set()
    for P, K, total, _ in PARITY_CASES:
        out = (ctypes.c_uint32 * 8)()
        assert N.load().rc_model_order1_plan_periodic_(K, total, P, out) == N.RC_OK
        seen.add((out[2], total == 65536))
        if K == 64:
            assert (out[0], out[4]) == (512, 768)
    assert seen == {(0, True), (0, False), (1, True), (1, False)}


# ---------------------------------------------------------------- 2. the decoder against the
# oracle's stream decoder
@pytest.mark.parametrize("P,total", [(2, 65536), (4, 40000), (8, 65536)])
def test_decoder_against_the_stream_decoder(ctx, P, total):
    """Sound streams, garbage, all-0xFF and truncated streams of at most 200 symbols: the flags
    equal the reference's, and so do the symbols before the first flag."""
    rng = np.random.default_rng(200 + P)
    K, n = 8, 256
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    cm = rng.integers(0, K, (P, n)).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=3, period=P)
    codes, counts = [], []
    for L in (0, 1, P, P + 1, 17, 64, 65, 100, 129, 200):       # sound
        s = ref.draw_markov(rng, c, cm, 3, L)
        f, b = ref.encode_ref(c, cum, total, cm, 3, s)
        assert f == 0
        codes.append(b)
        counts.append(L)
    for _ in range(16):                                         # garbage
        codes.append(rng.integers(0, 256, int(rng.integers(8, 300))).astype(np.uint8).tobytes())
        counts.append(int(rng.integers(1, 201)))
    for L in (8, 9, 64, 250):                                   # all 0xFF
        codes.append(b"\xff" * L)
        counts.append(200)
    for cut in range(1, 9):                                     # truncated
        s = ref.draw_markov(rng, c, cm, 3, 200)
        f, b = ref.encode_ref(c, cum, total, cm, 3, s)
        codes.append(b[:len(b) - cut])
        counts.append(200)
    codes += [bytes(7), bytes(7)]
    counts += [10, 0]
    exp = [ref.decode_ref(c, cum, total, cm, 3, codes[k], counts[k]) for k in range(len(codes))]
    assert all(f == 0 for f, _ in exp[:10])
    assert [f for f, _ in exp[-2:]] == [N.F_TRUNCATED, N.F_TRUNCATED]
    dec, fd = run_decode(o1, codes, counts, rng)
    for k, (f, s) in enumerate(exp):
        assert int(fd[k]) == f, (k, len(codes[k]), fd[k], f)
        assert np.array_equal(dec[k][:len(s)], s), k


# ---------------------------------------------------------------- 3. encoder errors
def test_encode_flags_follow_the_phase(ctx):
    """n = 200, K = 4, P = 4, total 40000; symbol 50 has c = 0 in row 2 only; the row of symbol
    i > 0 is (i + sym[i-1]) & 3: the same pair of symbols is refused at one phase and coded at
    another, and the first error of a chunk is judged against that row."""
    rng = np.random.default_rng(77)
    n, K, P, total = 200, 4, 4, 40000
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        rows[j] += rng.multinomial(total - n, np.ones(n) / n)
    rows[2, 0] += rows[2, 50]
    rows[2, 50] = 0
    c, cum = tables(rows)
    cm = ((np.arange(P)[:, None] + np.arange(n)[None, :]) & 3).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=1, period=P)
    chunks = [ref.draw_markov(rng, c, cm, 1, 300) for _ in range(70)]  # 0 .. 63 share a wave

    def put(k, pos, *syms):
        chunks[k][pos:pos + len(syms)] = syms

    put(3, 101, 4, 50, 9)       # i = 102, after 4: row (2 + 4) & 3 = 2: ZERO_FREQ
    put(4, 102, 4, 50, 9)       # the same pair one position on: row 3, coded
    put(5, 101, 5, 50, 9)       # the same position after 5: row 3, coded
    put(6, 100, 6, 50, 9)       # i = 101, after 6: row (1 + 6) & 3 = 3, coded ...
    put(7, 103, 6, 50, 9)       # ... and at i = 104: row (0 + 6) & 3 = 2: ZERO_FREQ
    put(8, 0, 50)               # a chunk's first symbol (first_row 1): coded
    put(9, 1, 1, 50)            # i = 2 in the byte-wise head or the first block: row 3, coded
    put(9, 297, 1, 50)          # i = 298 in the tail: row (2 + 1) & 3 = 3, coded
    put(10, 296, 4, 50)         # i = 297 in the tail: row (1 + 4) & 3 = 1, coded
    put(11, 297, 4, 50)         # i = 298 in the tail: row (2 + 4) & 3 = 2: ZERO_FREQ
    for ph in range(4):         # a symbol >= n at positions with every phase
        put(12 + ph, 200 + ph, n)
        put(16 + ph, ph, 255)
        put(20 + ph, 296 + ph, n + 5)
    put(30, 49, 4, 50)          # two errors in one chunk: the first wins (i = 50: row 2)
    put(30, 200, n)
    put(31, 50, n + 1)
    put(31, 201, 4, 50)
    put(32, 7, n, 50)           # after a bad symbol (row 0 follows: 50 would pass there)
    exp = [ref.encode_ref(c, cum, total, cm, 1, s) for s in chunks]
    Z, B = N.F_ZERO_FREQ, N.F_BAD_SYMBOL
    assert [exp[k][0] for k in range(3, 12)] == [Z, 0, 0, 0, Z, 0, 0, 0, Z]
    assert [exp[k][0] for k in range(12, 24)] == [B] * 12
    assert [exp[k][0] for k in (30, 31, 32)] == [Z, B, B]
    for seed in (5, 6):  # two arenas: other heads, so the positions fall in other code paths
        h, out_off, ol, fl = run_encode(o1, chunks, np.random.default_rng(seed))
        for k, (f, b) in enumerate(exp):
            assert int(fl[k]) == f, (seed, k, fl[k], f)
            if f == 0:  # the neighbours of the flagged chunks stay clean and bit-exact
                assert int(ol[k]) == len(b) and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, k


# ---------------------------------------------------------------- 4. identity with the
# existing sets
def _created_by_the_new_call(o1, cm2d, P):
    """o1's Python object with a device snapshot made by rc_model_create_order1_set_periodic."""
    m = rc.Order1ModelSet(o1.c, o1.cum, o1.total, ctx_map=cm2d if P > 1 else cm2d[0],
                          first_row=o1.first_row, period=P)
    h = ctypes.c_void_p()
    cmap = np.ascontiguousarray(cm2d, np.uint8)
    N.check(m.ctx._lib.rc_model_create_order1_set_periodic(
        m.ctx.handle, m.n_models, m.n_symbols, ctypes.c_void_p(m.c.ctypes.data),
        ctypes.c_void_p(m.cum.ctypes.data), ctypes.c_uint32(m.total), ctypes.c_uint32(P),
        ctypes.c_void_p(cmap.ctypes.data), ctypes.c_uint32(m.first_row), ctypes.byref(h)),
        "rc_model_create_order1_set_periodic")
    m._handle = h
    return m


@pytest.mark.parametrize("P", [1, 4])
def test_identical_slices_code_what_the_old_set_codes(ctx, P):
    """A period-1 set from the new call, and a P = 4 set with four identical slices, against
    the set rc_model_create_order1_set makes: the same slots byte for byte, lengths, flags,
    decoded symbols and ideal bits, bad symbols included."""
    rng = np.random.default_rng(40 + P)
    K, n, total = 8, 200, 40000
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    cm = rng.integers(0, K, n).astype(np.uint8)
    old = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=2)
    new = _created_by_the_new_call(old, np.tile(cm, (P, 1)), P)
    lens = rng.choice(parity_lens(4) + [1000], 300)
    chunks = [ref.draw_markov(rng, c, cm[None], 2, int(L)) for L in lens]
    chunks[7] = ref.draw_markov(rng, c, cm[None], 2, 100)
    chunks[7][5] = n + 1  # a flagged chunk: the flags agree too
    got = [run_encode(m, chunks, np.random.default_rng(9)) for m in (old, new)]
    (h0, off0, ol0, fl0), (h1, off1, ol1, fl1) = got
    assert np.array_equal(ol0, ol1) and np.array_equal(fl0, fl1) and fl0[7] == N.F_BAD_SYMBOL
    assert int(np.abs(fl0).sum()) == N.F_BAD_SYMBOL
    codes = []
    for k in range(len(chunks)):
        if fl0[k] == 0:
            a = bytes(h0[off0[k]:off0[k] + ol0[k]])
            assert a == bytes(h1[off1[k]:off1[k] + ol1[k]]), k
            codes.append(a)
        else:
            codes.append(bytes(16))  # (decoded as an empty chunk)
    counts = [0 if fl0[k] else len(s) for k, s in enumerate(chunks)]
    d0, f0 = run_decode(old, codes, counts, np.random.default_rng(10))
    d1, f1 = run_decode(new, codes, counts, np.random.default_rng(10))
    assert np.array_equal(f0, f1) and int(np.abs(f0).sum()) == 0
    for k, s in enumerate(chunks):
        assert np.array_equal(d0[k], d1[k]), k
        assert fl0[k] or np.array_equal(d0[k], s), k
    sym_off = np.concatenate([[0], np.cumsum([len(s) for s in chunks])]).astype(np.int64)
    syms = dev(np.concatenate(chunks + [np.zeros(1, np.uint8)]))
    b0 = rc.ideal_bits_order1(old, syms, dev(sym_off))
    b1 = rc.ideal_bits_order1(new, syms, dev(sym_off))
    torch.cuda.synchronize()
    assert torch.equal(b0, b1) and bool(torch.isinf(b0[7])) and int(torch.isinf(b0).sum()) == 1


# ---------------------------------------------------------------- 5. rc_histogram_pairs_periodic
@pytest.mark.parametrize("P", [2, 4, 8])
def test_histogram_pairs_periodic_is_exact(ctx, P):
    """700 chunks (more than one grid round) of 0, 1, 15, 16, 17, 4096 and 4097 symbols, starts
    on every residue mod 16: exact against numpy, added into the arrays; either output may be
    null; the sum over the phases is rc_histogram_pairs' result."""
    rng = np.random.default_rng(500 + P)
    lens = np.array([0, 1, 15, 16, 17, 4096, 4097] * 100, np.int64)
    rng.shuffle(lens)
    chunks = [rng.integers(0, 256, int(L)).astype(np.uint8) for L in lens]
    for s in chunks[::3]:  # a skewed part, so that some counters run far ahead of the rest
        s[rng.random(len(s)) < 0.6] = 7
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + 3
    assert len(set((sym_off[:-1] % 16).tolist())) == 16
    syms = arena(chunks, sym_off[:-1], int(sym_off[-1]), 0xA5)
    want_pair, want_first = ref.pairs(chunks, P)
    base = rng.integers(0, 1000, (P, 256, 256)).astype(np.int64)
    pair, first = rc.histogram_pairs_periodic(syms, dev(sym_off), P, pair_hist=dev(base.copy()))
    torch.cuda.synchronize()
    assert np.array_equal(pair.cpu().numpy() - base, want_pair)
    assert np.array_equal(first.cpu().numpy(), want_first)
    assert int(want_pair.sum()) == int((lens - 1).clip(0).sum())
    # either output may be null
    lib, off = ctx._lib, dev(sym_off)
    p2 = torch.zeros((P, 256, 256), dtype=torch.int64, device="cuda")
    f2 = torch.zeros(256, dtype=torch.int64, device="cuda")
    ctx.bind_stream()
    assert lib.rc_histogram_pairs_periodic(ctx.handle, P, _p(syms), _p(off), len(lens), _p(p2),
                                           None) == N.RC_OK
    assert lib.rc_histogram_pairs_periodic(ctx.handle, P, _p(syms), _p(off), len(lens), None,
                                           _p(f2)) == N.RC_OK
    assert lib.rc_histogram_pairs_periodic(ctx.handle, P, _p(syms), _p(off), len(lens), None,
                                           None) == N.RC_OK
    assert lib.rc_histogram_pairs_periodic(ctx.handle, 3, _p(syms), _p(off), len(lens), _p(p2),
                                           _p(f2)) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(p2.cpu().numpy(), want_pair)
    assert np.array_equal(f2.cpu().numpy(), want_first)
    # the sum over the phases
    pair1, first1 = rc.histogram_pairs(syms, off)
    torch.cuda.synchronize()
    assert torch.equal(p2.sum(dim=0), pair1) and torch.equal(f2, first1)


# ---------------------------------------------------------------- 6. rc_ideal_bits_order1
@pytest.mark.parametrize("P", [2, 4, 8])
def test_ideal_bits_on_a_periodic_set(ctx, P):
    """Within 1e-12 relative of numpy (the chunks are far below the 5.7e5 symbols up to which
    the kernel's summation order keeps that bound), +inf where a term has c = 0, 0.0 for an
    empty chunk."""
    rng = np.random.default_rng(600 + P)
    K, n, total = 8, 256, 65536
    rows = markov_rows(rng, K, n, total, 1.0)
    rows[5, 0] += rows[5, 9]
    rows[5, 9] = 0                      # symbol 9 cannot be coded with row 5
    c, cum = tables(rows)
    cm = rng.integers(0, K, (P, n)).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=1, period=P)
    lens = [0, 1, P, 15, 16, 17, 100, 1000, 1024, 1025, 4097, 20000, 0, 33]
    chunks = []
    for L in lens:
        s = rng.integers(0, n, L).astype(np.uint8)
        s[s == 9] = 10                  # finite so far
        chunks.append(s)
    # one chunk with a zero-frequency term: symbol 9 where the phase and the previous symbol
    # pick row 5
    bad = chunks[8].copy()
    at = int(np.flatnonzero(ref.derive_idx(cm, 1, bad, n)[1:] == 5)[3]) + 1
    bad[at] = 9
    chunks.append(bad)
    want = np.array([ref.ideal_bits(c, total, cm, 1, s) for s in chunks])
    assert np.isinf(want[-1]) and np.isfinite(want[:-1]).all() and want[0] == 0.0
    sym_off = np.concatenate([[0], np.cumsum([len(s) for s in chunks])]).astype(np.int64) + 5
    syms = arena(chunks, sym_off[:-1], int(sym_off[-1]), 0)
    got = rc.ideal_bits_order1(o1, syms, dev(sym_off)).cpu().numpy()
    assert np.isinf(got[-1]) and got[-1] > 0 and got[0] == 0.0 and got[12] == 0.0
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    pos = fin & (want > 0)
    err = np.abs(got[pos] - want[pos]) / want[pos]
    print("ideal bits, relative error:", err.max())
    assert err.max() <= 1e-12


# ---------------------------------------------------------------- 7. refusals
def test_every_other_entry_point_refuses_a_period(ctx):
    rng = np.random.default_rng(70)
    K, n, total = 4, 256, 65536
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=rng.integers(0, K, (2, n)), period=2)
    lib, h = ctx._lib, o1.handle
    syms = torch.zeros(256, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(256, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 128, 256], dtype=torch.int64, device="cuda")
    off16 = torch.tensor([0, 64, 128], dtype=torch.int64, device="cuda")
    out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    out_off = torch.tensor([0, 2048, 4096], dtype=torch.int64, device="cuda")
    ol = torch.zeros(2, dtype=torch.int64, device="cuda")
    fl = torch.zeros(2, dtype=torch.int32, device="cuda")
    dst = torch.full((65536,), SENT, dtype=torch.uint8, device="cuda")
    n_out = ctypes.c_uint64()
    E = N.RC_E_ARG
    assert lib.rc_encode_batch(ctx.handle, h, _p(syms), _p(off), 2, _p(out), _p(out_off), _p(ol),
                               _p(fl)) == E
    assert lib.rc_decode_batch(ctx.handle, h, _p(out), _p(out_off), _p(ol), _p(syms), _p(off), 2,
                               _p(fl)) == E
    assert lib.rc_encode_batch_indexed(ctx.handle, h, _p(syms), _p(idx), _p(off), 2, _p(out),
                                       _p(out_off), _p(ol), _p(fl)) == E
    assert lib.rc_decode_batch_indexed(ctx.handle, h, _p(out), _p(out_off), _p(ol), _p(idx),
                                       _p(syms), _p(off), 2, _p(fl)) == E
    assert lib.rc_encode_batch_wide(ctx.handle, h, _p(syms), _p(off16), 2, _p(out), _p(out_off),
                                    _p(ol), _p(fl)) == E
    assert lib.rc_decode_batch_wide(ctx.handle, h, _p(out), _p(out_off), _p(ol), _p(syms),
                                    _p(off16), 2, _p(fl)) == E
    assert lib.rc_container_pack(ctx.handle, h, _p(out), _p(out_off), _p(ol), _p(off), 2, _p(dst),
                                 dst.numel(), ctypes.byref(n_out)) == E
    assert lib.rc_container2_pack(ctx.handle, h, _p(out), _p(out_off), _p(ol), _p(off), 2, None,
                                  _p(dst), dst.numel(), ctypes.byref(n_out)) == E
    assert lib.rc_container2_pack(ctx.handle, h, _p(out), _p(out_off), _p(ol), _p(off), 2, None,
                                  None, 0, ctypes.byref(n_out)) == E  # the size query too
    assert lib.rc_ideal_bits_wide(ctx.handle, h, _p(syms), _p(off16), 2, _p(ol)) == E
    hs = np.zeros(256, np.uint8)
    ho = np.array([0, 128, 256], np.uint64)
    for call in (rc.encode_host, lambda m, *a: rc.encode_host_multi([m], *a)):
        with pytest.raises(N.RCError) as e:
            call(o1, hs, ho, np.array([0, 2048, 4096], np.uint64))
        assert e.value.code == E
    with pytest.raises(ValueError, match="period"):
        rc.container.pack(o1, out, out_off, ol, off)
    with pytest.raises(ValueError, match="period"):
        rc.compress(syms, chunk_size=128, model=o1)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (dst.cpu().numpy() == SENT).all()
    # a period-1 set made by the same Python class is framed as before
    o1p1 = rc.Order1ModelSet(c, cum, total, ctx_map=rng.integers(0, K, n), period=1)
    blob = rc.compress(syms, chunk_size=128, model=o1p1)
    assert torch.equal(rc.decompress(blob), syms)


# ---------------------------------------------------------------- 8. the fit pays
def _records(kind):
    rng = np.random.default_rng(7)
    if kind == "float32":
        a = rng.standard_normal(1 << 16).astype(np.float32)
    else:
        a = rng.integers(0, 3000, 1 << 16).astype(np.int32)
    return a.view(np.uint8)


def _coded_bytes(o1, syms, sym_off, L):
    n = sym_off.numel() - 1
    cap = rc.slot_capacity(L, 17.0)
    out_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap
    out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    out_len, fl = rc.encode_batch_order1(o1, syms, sym_off, out, out_off)
    dec = torch.zeros_like(syms)
    fd = rc.decode_batch_order1(o1, out, out_off[:-1].contiguous(), out_len, dec, sym_off)
    torch.cuda.synchronize()
    assert int(fl.abs().sum()) == 0 and int(fd.abs().sum()) == 0
    assert torch.equal(dec, syms)  # the round trip is exact
    return int(out_len.sum())


@pytest.mark.parametrize("kind", ["float32", "int32"])
def test_the_periodic_fit_beats_the_unphased_fit(ctx, kind):
    """2^18 bytes of 4-byte records as 16-KiB chunks: 8 rows with the position in the record
    (two classes per phase) code them in strictly fewer bytes than 64 rows without it.  The
    empirical entropies (4 positional rows against a full 256-context order-1 model, which
    bounds any unphased set from below) leave 5.5 % of room on the floats and 16 % on the
    integers.  The periodic payload is within 2 % of its ideal bits."""
    L = 16384
    syms = dev(_records(kind))
    n = syms.numel() // L
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    per = rc.fit_order1_set(syms, sym_off, n_models=8, period=4)
    flat = rc.fit_order1_set(syms, sym_off, n_models=64)
    assert per.period == 4 and per.n_models <= 8 and per.ctx_map.shape == (4, 256)
    # the phases share no row: phase ph's rows follow those of the phases before it
    tops = [int(per.ctx_map[ph].max()) for ph in range(4)]
    lows = [int(per.ctx_map[ph].min()) for ph in range(4)]
    assert all(lows[ph] > tops[ph - 1] for ph in range(1, 4))
    b_per = _coded_bytes(per, syms, sym_off, L)
    b_flat = _coded_bytes(flat, syms, sym_off, L)
    ideal = float(rc.ideal_bits_order1(per, syms, sym_off).sum())
    print(f"{kind}: periodic {b_per} B, unphased {b_flat} B, ratio {b_per / b_flat:.4f}; "
          f"ideal bits {ideal:.0f}, payload / ideal {8 * b_per / ideal:.5f}")
    assert b_per < b_flat
    assert np.isfinite(ideal) and ideal <= 8 * b_per <= 1.02 * ideal
