"""Lagged order-1 sets on the GPU (rc_model_create_order1_set_lagged: the context is the symbol D
positions back) through rc_encode_batch_order1 / rc_decode_batch_order1, against the CPU oracle
(lag_ref.py) and against the periodic coders: byte parity with per-lane heads of every length
(heads shorter than the lag included), the decoder on sound and bad streams, encoder errors judged
with the lag, identity with the periodic sets at lag 1, rc_histogram_pairs_lagged,
rc_ideal_bits_order1, the fit and the refusals."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from gpu_helpers import dev  # noqa: E402
from order1_ref import markov_rows  # noqa: E402
import lag_ref as ref  # noqa: E402
import periodic_ref  # noqa: E402
from test_lag_model import bf16_bytes, walk_bytes  # noqa: E402

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


def run_decode(o1, codes, counts, rng, pre=None, guard=0):
    """Decode `codes` (at random gaps) into symbol ranges laid back to back behind `pre` stray
    bytes (default: a random number).  guard > 0: a range of that many guard bytes follows every
    chunk's; the batch calls take one offset array, so the guards are chunks too, of a stream of
    no bytes, which the decoder flags TRUNCATED before it writes anything.  Returns (symbols per
    chunk, flags) of the real chunks; nothing is written outside their symbol ranges."""
    n = len(codes)
    counts = [int(x) for x in counts]
    if guard:
        codes = [x for c in codes for x in (c, b"")]
        counts = [x for c in counts for x in (c, guard)]
    clen = np.array([len(c) for c in codes], np.int64)
    gaps = rng.integers(0, 16, len(clen))
    cstart = np.cumsum(gaps + np.concatenate([[0], clen[:-1]])).astype(np.int64)
    csize = int(cstart[-1] + clen[-1])
    code = arena([np.frombuffer(bytes(c), np.uint8) for c in codes], cstart, csize + 64, 0x5A)
    pre = int(rng.integers(0, 64)) if pre is None else pre
    sym_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) + pre
    big = torch.full((int(sym_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 64 == 0
    flags = rc.decode_batch_order1(o1, code, dev(cstart), dev(clen), big, dev(sym_off))
    torch.cuda.synchronize()
    b = big.cpu().numpy()
    fl = flags.cpu().numpy()
    assert (b[:sym_off[0]] == SENT).all() and (b[sym_off[-1]:] == SENT).all()
    step = 2 if guard else 1
    for k in range(1, len(codes), 2) if guard else ():
        assert fl[k] == N.F_TRUNCATED and (b[sym_off[k]:sym_off[k + 1]] == SENT).all(), k
    return [b[sym_off[k]:sym_off[k + 1]] for k in range(0, len(codes), step)], fl[::step]


# ---------------------------------------------------------------- 1. byte parity
def parity_lens(D):
    """n in {0, 1, D - 1, D, D + 1}, lengths around the block and tile seams, and longer ones:
    with a start on any residue mod 64 these end inside the head, leave full tiles, ragged waves
    and every tail."""
    return [0, 1, D - 1, D, D + 1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 140, 150,
            170, 200, 260, 300]


PARITY_CASES = [(D, P, K, total, 256) for D in (2, 4, 8) for P in sorted({1, D, 8})
                for K in (1, 8, 64) for total in (65536, 40000)] + [(4, 4, 4, 40000, 100)]
N_PARITY = 600


def parity_layout(D, P, K, total, n):
    """The chunk lengths of one parity launch and the stray bytes in front of the symbols and
    of the decoded symbols: a function of the case alone, so that what the layout covers can be
    checked without a device.  The lengths are drawn, long ones twice as often, until the layout
    covers what check_layout asks for (the first such draw of a fixed sequence)."""
    choice = parity_lens(D)
    w = np.array([2.0 if x >= 128 else 1.0 for x in choice])
    for attempt in range(200):
        lay = np.random.default_rng([D, P, K, total, n, attempt])
        lens = lay.choice(choice, N_PARITY, p=w / w.sum())
        pre_enc, pre_dec = int(lay.integers(0, 64)), int(lay.integers(0, 64))
        try:
            check_layout(D, lens, pre_enc)
            check_starts(lens, pre_dec)
        except AssertionError:
            continue
        return lens, pre_enc, pre_dec
    raise AssertionError("no layout covers the paths")


def encoder_paths(D, lens, pre):
    """Per chunk, where the lagged encoder codes it: (symbols up to the first 64-B boundary, the
    byte-wise head, tiles, tail).  Behind a head shorter than the lag the next 64 symbols are
    four blocks of their own in front of the tiles (counted as a tile here); with fewer than 64
    left the whole chunk is coded byte-wise."""
    start = pre + np.concatenate([[0], np.cumsum(lens)[:-1]])
    head0 = np.minimum((64 - start % 64) % 64, lens)
    head = np.where((head0 < D) & (lens - head0 < 64), lens, head0)
    tiles = (lens - head) // 64
    return head0, head, tiles, lens - head - 64 * tiles


def check_starts(lens, pre):
    """Starts on every residue mod 64, so heads of 0 .. 63 symbols all occur; neighbouring lanes
    of the first wave mostly differ in head and in length."""
    res = (pre + np.concatenate([[0], np.cumsum(lens)[:-1]])) % 64
    assert len(set(res.tolist())) == 64
    assert (np.diff(res[:64]) != 0).sum() >= 40 and (np.diff(lens[:64]) != 0).sum() >= 40
    return res


def check_layout(D, lens, pre):
    """check_starts, and for the encoder: every head shorter than the lag with tiles behind it;
    chunks that end inside their head; full tiles; waves whose lanes differ in their tile counts;
    tails of 1 .. 15 symbols; every length of the list occurs."""
    res = check_starts(lens, pre)
    assert set(lens.tolist()) == set(parity_lens(D))
    head0, head, tiles, tail = encoder_paths(D, lens, pre)
    for h in range(D):  # a head shorter than the lag: with tiles behind it, and without
        assert ((head0 == h) & (tiles > 0)).any() and ((head0 == h) & (lens >= D)).any(), h
    assert ((lens > 0) & (lens < (64 - res) % 64)).any()          # ends inside the head
    # (the tail loop is the same behind tiles and behind none)
    assert (tiles >= 2).any() and set(range(1, 16)) <= set(tail[lens > head].tolist())
    assert len(set(tail[tiles > 0].tolist()) & set(range(1, 16))) >= 8
    for w in range(0, len(lens), 64):                              # ragged waves
        assert len(set(tiles[w:w + 64].tolist())) >= 2, w


def test_parity_layouts_cover_the_paths():
    """No device needed, but the cases are this file's: every launch reaches every path."""
    for D, P, K, total, n in PARITY_CASES:
        lens, pre_enc, pre_dec = parity_layout(D, P, K, total, n)
        check_layout(D, lens, pre_enc)
        check_starts(lens, pre_dec)


@pytest.mark.parametrize("D,P,K,total,n", PARITY_CASES)
def test_parity_with_the_oracle(ctx, D, P, K, total, n):
    """One launch of 600 chunks with a random map: more than two 256-lane workgroups with a
    partly dead last wave, lengths around every seam, symbol starts (encoder heads) and output
    starts (decoder heads) on every residue mod 64, neighbouring lanes differing in head and
    length.  Code bytes, lengths and flags equal the oracle's; decoding returns the symbols."""
    rng = np.random.default_rng([D, P, K, total, n])
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    first = int(rng.integers(0, K))
    cm = rng.integers(0, K, (P, n)).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=first, period=P, lag=D)
    lens, pre_enc, pre_dec = parity_layout(D, P, K, total, n)
    chunks = [ref.draw_markov(rng, c, cm, first, int(L), D) for L in lens]
    h, out_off, ol, fl = run_encode(o1, chunks, rng, pre_enc)
    codes = []
    for k, s in enumerate(chunks):
        f, b = ref.encode_ref(c, cum, total, cm, first, s, D)
        assert f == 0
        assert (int(fl[k]), int(ol[k])) == (0, len(b)), (k, len(s), fl[k], ol[k], len(b))
        assert bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, (k, len(s))
        codes.append(b)
    dec, fd = run_decode(o1, codes, [len(s) for s in chunks], rng, pre_dec)
    for k, s in enumerate(chunks):
        assert fd[k] == 0 and np.array_equal(dec[k], s), (k, len(s))
    o1.close()


# ---------------------------------------------------------------- 2. the decoder against the
# oracle's stream decoder
@pytest.mark.parametrize("D,P,total", [(2, 2, 65536), (4, 1, 40000), (4, 8, 65536),
                                       (8, 8, 40000)])
def test_decoder_on_sound_and_bad_streams(ctx, D, P, total):
    """test_gpu_periodic's directed streams of at most 200 symbols with 64 guard bytes behind
    every output slot: sound streams decode to lag_ref.decode_ref's symbols; on garbage, all-0xFF
    and truncated streams the flags equal the reference's; nothing is written outside a slot."""
    rng = np.random.default_rng(200 + 10 * D + P)
    K, n = 8, 256
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    cm = rng.integers(0, K, (P, n)).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=3, period=P, lag=D)
    codes, counts = [], []
    for L in (0, 1, D - 1, D, D + 1, 17, 64, 65, 100, 129, 200):   # sound
        s = ref.draw_markov(rng, c, cm, 3, L, D)
        f, b = ref.encode_ref(c, cum, total, cm, 3, s, D)
        assert f == 0
        codes.append(b)
        counts.append(L)
    n_sound = len(codes)
    for _ in range(16):                                         # garbage
        codes.append(rng.integers(0, 256, int(rng.integers(8, 300))).astype(np.uint8).tobytes())
        counts.append(int(rng.integers(1, 201)))
    for L in (8, 9, 64, 250):                                   # all 0xFF
        codes.append(b"\xff" * L)
        counts.append(200)
    for cut in range(1, 9):                                     # truncated
        s = ref.draw_markov(rng, c, cm, 3, 200, D)
        f, b = ref.encode_ref(c, cum, total, cm, 3, s, D)
        codes.append(b[:len(b) - cut])
        counts.append(200)
    codes += [bytes(7), bytes(7)]
    counts += [10, 0]
    exp = [ref.decode_ref(c, cum, total, cm, 3, codes[k], counts[k], D)
           for k in range(len(codes))]
    assert all(f == 0 for f, _ in exp[:n_sound])
    assert [f for f, _ in exp[-2:]] == [N.F_TRUNCATED, N.F_TRUNCATED]
    for seed in (1, 2):  # two arenas: other output heads
        dec, fd = run_decode(o1, codes, counts, np.random.default_rng(seed), guard=64)
        for k, (f, s) in enumerate(exp):
            assert int(fd[k]) == f, (seed, k, len(codes[k]), fd[k], f)
            if k < n_sound:
                assert np.array_equal(dec[k], s), (seed, k)


# ---------------------------------------------------------------- 3. encoder errors
def test_encode_flags_follow_the_lag(ctx):
    """n = 200, K = 4, P = 4, D = 4, total 40000; symbol 50 has c = 0 in row 2 only; the row of
    symbol i >= 4 is (i + sym[i-4]) & 3.  Symbol 50 is refused where the symbol four back picks
    row 2 (and the symbol before would pick row 3) and coded where the symbol four back picks row
    3 (and the symbol before would pick row 2): in the byte-wise head, at a block position below
    the lag, at one from the lag on, in the tail and in the blocks behind a head shorter than the
    lag, each place found from the chunk's own start in the arena.  A symbol >= n is
    refused wherever it stands, and the first error of a chunk wins."""
    rng = np.random.default_rng(77)
    n, K, P, D, total = 200, 4, 4, 4, 40000
    rows = np.ones((K, n), np.int64)
    for j in range(K):
        rows[j] += rng.multinomial(total - n, np.ones(n) / n)
    rows[2, 0] += rows[2, 50]
    rows[2, 50] = 0
    c, cum = tables(rows)
    cm = ((np.arange(P)[:, None] + np.arange(n)[None, :]) & 3).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=1, period=P, lag=D)
    L, pre = 300, 5
    Z, B = N.F_ZERO_FREQ, N.F_BAD_SYMBOL
    chunks = []
    for _ in range(70):  # 0 .. 63 share a wave
        s = ref.draw_markov(rng, c, cm, 1, L, D)
        s[s == 50] = 51  # (c > 0 in every row: clean until an error is planted)
        chunks.append(s)
    head0, head, tiles, tail = encoder_paths(D, np.full(len(chunks), L), pre)
    assert (tiles >= 2).all()
    # where each kind of place lies in chunk k (None: the chunk has no such place)
    kinds = {
        "head": lambda k: int(head[k]) - 1 if head0[k] >= 2 * D else None,
        "block below the lag": lambda k: int(head[k]) + 16 * 3 + 2,
        "block from the lag on": lambda k: int(head[k]) + 16 * 2 + 9,
        "tail": lambda k: L - 1 if tail[k] >= 1 else None,
        "second block behind a short head": lambda k: int(head0[k]) + 17 if head0[k] < D else None,
    }
    want, used = {}, set()

    def take(kind):
        for k in range(3, len(chunks)):
            if k not in used and kinds[kind](k) is not None:
                used.add(k)
                return k, kinds[kind](k)
        raise AssertionError(kind)

    def plant(k, i, far_row, near_row):
        """Symbol 50 at position i of chunk k; the symbol D before it picks far_row for it, the
        symbol before it would pick near_row."""
        s = chunks[k]
        s[i - D] = 4 + ((far_row - i) & 3)
        s[i - 1] = 8 + ((near_row - i) & 3)
        s[i] = 50

    for kind in kinds:
        k, i = take(kind)
        plant(k, i, 2, 3)        # refused by the lagged row alone
        want[k] = Z
        k, i = take(kind)
        plant(k, i, 3, 2)        # coded: only the lag-1 row would refuse it
        want[k] = 0
        k, i = take(kind)
        chunks[k][i] = n         # a symbol past the alphabet
        want[k] = B
    k, i = take("block from the lag on")   # two errors in one chunk: the first wins
    plant(k, i, 2, 3)
    chunks[k][i + 40] = n + 1
    want[k] = Z
    k, i = take("block below the lag")
    chunks[k][i - 30] = 255
    plant(k, i, 2, 3)
    want[k] = B
    k, i = take("tail")                    # row 0 follows a bad symbol D later: 50 passes there
    chunks[k][i - D] = n
    chunks[k][i] = 50
    want[k] = B
    chunks[0][:D] = 50                     # a chunk's first D symbols (first_row 1): coded
    want[0] = 0
    chunks[1][D] = 50                      # the first lagged symbol: (4 + s[0]) & 3
    chunks[1][0] = 6                       # row 2: refused
    want[1] = Z
    exp = [ref.encode_ref(c, cum, total, cm, 1, s, D) for s in chunks]
    for k, f in want.items():
        assert exp[k][0] == f, (k, exp[k][0], f)
    assert all(exp[k][0] == 0 for k in range(len(chunks)) if k not in want)
    for seed, pre_ in ((5, pre), (6, None)):  # the second arena: other heads, other code paths
        h, out_off, ol, fl = run_encode(o1, chunks, np.random.default_rng(seed), pre_)
        for k, (f, b) in enumerate(exp):
            assert int(fl[k]) == f, (seed, k, fl[k], f)
            if f == 0:  # the neighbours of the flagged chunks stay clean and bit-exact
                assert int(ol[k]) == len(b) and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, k


# ---------------------------------------------------------------- 4. identity at lag 1
def _created_by_the_lagged_call(o1, lag):
    """o1's Python object with a device snapshot made by rc_model_create_order1_set_lagged."""
    m = rc.Order1ModelSet(o1.c, o1.cum, o1.total, ctx_map=o1.ctx_map, first_row=o1.first_row,
                          period=o1.period, lag=lag)
    h = ctypes.c_void_p()
    N.check(m.ctx._lib.rc_model_create_order1_set_lagged(
        m.ctx.handle, m.n_models, m.n_symbols, ctypes.c_void_p(m.c.ctypes.data),
        ctypes.c_void_p(m.cum.ctypes.data), ctypes.c_uint32(m.total), ctypes.c_uint32(m.period),
        ctypes.c_uint32(lag), ctypes.c_void_p(m.ctx_map.ctypes.data),
        ctypes.c_uint32(m.first_row), ctypes.byref(h)), "rc_model_create_order1_set_lagged")
    m._handle = h
    return m


@pytest.mark.parametrize("P", [1, 4])
def test_lag_1_is_the_periodic_set(ctx, P):
    """A set from the lagged call at lag 1 against the set of the periodic call: the same slots
    byte for byte, lengths, flags, decoded symbols, ideal bits and pair counts, a bad symbol
    included."""
    rng = np.random.default_rng(40 + P)
    K, n, total = 8, 200, 40000
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    cm = rng.integers(0, K, (P, n)).astype(np.uint8)
    old = rc.Order1ModelSet(c, cum, total, ctx_map=cm if P > 1 else cm[0], first_row=2, period=P)
    new = _created_by_the_lagged_call(old, 1)
    lens = rng.choice(parity_lens(4) + [1000], 300)
    chunks = [periodic_ref.draw_markov(rng, c, cm, 2, int(L)) for L in lens]
    chunks[7] = periodic_ref.draw_markov(rng, c, cm, 2, 100)
    chunks[7][5] = n + 1  # a flagged chunk: the flags agree too
    got = [run_encode(m, chunks, np.random.default_rng(9)) for m in (old, new)]
    (h0, off0, ol0, fl0), (h1, off1, ol1, fl1) = got
    assert np.array_equal(ol0, ol1) and np.array_equal(fl0, fl1) and fl0[7] == N.F_BAD_SYMBOL
    assert int(np.abs(fl0).sum()) == N.F_BAD_SYMBOL and np.array_equal(off0, off1)
    assert np.array_equal(h0, h1)  # the whole arena, slots and sentinels
    codes = [bytes(h0[off0[k]:off0[k] + ol0[k]]) if fl0[k] == 0 else bytes(16)
             for k in range(len(chunks))]
    counts = [0 if fl0[k] else len(s) for k, s in enumerate(chunks)]
    d0, f0 = run_decode(old, codes, counts, np.random.default_rng(10))
    d1, f1 = run_decode(new, codes, counts, np.random.default_rng(10))
    assert np.array_equal(f0, f1) and int(np.abs(f0).sum()) == 0
    for k, s in enumerate(chunks):
        assert np.array_equal(d0[k], d1[k]), k
        assert fl0[k] or np.array_equal(d0[k], s), k
    sym_off = np.concatenate([[0], np.cumsum([len(s) for s in chunks])]).astype(np.int64)
    syms = dev(np.concatenate(chunks + [np.zeros(1, np.uint8)]))
    off = dev(sym_off)
    b0 = rc.ideal_bits_order1(old, syms, off)
    b1 = rc.ideal_bits_order1(new, syms, off)
    torch.cuda.synchronize()
    assert torch.equal(b0, b1) and bool(torch.isinf(b0[7])) and int(torch.isinf(b0).sum()) == 1
    pa, fa = rc.histogram_pairs_periodic(syms, off, P)
    pb, fb = rc.histogram_pairs_periodic(syms, off, P, lag=1)
    pc = torch.zeros_like(pa)
    fc = torch.zeros_like(fa)
    ctx.bind_stream()
    assert ctx._lib.rc_histogram_pairs_lagged(ctx.handle, P, 1, _p(syms), _p(off), len(chunks),
                                              _p(pc), _p(fc)) == N.RC_OK
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(pa, pc) and torch.equal(fa, fb)
    assert torch.equal(fa, fc)


# ---------------------------------------------------------------- 5. the counts
@pytest.mark.parametrize("D,P", [(2, 1), (2, 2), (4, 4), (4, 8), (8, 2), (8, 8)])
def test_histogram_pairs_lagged_is_exact(ctx, D, P):
    """700 chunks (more than one grid round) of 0, 1, D - 1, D, D + 1, 15, 16, 17, 4096 and 4097
    symbols, starts on every residue mod 16: exact against numpy, added into the arrays; either
    output may be null; pair and first together count every symbol."""
    rng = np.random.default_rng(500 + 10 * D + P)
    lens = np.array([0, 1, D - 1, D, D + 1, 15, 16, 17, 4096, 4097] * 70, np.int64)
    rng.shuffle(lens)
    chunks = [rng.integers(0, 256, int(L)).astype(np.uint8) for L in lens]
    for s in chunks[::3]:  # a skewed part, so that some counters run far ahead of the rest
        s[rng.random(len(s)) < 0.6] = 7
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + 3
    assert len(set((sym_off[:-1] % 16).tolist())) == 16
    syms = arena(chunks, sym_off[:-1], int(sym_off[-1]), 0xA5)
    want_pair, want_first = ref.pairs(chunks, P, D)
    assert int(want_pair.sum() + want_first.sum()) == int(lens.sum())
    assert int(want_first.sum()) == int(np.minimum(lens, D).sum())
    base = rng.integers(0, 1000, (P, 256, 256)).astype(np.int64)
    pair, first = rc.histogram_pairs_periodic(syms, dev(sym_off), P, pair_hist=dev(base.copy()),
                                              lag=D)
    torch.cuda.synchronize()
    assert np.array_equal(pair.cpu().numpy() - base, want_pair)
    assert np.array_equal(first.cpu().numpy(), want_first)
    assert int((pair.cpu().numpy() - base).sum() + first.sum()) == int(lens.sum())
    # either output may be null
    lib, off = ctx._lib, dev(sym_off)
    p2 = torch.zeros((P, 256, 256), dtype=torch.int64, device="cuda")
    f2 = torch.zeros(256, dtype=torch.int64, device="cuda")
    ctx.bind_stream()
    call = lib.rc_histogram_pairs_lagged
    assert call(ctx.handle, P, D, _p(syms), _p(off), len(lens), _p(p2), None) == N.RC_OK
    assert call(ctx.handle, P, D, _p(syms), _p(off), len(lens), None, _p(f2)) == N.RC_OK
    assert call(ctx.handle, P, D, _p(syms), _p(off), len(lens), None, None) == N.RC_OK
    assert call(ctx.handle, P, 3, _p(syms), _p(off), len(lens), _p(p2), _p(f2)) == N.RC_E_ARG
    assert call(ctx.handle, 3, D, _p(syms), _p(off), len(lens), _p(p2), _p(f2)) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(p2.cpu().numpy(), want_pair)
    assert np.array_equal(f2.cpu().numpy(), want_first)


@pytest.mark.parametrize("D,P", [(2, 2), (4, 1), (4, 4), (8, 4)])
def test_ideal_bits_on_a_lagged_set(ctx, D, P):
    """Within 1e-12 relative of numpy (the chunks are far below the 5.7e5 symbols up to which
    the kernel's summation order keeps that bound), +inf where a term has c = 0, 0.0 for an
    empty chunk."""
    rng = np.random.default_rng(600 + 10 * D + P)
    K, n, total = 8, 256, 65536
    rows = markov_rows(rng, K, n, total, 1.0)
    rows[5, 0] += rows[5, 9]
    rows[5, 9] = 0                      # symbol 9 cannot be coded with row 5
    c, cum = tables(rows)
    cm = rng.integers(0, K, (P, n)).astype(np.uint8)
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=cm, first_row=1, period=P, lag=D)
    lens = [0, 1, D - 1, D, D + 1, 15, 16, 17, 100, 1000, 1024, 1025, 4097, 20000, 0, 33]
    chunks = []
    for L in lens:
        s = rng.integers(0, n, L).astype(np.uint8)
        s[s == 9] = 10                  # finite so far
        chunks.append(s)
    # one chunk with a zero-frequency term: symbol 9 where the phase and the symbol D before
    # pick row 5
    bad = chunks[9].copy()
    at = int(np.flatnonzero(ref.derive_idx(cm, 1, bad, n, D)[D:] == 5)[3]) + D
    bad[at] = 9
    chunks.append(bad)
    want = np.array([ref.ideal_bits(c, total, cm, 1, s, D) for s in chunks])
    assert np.isinf(want[-1]) and np.isfinite(want[:-1]).all() and want[0] == 0.0
    sym_off = np.concatenate([[0], np.cumsum([len(s) for s in chunks])]).astype(np.int64) + 5
    syms = arena(chunks, sym_off[:-1], int(sym_off[-1]), 0)
    got = rc.ideal_bits_order1(o1, syms, dev(sym_off)).cpu().numpy()
    assert np.isinf(got[-1]) and got[-1] > 0 and got[0] == 0.0 and got[14] == 0.0
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    pos = fin & (want > 0)
    err = np.abs(got[pos] - want[pos]) / want[pos]
    print("ideal bits, relative error:", err.max())
    assert err.max() <= 1e-12


# ---------------------------------------------------------------- 6. the fit
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


@pytest.mark.parametrize("source,P", [(walk_bytes, 4), (bf16_bytes, 2)])
def test_the_lagged_fit_beats_the_lag_1_fit(ctx, source, P):
    """2^18 bytes of P-byte records as 16-KiB chunks, K = 8 rows shared by the phases: the set
    fitted at lag P round-trips, stays within 2 % of its own ideal bits and codes strictly fewer
    bytes than the set fitted at lag 1 with the same K and P (the fitted costs of the two differ
    by 17 %, test_lag_model.py)."""
    L = 16384
    syms = dev(source())
    n = syms.numel() // L
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    far = rc.fit_order1_set(syms, sym_off, n_models=8, period=P, lag=P, joint=True)
    near = rc.fit_order1_set(syms, sym_off, n_models=8, period=P, lag=1, joint=True)
    assert (far.period, far.lag, near.period, near.lag) == (P, P, P, 1)
    assert far.n_models <= 8 and far.ctx_map.shape == (P, 256)
    b_far = _coded_bytes(far, syms, sym_off, L)
    b_near = _coded_bytes(near, syms, sym_off, L)
    ideal = float(rc.ideal_bits_order1(far, syms, sym_off).sum())
    print(f"{source.__name__}: lag {P} {b_far} B, lag 1 {b_near} B, ratio {b_far / b_near:.4f}; "
          f"ideal bits {ideal:.0f}, payload / ideal {8 * b_far / ideal:.5f}")
    assert b_far < b_near
    assert np.isfinite(ideal) and ideal <= 8 * b_far <= 1.02 * ideal
    # the fit without `joint` takes the lag too
    per_phase = rc.fit_order1_set(syms, sym_off, n_models=8, period=P, lag=P)
    assert (per_phase.period, per_phase.lag) == (P, P)
    _coded_bytes(per_phase, syms, sym_off, L)  # (round-trips)


# ---------------------------------------------------------------- 7. refusals
def test_every_other_entry_point_refuses_a_lag(ctx):
    rng = np.random.default_rng(70)
    K, n, total = 4, 256, 65536
    c, cum = tables(markov_rows(rng, K, n, total, 1.0))
    o1 = rc.Order1ModelSet(c, cum, total, ctx_map=rng.integers(0, K, n), lag=2)  # period 1
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
    with pytest.raises(ValueError, match="lag"):
        rc.container.pack(o1, out, out_off, ol, off)
    with pytest.raises(ValueError, match="lag"):
        rc.compress(syms, chunk_size=128, model=o1)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (dst.cpu().numpy() == SENT).all()
    # a lag-1 set made by the same Python class is framed as before
    o1l1 = rc.Order1ModelSet(c, cum, total, ctx_map=rng.integers(0, K, n), lag=1)
    blob = rc.compress(syms, chunk_size=128, model=o1l1)
    assert torch.equal(rc.decompress(blob), syms)
