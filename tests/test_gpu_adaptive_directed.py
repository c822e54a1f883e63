"""Directed GPU tests of the adaptive order-0 coder (rc_adaptive.hip): k_encode_adaptive and the
three k_decode_adaptive instantiations through the C ABI against the C oracle, byte for byte
(bytes, out_len, flags, decoded symbols; no tolerances).

  a. the steered fixtures (tests/golden/adaptive_fixtures.json: range_reduction_expansion
     mid-stream, halvings) at all 16 symbol-buffer and decoded-buffer alignments;
  b. the decoder's uniform-head path, dec_tiles<true>, at heads 0, 15, 9 and 1 and periods 1-256;
  c. wave shapes: T = 0..9 steps of the two-wave encoder, block look-ahead at the chunk's last
     block, several workgroups, a partly dead last one, launches of empty chunks;
  d. garbage, saturated and truncated streams on every decoder variant;
  e. the encoder's slow path: a bad symbol in every FIFO slot, slots below their need.

Which branch an input reaches is proved on the CPU, in tests/test_adaptive_ref.py, for the same
inputs (tests/adaptive_cases.py); the layout properties the cases rely on (alignments, equal
heads, step counts) are computed from the layouts and asserted here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import dev  # noqa: E402
import adaptive_cases as ac  # noqa: E402

DEV = "cuda"
SENT = 0xEE
SET_A, SET_C = ac.SETS["A"][0], ac.SETS["C"][0]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return ac.load_fixtures(golden_dir)[1]


# ---- the oracle, computed once per (parameters, chunk) and shared by every test ----
_ENC = {}


def orc(params, syms):
    """(flag, code, out_len) of cpu.encode_adaptive for a slot that is large enough."""
    key = (tuple(params), bytes(syms))
    if key not in _ENC:
        _ENC[key] = cpu.encode_adaptive(*params, np.asarray(syms, np.uint8))
    return _ENC[key]


def model(ctx, params):
    return rc.AdaptiveModel(*params, ctx=ctx)


# ---- launches with every offset chosen by the caller ----
def encode_at(m, chunks, caps, base_s=0, base_o=0):
    """One encode launch: chunk k at symbol offset base_s + (lengths before it), its slot at
    base_o + (capacities before it).  Returns (out bytes, sym_off, out_off, out_len, flags);
    the bytes before the first slot and after the last must still hold the sentinel."""
    lens = np.array([len(c) for c in chunks], np.int64)
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + base_s
    syms = np.concatenate([np.full(base_s, 0xA5, np.uint8)] +
                          [np.asarray(c, np.uint8) for c in chunks] + [np.zeros(16, np.uint8)])
    out_off = np.concatenate([[0], np.cumsum(np.asarray(caps, np.int64))]).astype(np.int64) + base_o
    d_syms = dev(syms)
    out = torch.full((int(out_off[-1]) + 64,), SENT, dtype=torch.uint8, device=DEV)
    # offsets are alignments only if both buffers start on a 16-B boundary
    assert d_syms.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    out_len, flags = rc.encode_batch(m, d_syms, dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:base_o] == SENT).all() and (h[out_off[-1]:] == SENT).all()
    return h, sym_off, out_off, out_len.cpu().numpy(), flags.cpu().numpy()


def decode_at(m, codes, counts, base=0, seed=0):
    """One decode launch: code k after a gap of 0..15 random bytes (so at an arbitrary byte
    alignment), chunk k's symbols at base + (counts before it).  Returns (decoded buffer,
    sym_off, flags); the bytes before the first chunk and the 16 after the last must still hold
    the sentinel."""
    rng = np.random.default_rng(seed)
    parts, coff, pos = [], [], 0
    for c in codes:
        gap = int(rng.integers(0, 16))
        parts.append(rng.integers(0, 256, gap).astype(np.uint8))
        coff.append(pos + gap)
        parts.append(np.frombuffer(bytes(c), np.uint8))
        pos += gap + len(c)
    parts.append(np.zeros(16, np.uint8))
    clen = np.array([len(c) for c in codes], np.int64)
    sym_off = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64) + base
    blob = dev(np.concatenate(parts))
    syms = torch.full((int(sym_off[-1]) + 16,), SENT, dtype=torch.uint8, device=DEV)
    assert blob.data_ptr() % 16 == 0 and syms.data_ptr() % 16 == 0
    flags = rc.decode_batch(m, blob, dev(np.array(coff, np.int64)), dev(clen), syms, dev(sym_off))
    torch.cuda.synchronize()
    s = syms.cpu().numpy()
    assert (s[:base] == SENT).all() and (s[sym_off[-1]:] == SENT).all()
    return s, sym_off, flags.cpu().numpy()


def check_encode(m, params, chunks, base_s=0, base_o=0, extra=0):
    """Every chunk of one launch against the oracle; slot k has room to spare plus
    (extra * k) % 13 bytes, so with extra the slots start at every alignment.  Returns the
    symbol offsets."""
    caps = [rc.slot_capacity(len(c), 16) + (extra * k) % 13 for k, c in enumerate(chunks)]
    h, sym_off, out_off, ol, fl = encode_at(m, chunks, caps, base_s, base_o)
    for k, c in enumerate(chunks):
        f, want, L = orc(params, c)
        assert f == 0 and fl[k] == 0 and ol[k] == L, (k, len(c), fl[k], ol[k], L)
        assert bytes(h[out_off[k]:out_off[k] + L]) == want, f"chunk {k} (len {len(c)})"
    return sym_off


def check_decode(m, params, chunks, base=0, seed=0):
    """The oracle's codes of the chunks decode to the chunks.  Returns the symbol offsets."""
    codes = [orc(params, c)[1] for c in chunks]
    s, sym_off, fd = decode_at(m, codes, [len(c) for c in chunks], base, seed)
    assert (fd == 0).all(), np.flatnonzero(fd)
    for k, c in enumerate(chunks):
        assert bytes(s[sym_off[k]:sym_off[k + 1]]) == bytes(c), f"chunk {k} (len {len(c)})"
    return sym_off


def heads(sym_off):
    """Per chunk, the symbols k_decode_adaptive decodes singly before its output is 16-B
    aligned: min((16 - address) & 15, n)."""
    off, n = sym_off[:-1], np.diff(sym_off)
    return np.minimum((16 - off) & 15, n)


def steps(lens):
    """k_encode_adaptive's step count T of one workgroup: wave_max((n + 7) >> 3)."""
    return max((int(L) + 7) >> 3 for L in lens) if len(lens) else 0


def test_params_in_step():
    import test_gpu_adaptive
    assert ac.PARAMS == test_gpu_adaptive.PARAMS and ac.C4 == test_gpu_adaptive.C4


# ------------------------------------------------------------------------------------------
# a. fixtures at every phase
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.SETS))
def test_fixtures_at_every_alignment(ctx, fixtures, name):
    """Each fixture chunk 16 times in one launch, behind padding chunks sized so that its
    symbols start at every offset mod 16: on encode that is the model wave's mis (funnel4), on
    decode head lengths 0..15, so every rare_at and halve_at index lands on every tile phase and
    in head, tiles and tail, on the non-uniform path.  Slots and codes start at arbitrary
    alignments.  The padding chunks are checked like the rest."""
    params = fixtures[name]["params"]
    rng = np.random.default_rng(ord(name))
    m = model(ctx, params)
    chunks, copies, pos = [], {}, 0
    for fi, fc in enumerate(fixtures[name]["chunks"]):
        for r in range(16):
            pad = (r - pos) % 16 + 16 * ((r + fi) % 3)
            chunks.append(ac.zipf_syms(rng, params[0], pad, s=float(rng.uniform(0.0, 1.6))))
            copies.setdefault(fi, []).append(len(chunks))
            chunks.append(fc["symbols"])
            pos += pad + len(fc["symbols"])
    assert len(chunks) <= 192
    for base_o in (0, 5):
        sym_off = check_encode(m, params, chunks, base_o=base_o, extra=5)
        for fi, ks in copies.items():
            assert sorted(int(sym_off[k]) % 16 for k in ks) == list(range(16))
    sym_off = check_decode(m, params, chunks, seed=ord(name))
    hd = heads(sym_off)
    for fi, ks in copies.items():
        assert sorted(int(hd[k]) for k in ks) == list(range(16))
    for g in range(0, len(chunks), 64):  # every workgroup takes dec_tiles<false>
        assert hd[g:g + 64].min() < hd[g:g + 64].max()


# ------------------------------------------------------------------------------------------
# b. uniform-head decode
# ------------------------------------------------------------------------------------------
UNIFORM_PARAMS = [p for p in ac.PARAMS if p[3] in (1, 4, 8, 16, 256)] + [ac.SETS["B"][0]]


@pytest.mark.parametrize("params", UNIFORM_PARAMS)
def test_uniform_head_decode(ctx, fixtures, params):
    """64 and 70 chunks whose lengths are multiples of 16 (16..400, and the fixture chunks of
    these parameters cut to a multiple of 16), decoded into a buffer that starts at offset b:
    every lane has head (16 - b) & 15, which selects dec_tiles<true> with its period ends at
    ((head + 16 t + j) & pmask) == pmask, and lanes finish at different tiles and run along."""
    assert {p[3] for p in UNIFORM_PARAMS} == {1, 4, 8, 16, 256}
    n = params[0]
    rng = np.random.default_rng(n * 31 + params[1])
    m = model(ctx, params)
    chunks = [ac.zipf_syms(rng, n, 16 * int(rng.integers(1, 26)), s=float(rng.uniform(0.0, 1.6)))
              for _ in range(70)]
    cuts = [fc["symbols"][:len(fc["symbols"]) & ~15]
            for s in fixtures.values() if s["params"] == params for fc in s["chunks"]]
    for j, c in enumerate(cuts):
        chunks[5 + 13 * j] = c
    for count in (64, 70):
        part = chunks[:count]
        tiles = {len(c) // 16 for c in part}
        assert len(tiles) > 8  # mixed tile counts
        for b in (0, 1, 7, 15):
            sym_off = check_decode(m, params, part, base=b, seed=b)
            hd = heads(sym_off)
            assert (hd == (16 - b) & 15).all()


# ------------------------------------------------------------------------------------------
# c. wave shapes
# ------------------------------------------------------------------------------------------
# 0..40 give T = 0..5 and 63..73 give T = 8..10; 41, 48, 49 and 56 add T = 6 and 7, so that every
# T of 0..9 is run
SHAPE_LENS = list(range(41)) + [41, 48, 49, 56] + [63, 64, 65, 71, 72, 73]
SHAPE_PARAMS = [SET_A, SET_C, (17, 5, 1000, 4)]


@pytest.mark.parametrize("params", SHAPE_PARAMS)
def test_short_chunks_every_step_count(ctx, params):
    """One chunk of length L, and 64 chunks all of length L, per launch: T = 0..9 steps (and up
    to 10) of the encoder's shared barrier sequence, with both parities of its unrolled loops,
    and the decoder's head-only, one-tile and tail-only shapes."""
    n = params[0]
    rng = np.random.default_rng(n + 77)
    m = model(ctx, params)
    seen = set()
    for L in SHAPE_LENS:
        for count in (1, 64):
            chunks = [ac.zipf_syms(rng, n, L, s=float(rng.uniform(0.0, 1.6)))
                      for _ in range(count)]
            assert steps([len(c) for c in chunks]) == (L + 7) >> 3
            seen.add((count, (L + 7) >> 3))
            check_encode(m, params, chunks)
            check_decode(m, params, chunks, seed=L)
    for count in (1, 64):
        assert {t for c, t in seen if c == count} >= set(range(10))


def test_block_lookahead_at_the_last_block(ctx):
    """One chunk of n = 256, C4, at each symbol alignment 0..15 and lengths around one and two
    16-B blocks: the model wave's look-ahead loads, clamped at the chunk's last block (blast)."""
    m = model(ctx, SET_A)
    rng = np.random.default_rng(16)
    blast = set()
    for L in (1, 15, 16, 17, 33):
        for al in range(16):
            chunk = ac.zipf_syms(rng, 256, L, s=0.5)
            sym_off = check_encode(m, SET_A, [chunk], base_s=al)
            assert sym_off[0] % 16 == al
            blast.add((L, (al + L - 1) >> 4))
            check_decode(m, SET_A, [chunk], base=al, seed=al)
    # (length, last block): the last block is 0, 1 or 2, at or below the blocks 1, 2 and 3 that
    # the look-ahead asks for; lengths 15 and 16 end in block 0 or 1, depending on the alignment
    assert blast == {(1, 0), (15, 0), (15, 1), (16, 0), (16, 1), (17, 1), (33, 2)}


@pytest.mark.parametrize("params", SHAPE_PARAMS)
def test_ragged_workgroups(ctx, params):
    """65, 130 and 191 ragged chunks of 0..300 symbols: a second and a third workgroup, and a
    last one with dead lanes beside full ones, every chunk against the oracle."""
    n = params[0]
    rng = np.random.default_rng(n + 191)
    m = model(ctx, params)
    for count in (65, 130, 191):
        lens = rng.integers(0, 301, count)
        chunks = [ac.zipf_syms(rng, n, int(L), s=float(rng.uniform(0.0, 1.6))) for L in lens]
        assert count % 64 != 0 and count > 64
        check_encode(m, params, chunks, base_s=count % 16, base_o=3, extra=7)
        check_decode(m, params, chunks, base=count % 16, seed=count)


@pytest.mark.parametrize("params", SHAPE_PARAMS)
def test_empty_chunks_only(ctx, params):
    """A launch whose chunks are all empty (T = 0 in every workgroup): 8 zero bytes each
    (Encoder::finish of the initial state), which decode to nothing with flag 0."""
    m = model(ctx, params)
    for count in (1, 64, 70):
        chunks = [np.zeros(0, np.uint8)] * count
        assert steps([0] * count) == 0
        h, _, out_off, ol, fl = encode_at(m, chunks, [16] * count, base_o=2)
        assert (fl == 0).all() and (ol == 8).all()
        for k in range(count):
            assert bytes(h[out_off[k]:out_off[k] + 8]) == bytes(8) == orc(params, chunks[k])[1]
        _, _, fd = decode_at(m, [bytes(8)] * count, [0] * count, base=3)
        assert (fd == 0).all()


# ------------------------------------------------------------------------------------------
# d. bad streams on every decoder variant
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", ac.BAD_VARIANTS)
def test_bad_streams(ctx, fixtures, params):
    """64 garbage streams (random, all 0xFF, 0xFF before a valid tail) decoded for 500 symbols
    and the truncations of one valid stream, in one launch at arbitrary code alignments: the
    oracle's flags, and its symbols wherever its flag is 0.  test_adaptive_ref.py shows from the
    same streams that the clamp of the exact target to total - 1 is reached on every variant."""
    garbage, truncated = ac.bad_streams(params, fixtures, cpu.encode_adaptive)
    codes = garbage + [c for c, _ in truncated]
    counts = [ac.BAD_COUNT] * len(garbage) + [n for _, n in truncated]
    m = model(ctx, params)
    s, sym_off, fd = decode_at(m, codes, counts, base=3, seed=params[0])
    clean = 0
    for k, (code, count) in enumerate(zip(codes, counts)):
        f, d = cpu.decode_adaptive(*params, code, count)
        assert fd[k] == f, (k, len(code))
        if f == 0:
            clean += 1
            assert bytes(s[sym_off[k]:sym_off[k + 1]]) == bytes(d), (k, len(code))
    assert clean >= 20 and (fd != 0).sum() >= 20  # both outcomes are well represented


# ------------------------------------------------------------------------------------------
# e. encoder slow path
# ------------------------------------------------------------------------------------------
def test_bad_symbol_in_every_slot(ctx):
    """64 copies of one 100-symbol chunk (n = 100), 23 of them with one symbol outside the
    alphabet: at indices 0..7 and 8..15 (every FIFO slot, step 0 and step 1) and 93..99 (the
    final partial step).  Those stop there with RC_F_BAD_SYMBOL and the oracle's out_len and
    bytes; the clean copies between them are bit-exact."""
    params = SET_C
    rng = np.random.default_rng(100)
    base = ac.zipf_syms(rng, 100, 100, s=0.8)
    where = list(range(16)) + list(range(93, 100))
    lanes = [int(v) for v in rng.permutation(64)[:len(where)]]
    chunks = [base.copy() for _ in range(64)]
    for lane, p in zip(lanes, where):
        chunks[lane][p] = (100, 128, 255)[p % 3]
    m = model(ctx, params)
    caps = [rc.slot_capacity(100, 16) + k % 5 for k in range(64)]
    h, _, out_off, ol, fl = encode_at(m, chunks, caps, base_o=1)
    n_bad = 0
    for k, c in enumerate(chunks):
        f, want, L = orc(params, c)
        assert f == (rc.api.N.F_BAD_SYMBOL if k in lanes else 0)
        n_bad += f != 0
        assert fl[k] == f and ol[k] == L, (k, fl[k], ol[k], L)
        assert bytes(h[out_off[k]:out_off[k] + L]) == want, k
    assert n_bad == 23


def test_capacity_limited_slots(ctx):
    """64 chunks of 300 symbols, every third slot smaller than its code (0, 1, 7, 8, 9, 16, 63
    bytes): RC_F_CAPACITY with the exact length and the first cap bytes; the chunks between
    them whole and bit-exact (so nothing spilled into a neighbour), sentinels untouched."""
    params = SET_C
    rng = np.random.default_rng(300)
    chunks = [ac.zipf_syms(rng, 100, 300, s=float(rng.uniform(0.0, 1.6))) for _ in range(64)]
    small = (0, 1, 7, 8, 9, 16, 63)
    caps, limited = [], []
    for k, c in enumerate(chunks):
        L = orc(params, c)[2]
        if k % 3 == 1:
            caps.append(small[(k // 3) % len(small)])
            assert caps[-1] < L
            limited.append(k)
        else:
            caps.append(L + k % 4)  # down to no spare byte at all
    assert {caps[k] for k in limited} == set(small)
    m = model(ctx, params)
    h, _, out_off, ol, fl = encode_at(m, chunks, caps, base_o=5)
    for k, c in enumerate(chunks):
        _, want, L = orc(params, c)
        f, cut, Lc = cpu.encode_adaptive(*params, c, cap=caps[k])
        assert f == (rc.api.N.F_CAPACITY if k in limited else 0) and Lc == L
        assert fl[k] == f and ol[k] == L, (k, fl[k], ol[k], L)
        assert bytes(h[out_off[k]:out_off[k] + min(L, caps[k])]) == cut == want[:caps[k]], k
