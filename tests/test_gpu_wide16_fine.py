"""Wide16 fine models (rc_model_create_static_wide16_fine: one table of up to 65536 16-bit symbols
with a total in (2^16, 2^24]) through the wide16 batch calls: byte-exact per chunk against the CPU
oracles (wide_ref.py, agnostic to alphabet and total) and by the round trip; against the 8-bit
static coders' route for totals above 2^16 where the alphabet fits a byte; every length at every
2-byte phase of a line, chunks of nothing but the costliest symbols beside healthy lanes,
workgroup seams, encoder flags, cut and garbage streams, the kind checks, model building and the
C++ example.  The arenas, guards and comparisons are test_gpu_wide16.py's."""
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
from test_gpu_wide16 import (SENT, check_round_trip, launch_lanes, reference,  # noqa: E402
                             run_decode, run_encode, zipf)
from wide_ref import decode_ref, encode_ref, literal_table, table  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T24 = 1 << 24


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def sparse_table():
    """2,048 occupied symbols of c in 1..3, a zero-frequency symbol between each pair, and one
    heavy symbol far behind them: total 2^20."""
    f = np.zeros(65536, np.int64)
    f[100:100 + 4096:2] = 1 + np.arange(2048) % 3
    f[50000] = (1 << 20) - int(f.sum())
    return f


def two_symbols():
    """Two occupied symbols 60,000 apart at total 2^24, the light one with c = 1."""
    f = np.zeros(65536, np.int64)
    f[3000], f[63000] = 1, T24 - 1
    return f


def skewed():
    """All 65536 symbols at total 2^24: Zipf(1.2) over half of them, c = 1 for the other half."""
    f = zipf(65536, T24 - 32768, live=32768)
    f[32768:] = 1
    return f


def models():
    rng = np.random.default_rng(24)
    ones = np.ones(65536, np.int64)
    ones[40000] = 2
    g = np.full(65535, 200, np.int64)
    g[::3] = 0
    g[65534] += T24 - 3 - int(g.sum())
    f5000 = np.zeros(5000, np.int64)
    f5000[rng.permutation(5000)[:3000]] = 1 + rng.multinomial(100003 - 3000, np.full(3000, 1 / 3000))
    return {
        "ones_65537": ones,
        "zipf_2p24": skewed()[rng.permutation(65536)],
        "sparse_2p20": sparse_table(),
        "two_2p24": two_symbols(),
        "n300_2p17": zipf(300, 1 << 17),
        "n5000_100003": f5000,
        "n65535_2p24m3": g,
    }


SHAPES = {"ones_65537": (65536, 65537), "zipf_2p24": (65536, T24), "sparse_2p20": (65536, 1 << 20),
          "two_2p24": (65536, T24), "n300_2p17": (300, 1 << 17), "n5000_100003": (5000, 100003),
          "n65535_2p24m3": (65535, T24 - 3)}
LENS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 300]


def mixed(rng, c, L):
    """L symbols of the table: half drawn by frequency, half evenly over the occupied symbols, so
    that the rare ones (the decoder's search and fix-up, the 4-byte symbols) come up."""
    occ = np.flatnonzero(c)
    p = np.asarray(c, np.float64)
    s = rng.choice(len(c), size=L, p=p / p.sum())
    even = rng.random(L) < 0.5
    s[even] = occ[rng.integers(0, len(occ), int(even.sum()))]
    return s.astype(np.uint16)


def last_lanes():
    out = (ctypes.c_uint32 * 2)()
    N.load().rc_wide16_fine_last_lanes_(out)
    return int(out[0]), int(out[1])


# ---------------------------------------------------------------- 1. parity, every model
@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_with_the_oracle(ctx, name):
    rng = np.random.default_rng(len(name) * 7 + SHAPES[name][0])
    c, cum, total = table(models()[name])
    assert (len(c), total) == SHAPES[name]
    model = rc.Wide16FineModel(c, cum, total)
    lens = LENS + [int(x) for x in rng.integers(0, 300, 40 - len(LENS))]
    chunks = [mixed(rng, c, lens[i]) for i in rng.permutation(len(lens))]
    if len(c) == 65536 and c[65535]:
        max(chunks, key=len)[-1] = 65535  # the largest 16-bit value, in a chunk's tail
    exp = reference(c, cum, total, chunks)
    assert all(f == 0 for f, _ in exp)
    for shift in (0, 5):
        check_round_trip(model, chunks, exp, shift, seed=shift + 1)


def test_every_length_at_every_symbol_phase_of_a_line(ctx):
    """Every length from 0 to 300, the first symbol at each of the 32 2-byte phases of a 64-B line
    (heads of 0 .. 31 symbols in both kernels), slots at odd byte offsets; a total that is no power
    of two."""
    rng = np.random.default_rng(32)
    c, cum, total = table(models()["n5000_100003"])
    model = rc.Wide16FineModel(c, cum, total)
    chunks = [mixed(rng, c, L) for L in rng.permutation(301)]
    exp = reference(c, cum, total, chunks)
    for shift in range(32):
        check_round_trip(model, chunks, exp, shift, seed=100 + shift)


# ---------------------------------------------------------------- 2. the rings' margins
@pytest.mark.parametrize("length", [300, 4097])
def test_chunks_of_nothing_but_the_costliest_symbols(ctx, length):
    """Chunks made only of c = 1 symbols at total 2^24, 24 bits each: the most bytes per symbol
    both rings see and the most range_reduction_expansion, in lanes of the same wave as chunks
    drawn from the table."""
    rng = np.random.default_rng(length)
    c, cum, total = table(models()["zipf_2p24"])
    assert total == T24
    model = rc.Wide16FineModel(c, cum, total)
    rare = np.flatnonzero(c == 1)
    assert len(rare) > 1000
    chunks = [mixed(rng, c, int(L)) for L in rng.integers(200, 400, 40)]
    for k in (0, 5, 17, 18, 39):
        chunks[k] = rare[rng.integers(0, len(rare), length)].astype(np.uint16)
    exp = reference(c, cum, total, chunks)
    assert all(f == 0 for f, _ in exp)
    assert len(exp[5][1]) >= 3 * length  # 24 bits a symbol
    for shift in (0, 3):
        check_round_trip(model, chunks, exp, shift, seed=length + shift)


@pytest.mark.parametrize("length", [128, 32])
def test_a_whole_wave_of_costliest_chunks_behind_a_long_head(ctx, length):
    """Every chunk of the wave is c = 1 symbols at total 2^24, so no healthier lane starts a flush
    round early.  The symbols start 2, 18 or 34 bytes past a 64-B line (heads of 31, 23 and 15
    symbols: the head ends 7 symbols past its last flush check and the body or the tail adds 8
    more before theirs) and the slots 11 to 15 bytes past one (the pad bytes count in the ring):
    the encoder's ring must take 3 bytes per symbol between any two checks.  Lengths are multiples
    of 32 symbols, so every chunk of the launch has the same head; 32 is a head and a tail with
    no tile between them."""
    rng = np.random.default_rng(length)
    c, cum, total = table(models()["zipf_2p24"])
    model = rc.Wide16FineModel(c, cum, total)
    rare = np.flatnonzero(c == 1)
    chunks = [rare[rng.integers(0, len(rare), length)].astype(np.uint16) for _ in range(64)]
    exp = reference(c, cum, total, chunks)
    assert all(f == 0 and len(b) >= 3 * length for f, b in exp)
    cat = np.concatenate(chunks).view(np.int16)
    sym_off = np.arange(65, dtype=np.int64) * length
    cap = (max(len(b) for _, b in exp) + 63) // 64 * 64 + 64
    for head in (31, 23, 15):
        shift = 32 - head
        big = torch.full((len(cat) + shift + 64,), -4370, dtype=torch.int16, device="cuda")
        assert big.data_ptr() % 64 == 0
        syms = big[shift:shift + len(cat)]
        syms.copy_(dev(cat))
        for al in range(11, 16):
            out = torch.full((64 * cap + 128,), SENT, dtype=torch.uint8, device="cuda")
            assert out.data_ptr() % 64 == 0
            out_off = np.arange(65, dtype=np.int64) * cap + al
            ol, fl = rc.encode_batch_wide16(model, syms, dev(sym_off), out, dev(out_off))
            torch.cuda.synchronize()
            h, ol, fl = out.cpu().numpy(), ol.cpu().numpy(), fl.cpu().numpy()
            assert (h[:al] == SENT).all() and (h[out_off[-1]:] == SENT).all()
            for k, (_, b) in enumerate(exp):
                assert (int(fl[k]), int(ol[k])) == (0, len(b)), (head, al, k)
                assert bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, (head, al, k)
    dec, fd = run_decode(model, [b for _, b in exp], [length] * 64, 1, seed=length)
    assert (fd == 0).all() and all(np.array_equal(d, s) for d, s in zip(dec, chunks))


# ---------------------------------------------------------------- 3. workgroups
@pytest.fixture(scope="module")
def seam_reference():
    rng = np.random.default_rng(2049)
    c, cum, total = table(models()["zipf_2p24"])
    chunks = [mixed(rng, c, 24) for _ in range(2049)]
    return c, cum, total, chunks, reference(c, cum, total, chunks)


def _dec_lanes():
    return rc.Wide16FineModel(np.full(256, 4096, np.uint32)).plan()["dec_lanes"]


@pytest.mark.parametrize("n_chunks", [1, 63, 64, 65, "lanes-1", "lanes", "lanes+1", 2049])
def test_workgroup_seams(ctx, seam_reference, n_chunks):
    c, cum, total, chunks, exp = seam_reference
    model = rc.Wide16FineModel(c, cum, total)
    plan = model.plan()["dec_lanes"]
    assert plan == _dec_lanes() and plan in (384, 1024)
    if isinstance(n_chunks, str):
        n_chunks = plan + {"lanes-1": -1, "lanes": 0, "lanes+1": 1}[n_chunks]
    check_round_trip(model, chunks[:n_chunks], exp[:n_chunks], shift=0, seed=3)
    assert last_lanes() == (launch_lanes(n_chunks), launch_lanes(n_chunks, plan))


def test_a_launch_of_the_plans_workgroups(ctx):
    """Enough chunks for the plan's own workgroup sizes in both directions, the last workgroup
    ragged: no oracle at this count, so the round trip, and chunk 0 against the oracle."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c, cum, total = table(models()["zipf_2p24"])
    model = rc.Wide16FineModel(c, cum, total)
    plan = model.plan()["dec_lanes"]
    n, L = cus * 1025 - 37, 12
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    cap = 80
    out_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap
    g = torch.Generator(device="cuda").manual_seed(1025)
    order = torch.from_numpy(np.argsort(-c.astype(np.int64), kind="stable").astype(np.int32)).cuda()
    rank = (torch.rand(n * L, device="cuda", generator=g) ** 4 * 65536).to(torch.int64)
    syms = order[rank.clamp_(0, 65535)].to(torch.int16)
    out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    ol, fl = rc.encode_batch_wide16(model, syms, sym_off, out, out_off)
    dec = torch.full_like(syms, -4370)
    fd = rc.decode_batch_wide16(model, out, out_off[:-1].contiguous(), ol, dec, sym_off)
    torch.cuda.synchronize()
    assert last_lanes() == (1024, plan) == (launch_lanes(n), launch_lanes(n, plan))
    assert int(fl.abs().sum()) == 0 and int(fd.abs().sum()) == 0 and torch.equal(dec, syms)
    f, b = encode_ref(c, cum, total, syms[:L].cpu().numpy().view(np.uint16))
    assert f == 0 and bytes(out[:int(ol[0])].cpu().numpy()) == b


# ---------------------------------------------------------------- 4. the 8-bit coders' route
@pytest.mark.parametrize("total", [1 << 17, 1 << 20, T24 - 3])
def test_static_coders_give_the_same_bytes(ctx, total):
    """n <= 256: the 8-bit static coders code a total above 2^16 on their own wide route (other
    kernels, other tables); the fine model's bytes on the same symbol values equal theirs, and the
    fine decoder returns the symbols from their bytes."""
    rng = np.random.default_rng(total)
    f = zipf(256, total, live=200)
    f[7] += f[9]
    f[9] = 0
    c, cum, t = table(f[rng.permutation(256)])
    assert t == total
    fine, m8 = rc.Wide16FineModel(c, cum, total), rc.StaticModel(c, cum, total)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 300, 1000] + [int(x) for x in rng.integers(0, 600, 60)]
    chunks = [mixed(rng, c, L) for L in lens]
    n = len(chunks)
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cat = np.concatenate(chunks + [np.zeros(1, np.uint16)])
    caps = np.array([rc.slot_capacity(L, 25.0) + 64 for L in lens], np.int64)
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    out8 = torch.full((int(out_off[-1]),), SENT, dtype=torch.uint8, device="cuda")
    out16 = torch.full_like(out8, SENT)
    ol8, fl8 = rc.encode_batch(m8, dev(cat.astype(np.uint8)), dev(sym_off), out8, dev(out_off))
    ol16, fl16 = rc.encode_batch_wide16(fine, dev(cat.view(np.int16)), dev(sym_off), out16,
                                        dev(out_off))
    torch.cuda.synchronize()
    assert int(fl8.abs().sum()) == 0 and int(fl16.abs().sum()) == 0 and torch.equal(ol8, ol16)
    h8, h16, ol = out8.cpu().numpy(), out16.cpu().numpy(), ol8.cpu().numpy()
    for k in range(n):
        a = slice(out_off[k], out_off[k] + ol[k])
        assert bytes(h8[a]) == bytes(h16[a]), (k, lens[k])
    assert bytes(h16[out_off[8]:out_off[8] + ol[8]]) == encode_ref(c, cum, total, chunks[8])[1]
    dec = torch.full((int(sym_off[-1]) + 1,), -4370, dtype=torch.int16, device="cuda")
    fd = rc.decode_batch_wide16(fine, out8, dev(out_off[:-1].copy()), ol8, dec, dev(sym_off))
    torch.cuda.synchronize()
    assert int(fd.abs().sum()) == 0
    assert np.array_equal(dec.cpu().numpy().view(np.uint16)[:-1], cat[:-1])


# ---------------------------------------------------------------- 5. encode flags
@pytest.mark.parametrize("name", ["n300_2p17", "n65535_2p24m3", "zipf_2p24"])
def test_encode_flags(ctx, name):
    f = models()[name].copy()
    n = len(f)
    zero = None
    if n < 65536:
        zero = int(np.flatnonzero(f)[5])
        f[int(np.flatnonzero(f)[0])] += f[zero]
        f[zero] = 0  # a zero-frequency symbol among occupied ones
    c, cum, total = table(f)
    model = rc.Wide16FineModel(c, cum, total)
    rng = np.random.default_rng(78)
    chunks = [mixed(rng, c, 300) for _ in range(70)]  # chunks 0..63 share a wave
    want = {}
    if n < 65536:
        for k, (at, v) in enumerate([(0, n), (150, n), (299, n), (0, 65535), (150, 65535),
                                     (299, 65535)]):
            chunks[10 + k][at] = v  # a value >= n at the first, a middle and the last symbol
            want[10 + k] = N.F_BAD_SYMBOL
        chunks[3][100] = zero
        want[3] = N.F_ZERO_FREQ
        chunks[30][50], chunks[30][200] = zero, n  # the first error wins, whatever its kind
        want[30] = N.F_ZERO_FREQ
        chunks[31][7], chunks[31][8] = 65535, zero
        want[31] = N.F_BAD_SYMBOL
    else:
        for k, at in enumerate((0, 150, 299)):
            chunks[10 + k][at] = 65535  # no 16-bit value is outside this alphabet
    exp = reference(c, cum, total, chunks)
    assert {k: f for k, (f, _) in enumerate(exp) if f} == want
    caps = [rc.slot_capacity(300, 25.0)] * 70
    caps[40] = len(exp[40][1]) - 1  # a slot one byte short
    for shift in (0, 7):
        h, out_off, ol, fl = run_encode(model, chunks, caps, shift, seed=5 + shift)
        for k, (f, b) in enumerate(exp):
            if k == 40:
                assert (int(fl[k]), int(ol[k])) == (N.F_CAPACITY, len(b))  # the exact length
                continue
            assert int(fl[k]) == f, (k, fl[k], f)
            if f == 0:  # the neighbours of the flagged chunks stay clean and bit-exact
                assert int(ol[k]) == len(b) and bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, k
        h, out_off, ol, fl = run_encode(model, [chunks[40]], [int(ol[40])], shift, seed=6)
        assert int(fl[0]) == 0 and bytes(h[out_off[0]:out_off[0] + ol[0]]) == exp[40][1]


# ---------------------------------------------------------------- 6. bad streams
@pytest.mark.parametrize("which", ["sparse", "two"])
def test_bad_streams(ctx, which):
    """One stream of 48 symbols cut at every length from 0 to its own, and 32 more with garbage
    tails or of garbage alone: flags and the symbols before the first error equal the literal
    decoder's, its choice of n - 1 when rfreq >= total (c = 0 there: CORRUPT) included; nothing
    is written outside the chunks.  Every stream is compared."""
    rng = np.random.default_rng(60)
    f = sparse_table() if which == "sparse" else two_symbols()
    if which == "two":  # (evened out, so that the stream is worth cutting)
        f[3000], f[63000] = T24 // 3, T24 - T24 // 3
    c, cum, total = table(f)
    lit = literal_table(c)
    model = rc.Wide16FineModel(c, cum, total)
    s = mixed(rng, c, 48)
    fl, good = encode_ref(c, cum, total, s)
    assert fl == 0 and len(good) > 12
    codes = [good[:cut] for cut in range(len(good) + 1)]
    counts = [48] * len(codes)
    n_cut = len(codes)
    for j in range(32):
        cut = int(rng.integers(0, len(good)))
        tail = rng.integers(0, 256, int(rng.integers(8, 200))).astype(np.uint8).tobytes()
        codes.append(tail if j % 4 == 3 else good[:cut] + tail)
        counts.append(int(rng.integers(1, 65)))
    codes[-1] = b"\xff" * 64  # data - low at its largest: rfreq >= total at the first symbol
    exp = [decode_ref(c, cum, total, codes[k], counts[k], lit) for k in range(len(codes))]
    assert all(exp[cut][0] == N.F_TRUNCATED for cut in range(8)) and exp[n_cut - 1][0] == 0
    assert np.array_equal(exp[n_cut - 1][1], s)
    assert {f for f, _ in exp} <= {0, N.F_TRUNCATED, N.F_CORRUPT}
    assert N.F_CORRUPT in {f for f, _ in exp}
    for shift in (0, 9):
        dec, fd = run_decode(model, codes, counts, shift, seed=61 + shift)
        for k, (f, want) in enumerate(exp):
            assert int(fd[k]) == f, (k, len(codes[k]), fd[k], f)
            assert np.array_equal(dec[k][:len(want)], want), (k, f)
            if f == 0:
                assert len(want) == counts[k]


# ---------------------------------------------------------------- 7. kinds do not mix
def test_kinds_do_not_mix(ctx):
    c, cum, total = table(models()["n300_2p17"])
    fine = rc.Wide16FineModel(c, cum, total)
    lib = ctx._lib
    zc, zcum, zt = synth.zipf_table()
    m = rc.StaticModel(zc, zcum, zt)
    w = rc.WideStaticModel(np.full(300, 200, np.uint32))
    ms = rc.StaticModelSet(np.tile(np.asarray(zc, np.uint32), (2, 1)), None, zt)
    o1 = rc.Order1ModelSet(np.tile(np.asarray(zc, np.uint32), (2, 1)), None, zt,
                           np.zeros(256, np.uint8))
    cs = rc.ChunkModelSet(np.tile(np.asarray(zc, np.uint32), (2, 1)), None, zt)
    syms = torch.zeros(512, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 128, 256], dtype=torch.int64, device="cuda")
    out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    out_off = torch.tensor([0, 2048, 4096], dtype=torch.int64, device="cuda")
    ol = torch.zeros(2, dtype=torch.int64, device="cuda")
    fl = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    h = fine.handle
    C = ctx.handle
    enc_args = (p(syms), p(off), 2, p(out), p(out_off), p(ol), p(fl))
    dec_args = (p(out), p(out_off), p(ol), p(syms), p(off), 2, p(fl))
    # a fine model to every other entry point that takes a model
    for e, d in (("rc_encode_batch", "rc_decode_batch"),
                 ("rc_encode_batch_wide", "rc_decode_batch_wide"),
                 ("rc_encode_batch_order1", "rc_decode_batch_order1")):
        assert getattr(lib, e)(C, h, *enc_args) == N.RC_E_ARG, e
        assert getattr(lib, d)(C, h, *dec_args) == N.RC_E_ARG, d
    for e, d in (("rc_encode_batch_indexed", "rc_decode_batch_indexed"),
                 ("rc_encode_batch_chunk_set", "rc_decode_batch_chunk_set")):
        assert getattr(lib, e)(C, h, p(syms), p(syms), p(off), 2, p(out), p(out_off), p(ol),
                               p(fl)) == N.RC_E_ARG, e
        assert getattr(lib, d)(C, h, p(out), p(out_off), p(ol), p(syms), p(syms), p(off), 2,
                               p(fl)) == N.RC_E_ARG, d
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    n_out = ctypes.c_uint64()
    assert lib.rc_container_pack(C, h, p(out), p(out_off), p(ol), p(off), 2, p(dst), 8192,
                                 ctypes.byref(n_out)) == N.RC_E_ARG
    assert lib.rc_container2_pack(C, h, p(out), p(out_off), p(ol), p(off), 2, None, p(dst), 8192,
                                  ctypes.byref(n_out)) == N.RC_E_ARG
    bits = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert lib.rc_ideal_bits_wide(C, h, p(syms), p(off), 2, p(bits)) == N.RC_E_ARG
    with pytest.raises(N.RCError) as e:
        rc.encode_host(fine, np.zeros(256, np.uint8), np.array([0, 128, 256], np.uint64),
                       np.array([0, 2048, 4096], np.uint64))
    assert e.value.code == N.RC_E_ARG
    # every other model to the wide16 calls, as before
    for other in (m, w, ms, o1, cs):
        assert lib.rc_encode_batch_wide16(C, other.handle, *enc_args) == N.RC_E_ARG
        assert lib.rc_decode_batch_wide16(C, other.handle, *dec_args) == N.RC_E_ARG
    # 16-bit symbols at an odd address
    odd = ctypes.c_void_p(syms.data_ptr() + 1)
    assert lib.rc_encode_batch_wide16(C, h, odd, p(off), 2, p(out), p(out_off), p(ol),
                                      p(fl)) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()  # nothing was launched
    # each table has one constructor: 65536 is the wide16 one's, 65537 the fine one's
    hh = ctypes.c_void_p()
    pa = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for tot, fine_rc, w16_rc in ((65536, N.RC_E_BAD_MODEL, N.RC_OK),
                                 (65537, N.RC_OK, N.RC_E_BAD_MODEL),
                                 (T24 + 1, N.RC_E_BAD_MODEL, N.RC_E_BAD_MODEL)):
        f = np.full(256, tot // 256, np.int64)
        f[0] += tot - int(f.sum())
        cc, cu, _ = table(f)
        for fn, want in (("rc_model_create_static_wide16_fine", fine_rc),
                         ("rc_model_create_static_wide16", w16_rc)):
            assert getattr(lib, fn)(C, 256, pa(cc), pa(cu), tot, ctypes.byref(hh)) == want, (fn, tot)
            if want == N.RC_OK:
                lib.rc_model_destroy(hh)


# ---------------------------------------------------------------- 8. model building
def test_build_wide16_model_at_a_fine_total_codes_shorter(ctx):
    """2^18 int16 Laplace(b = 1500) samples in 16-Ki chunks: the table of target_total 2^20 is a
    fine model, round-trips the data, and its code is strictly shorter than the code under the
    table of target_total 2^16 (ideal lengths under a plain quantiser: 12.94 against 13.14 bits
    per symbol, so the inequality has about 1.5 % of room)."""
    rng = np.random.default_rng(1500)
    n = 1 << 18
    s = np.clip(np.rint(rng.laplace(0.0, 1500.0, n)), -32768, 32767).astype(np.int16)
    u = s.view(np.uint16)
    sym_off = np.arange(0, n + 1, 1 << 14, dtype=np.int64)
    chunks = [u[sym_off[k]:sym_off[k + 1]] for k in range(len(sym_off) - 1)]
    fine = rc.build_wide16_model(dev(s), dev(sym_off), target_total=1 << 20)
    coarse = rc.build_wide16_model(dev(s), dev(sym_off), target_total=1 << 16)
    assert type(fine) is rc.Wide16FineModel and fine.total == 1 << 20
    assert type(coarse) is rc.Wide16StaticModel and coarse.total == 1 << 16
    assert ((fine.c > 0) == (np.bincount(u, minlength=fine.n_symbols) > 0)).all()
    codes = rc.encode_chunks_wide16(fine, chunks)
    assert codes[3] == encode_ref(fine.c, fine.cum, fine.total, chunks[3])[1]
    back = rc.decode_chunks_wide16(fine, codes, [len(x) for x in chunks])
    assert all(np.array_equal(a, b) for a, b in zip(chunks, back))
    size_fine = sum(len(x) for x in codes)
    size_coarse = sum(len(x) for x in rc.encode_chunks_wide16(coarse, chunks))
    print(f"code bytes: {size_fine} at total 2^20 ({8 * size_fine / n:.4f} bits/symbol), "
          f"{size_coarse} at total 2^16 ({8 * size_coarse / n:.4f} bits/symbol)")
    assert size_fine < size_coarse
    with pytest.raises(ValueError):
        rc.build_wide16_model(dev(s), dev(sym_off), target_total=T24 + 1)


# ---------------------------------------------------------------- 9. the C++ example
def test_cpp_wide16_fine_impl(ctx):
    """examples/wide16_fine_impl: a skewed table over all 65536 symbols at total 2^20 through
    rc::Wide16FineModel, against the per-call rc::Encoder given the same table, and back."""
    exe = os.path.join(ROOT, "examples", "wide16_fine_impl")
    assert os.path.exists(exe), "examples/wide16_fine_impl not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "round trip ok" in r.stdout and "test passed" in r.stdout
    assert "all ones at total 2^16" in r.stdout
