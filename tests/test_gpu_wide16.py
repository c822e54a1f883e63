"""The wide16 batch coders (rc_encode_batch_wide16 / rc_decode_batch_wide16: 16-bit symbols
against one static table of up to 65536 symbols held in device memory) through the C ABI:
byte-exact per chunk against the CPU oracles (wide_ref.py, alphabet-agnostic) and by the round
trip, and equal to the wide coders where both accept the table.  Ragged arenas at every 2-byte
phase of a 64-B line, odd slot offsets, guard bytes around slots and decoded symbols, workgroup
seams and the smaller workgroups of small launches, flags, bad streams, the fix-up's tables, the
tight code-ring fixtures, the kind checks, model building and the C++ example."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N, synth  # noqa: E402
from gpu_helpers import dev, ring_check_exact, ring_decode_at  # noqa: E402
from wide_ref import decode_ref, encode_ref, literal_table, table  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xEE
SENT16 = np.uint16(0xEEEE).view(np.int16)
W16 = (rc.encode_batch_wide16, rc.decode_batch_wide16)
WIDE = (rc.encode_batch_wide, rc.decode_batch_wide)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


# ---------------------------------------------------------------- arenas through the C ABI
def _sym_arena(values, shift):
    """An int16 tensor holding the uint16 `values`, its first symbol `shift` symbols past a
    256-B aligned allocation, guard symbols on both sides."""
    v = np.ascontiguousarray(values, np.uint16).view(np.int16)
    big = torch.full((len(v) + shift + 64,), int(SENT16), dtype=torch.int16, device="cuda")
    view = big[shift:shift + len(v)]
    view.copy_(dev(v))
    return view, big


def run_encode(model, chunks, caps, shift=0, seed=0, calls=W16):
    """chunks: uint16 arrays at contiguous ragged offsets.  shift: symbols between an aligned
    base and the first symbol; with a shift the slots start at an odd byte offset too."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(s) for s in chunks], np.int64)
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cat = np.concatenate([np.asarray(s, np.uint16) for s in chunks] + [np.zeros(1, np.uint16)])
    syms, _keep = _sym_arena(cat, shift)
    bo = 2 * int(rng.integers(0, 8)) + 1 if shift else 0
    caps = np.asarray(caps, np.int64)
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + bo
    out = torch.full((int(out_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = calls[0](model, syms, dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    # nothing is written outside the slots (bytes past out_len inside a slot are unspecified)
    assert (h[:bo] == SENT).all() and (h[out_off[-1]:] == SENT).all()
    return h, out_off, out_len.cpu().numpy(), flags.cpu().numpy()


def run_decode(model, codes, counts, shift=0, seed=0, calls=W16):
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
    flags = calls[1](model, dev(np.concatenate(parts)), dev(coff), dev(clen), syms, dev(sym_off))
    torch.cuda.synchronize()
    s = syms.cpu().numpy().view(np.uint16)
    b = big.cpu().numpy()
    # nothing is written outside the chunks' symbol ranges
    assert (b[:shift + sym_off[0]] == SENT16).all() and (b[shift + sym_off[-1]:] == SENT16).all()
    return [s[sym_off[k]:sym_off[k + 1]] for k in range(n)], flags.cpu().numpy()


def reference(c, cum, total, chunks):
    return [encode_ref(c, cum, total, s) for s in chunks]


def check_round_trip(model, chunks, exp, shift, seed, slack=64, calls=W16):
    """Encode and decode `chunks`; bytes, lengths and flags equal the oracle's (exp), and the GPU
    decoder returns the symbols from those bytes."""
    bits = model.max_bits_per_symbol() + 1
    caps = [rc.slot_capacity(len(s), bits) + slack for s in chunks]
    h, out_off, ol, fl = run_encode(model, chunks, caps, shift, seed, calls)
    for k, (s, (f, b)) in enumerate(zip(chunks, exp)):
        assert (int(fl[k]), int(ol[k])) == (f, len(b)), (k, len(s), fl[k], ol[k], f, len(b))
        assert bytes(h[out_off[k]:out_off[k] + ol[k]]) == b, (k, len(s))
    dec, fd = run_decode(model, [b for _, b in exp], [len(s) for s in chunks], shift, seed + 1,
                         calls)
    for k, s in enumerate(chunks):
        assert fd[k] == 0 and np.array_equal(dec[k], np.asarray(s, np.uint16)), (k, len(s))


def draw(rng, c, L):
    p = np.asarray(c, np.float64)
    return rng.choice(len(c), size=L, p=p / p.sum()).astype(np.uint16)


def spread(rng, live, total):
    """`live` frequencies >= 1 summing to total, unevenly."""
    w = rng.random(live) ** 3 + 1e-9
    return 1 + rng.multinomial(total - live, w / w.sum())


def zipf(n, total, live=None):
    """Zipf(1.2) over the first `live` of n symbols, every one of them c >= 1, zeros behind."""
    live = n if live is None else live
    z = 1.0 / np.arange(1, live + 1) ** 1.2
    f = np.zeros(n, np.int64)
    f[:live] = 1 + np.floor(z / z.sum() * (total - live)).astype(np.int64)
    f[0] += total - int(f.sum())
    return f


def three_symbols():
    f = np.zeros(65536, np.int64)
    f[0], f[30000], f[65535] = 1000, 64000, 536
    return f


def gap_table():
    """Two occupied symbols 60,000 zero-frequency ones apart (and narrow neighbours)."""
    f = np.zeros(65536, np.int64)
    f[99], f[100], f[60101], f[60102] = 3, 20000, 20000, 5
    f[65000] = 65536 - int(f.sum())
    return f


def narrow_table():
    """4096 symbols, every second one c = 0, the others c in 1..3: hint misses are frequent."""
    rng = np.random.default_rng(4096)
    f = np.zeros(4096, np.int64)
    f[1::2] = rng.integers(1, 4, 2048)
    return f


def models():
    rng = np.random.default_rng(16)
    z = zipf(65536, 65536, live=30000)
    return {
        "n1": [256],
        "n256": spread(rng, 256, 65536),
        "n4096": spread(rng, 4096, 65536),
        "n4097": spread(rng, 4097, 65536),
        "n20000": spread(rng, 20000, 65535),
        "n65535": np.concatenate([spread(rng, 30000, 40000),
                                  np.zeros(35535, np.int64)])[rng.permutation(65535)],
        "ones": np.ones(65536, np.int64),
        "zipf_zeros": z[rng.permutation(65536)],
        "three": three_symbols(),
    }


SHAPES = {"n1": (1, 256), "n256": (256, 65536), "n4096": (4096, 65536), "n4097": (4097, 65536),
          "n20000": (20000, 65535), "n65535": (65535, 40000), "ones": (65536, 65536),
          "zipf_zeros": (65536, 65536), "three": (65536, 65536)}
LENS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 300]


# ---------------------------------------------------------------- 1. parity, every model
@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_with_the_oracle(ctx, name):
    rng = np.random.default_rng(len(name) * 7 + SHAPES[name][0])
    c, cum, total = table(models()[name])
    assert (len(c), total) == SHAPES[name]
    model = rc.Wide16StaticModel(c, cum, total)
    lens = LENS + [int(x) for x in rng.integers(0, 300, 40 - len(LENS))]
    chunks = [draw(rng, c, lens[i]) for i in rng.permutation(len(lens))]
    if len(c) == 65536 and c[65535]:
        max(chunks, key=len)[-1] = 65535  # the largest 16-bit value, in a chunk's tail
    exp = reference(c, cum, total, chunks)
    assert all(f == 0 for f, _ in exp)
    for shift in (0, 5):
        check_round_trip(model, chunks, exp, shift, seed=shift + 1)


def test_every_symbol_phase_of_a_line(ctx):
    """The first symbol at each of the 32 2-byte phases of a 64-B line (heads of 0 .. 31 symbols
    in both kernels), slots at odd byte offsets, every length of the list."""
    rng = np.random.default_rng(32)
    c, cum, total = table(models()["n4097"])
    model = rc.Wide16StaticModel(c, cum, total)
    chunks = [draw(rng, c, L) for L in LENS + LENS[::-1]]
    exp = reference(c, cum, total, chunks)
    for shift in range(32):
        check_round_trip(model, chunks, exp, shift, seed=100 + shift)


# ---------------------------------------------------------------- 2. the wide coders' bytes
@pytest.mark.parametrize("which", ["dense", "narrow"])
def test_wide_calls_give_the_same_bytes(ctx, which):
    """n = 4096: bytes, lengths and flags equal rc_encode_batch_wide / rc_decode_batch_wide on the
    same inputs (and the oracle's).  "narrow" is the fix-up's table: 2,048 occupied symbols of c
    in 1..3, a zero-frequency one between each two, so a hint one q off names another symbol."""
    rng = np.random.default_rng(11)
    c, cum, total = table(zipf(4096, 65536) if which == "dense" else narrow_table())
    w16, w = rc.Wide16StaticModel(c, cum, total), rc.WideStaticModel(c, cum, total)
    chunks = [draw(rng, c, 300) for _ in range(70)] + [draw(rng, c, L) for L in LENS]
    chunks[3][17] = 4096  # flagged chunks too
    chunks[4][299] = 65535
    if which == "narrow":
        chunks[6][150] = 2  # c = 0
    exp = reference(c, cum, total, chunks)
    caps = [rc.slot_capacity(len(s), w16.max_bits_per_symbol() + 1) + 64 for s in chunks]
    caps[9] = len(exp[9][1]) - 3
    got = [run_encode(m, chunks, caps, 3, 7, calls) for m, calls in ((w16, W16), (w, WIDE))]
    (h, off, ol, fl), (h2, off2, ol2, fl2) = got
    assert np.array_equal(fl, fl2) and np.array_equal(off, off2)
    for k, (f, b) in enumerate(exp):
        if k == 9:
            assert (int(fl[k]), int(ol[k]), int(ol2[k])) == (N.F_CAPACITY, len(b), len(b))
            continue
        assert int(fl[k]) == f, k
        if f == 0:
            assert int(ol[k]) == int(ol2[k]) == len(b)
            assert bytes(h[off[k]:off[k] + ol[k]]) == bytes(h2[off[k]:off[k] + ol[k]]) == b, k
    good = [k for k, (f, _) in enumerate(exp) if f == 0]
    codes = [exp[k][1] for k in good]
    # cut and garbage streams as well: the decoders agree on flags and on every symbol written
    codes += [codes[0][:40], codes[1][:8], rng.integers(0, 256, 200).astype(np.uint8).tobytes()]
    counts = [len(chunks[k]) for k in good] + [300, 300, 150]
    d16, f16 = run_decode(w16, codes, counts, 3, 8, W16)
    dw, fw = run_decode(w, codes, counts, 3, 8, WIDE)
    assert np.array_equal(f16, fw) and (f16[:len(good)] == 0).all()
    for j, k in enumerate(good):
        assert np.array_equal(d16[j], chunks[k]) and np.array_equal(dw[j], chunks[k]), k
    for j in range(len(good), len(codes)):
        f, want = decode_ref(c, cum, total, codes[j], counts[j])
        assert int(f16[j]) == f
        assert np.array_equal(d16[j][:len(want)], want) and np.array_equal(dw[j][:len(want)], want)


def test_occupied_symbols_60000_apart(ctx):
    """The fix-up steps from one occupied symbol to the next through the q-to-symbol table, so
    60,000 zero-frequency symbols between two neighbours cost it one step."""
    rng = np.random.default_rng(60000)
    c, cum, total = table(gap_table())
    model = rc.Wide16StaticModel(c, cum, total)
    chunks = [draw(rng, c, 300) for _ in range(66)]
    chunks[0][:8] = [99, 100, 60101, 60102, 60101, 100, 99, 65000]
    check_round_trip(model, chunks, reference(c, cum, total, chunks), 1, seed=6)


# ---------------------------------------------------------------- 3. workgroups
def launch_lanes(n_chunks, plan_lanes=1024):
    """set_launch_lanes: the plan's lanes, or fewer so that a small launch reaches every CU."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = ((n_chunks + cus - 1) // cus + 63) & ~63
    return min(plan_lanes, 256) if per < 256 else min(per, plan_lanes)


def last_lanes():
    out = (ctypes.c_uint32 * 2)()
    N.load().rc_wide16_last_lanes_(out)
    return int(out[0]), int(out[1])


@pytest.fixture(scope="module")
def seam_reference():
    rng = np.random.default_rng(2049)
    c, cum, total = table(models()["zipf_zeros"])
    chunks = [draw(rng, c, 40) for _ in range(2049)]
    return c, cum, total, chunks, reference(c, cum, total, chunks)


@pytest.mark.parametrize("n_chunks", [1023, 1024, 1025, 2049, 3])
def test_workgroup_seams(ctx, seam_reference, n_chunks):
    c, cum, total, chunks, exp = seam_reference
    model = rc.Wide16StaticModel(c, cum, total)
    check_round_trip(model, chunks[:n_chunks], exp[:n_chunks], shift=0, seed=3)
    assert last_lanes() == (launch_lanes(n_chunks), launch_lanes(n_chunks, 384))


@pytest.mark.parametrize("per_cu,total", [(300, 65536), (700, 65536), (1025, 65536),
                                          (700, 32768), (1025, 32768)])
def test_workgroup_sizes_of_larger_launches(ctx, per_cu, total):
    """Enough chunks for encoder workgroups of 320, 704 and 1,024 lanes (the plan's) and decoder
    workgroups of 320 and 384 lanes (the plan's above a total of 2^15) and of 704 and 1,024 (at
    2^15), the last workgroup ragged: no oracle at this count, so the n = 4096 model against the
    wide calls on the same symbols, and the n = 65536 model by its round trip."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, L = cus * per_cu - 37, 12
    lanes = launch_lanes(n)
    assert lanes == min(1024, (per_cu + 63) & ~63)
    dec_plan = 384 if total > 32768 else 1024
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    cap = 64
    out_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap
    g = torch.Generator(device="cuda").manual_seed(per_cu)
    for nsym in (4096, 65536):
        live = min(nsym, 30000)
        c, cum, t = table(zipf(nsym, total, live=live))
        assert t == total
        w16 = rc.Wide16StaticModel(c, cum, total)
        assert w16.plan()["dec_lanes"] == dec_plan
        syms = (torch.rand(n * L, device="cuda", generator=g) ** 4 * live).to(torch.int32)
        syms = syms.clamp_(0, live - 1).to(torch.int16)
        out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        ol, fl = rc.encode_batch_wide16(w16, syms, sym_off, out, out_off)
        dec = torch.full_like(syms, int(SENT16))
        fd = rc.decode_batch_wide16(w16, out, out_off[:-1].contiguous(), ol, dec, sym_off)
        torch.cuda.synchronize()
        assert last_lanes() == (lanes, launch_lanes(n, dec_plan))
        assert int(fl.abs().sum()) == 0 and int(fd.abs().sum()) == 0 and torch.equal(dec, syms)
        if nsym == 4096:
            w = rc.WideStaticModel(c, cum, total)
            out2 = torch.zeros_like(out)
            ol2, fl2 = rc.encode_batch_wide(w, syms, sym_off, out2, out_off)
            torch.cuda.synchronize()
            valid = torch.arange(cap, device="cuda")[None, :] < ol[:, None]
            assert torch.equal(ol, ol2) and torch.equal(fl, fl2)
            assert torch.equal(out.view(n, cap) * valid, out2.view(n, cap) * valid)


# ---------------------------------------------------------------- 4. encode flags
@pytest.mark.parametrize("name", ["n4097", "n65535", "ones"])
def test_encode_flags(ctx, name):
    f = models()[name].copy()
    n = len(f)
    zero = None
    if name != "ones":
        zero = int(np.flatnonzero(f)[5])
        f[int(np.flatnonzero(f)[0])] += f[zero]
        f[zero] = 0  # a zero-frequency symbol among occupied ones
    c, cum, total = table(f)
    model = rc.Wide16StaticModel(c, cum, total)
    rng = np.random.default_rng(78)
    chunks = [draw(rng, c, 300) for _ in range(70)]  # chunks 0..63 share a wave
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
    caps = [rc.slot_capacity(300, 16.5)] * 70
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


# ---------------------------------------------------------------- 5. bad streams
@pytest.mark.parametrize("which", ["three", "gap", "narrow"])
def test_bad_streams(ctx, which):
    """32 cut and garbage streams over the sparse tables: flags and the symbols before the first
    error equal the literal decoder's, its choice of n - 1 when rfreq >= total (c = 0 there:
    CORRUPT) and its walk's end included; nothing is written outside the chunks."""
    rng = np.random.default_rng(60)
    f = {"three": three_symbols, "gap": gap_table, "narrow": narrow_table}[which]()
    if which == "three":  # (evened out, so that 120 symbols make a stream worth cutting)
        f[0], f[30000] = 30000, 35000
        f[65535], f[65534] = 0, 536  # the last symbol empty: rfreq >= total lands on c = 0
    c, cum, total = table(f)
    lit = literal_table(c)
    model = rc.Wide16StaticModel(c, cum, total)
    s = draw(rng, c, 120)
    fl, good = encode_ref(c, cum, total, s)
    assert fl == 0 and len(good) > 12
    codes = [good[:cut] for cut in list(range(10)) + [len(good) // 2, len(good) - 1, len(good)]]
    counts = [120] * len(codes)
    while len(codes) < 32:
        codes.append(rng.integers(0, 256, int(rng.integers(8, 200))).astype(np.uint8).tobytes())
        counts.append(int(rng.integers(1, 201)))
    codes[-1] = b"\xff" * 64  # data - low at its largest: rfreq >= total at the first symbol
    exp = [decode_ref(c, cum, total, codes[k], counts[k], lit) for k in range(32)]
    assert all(exp[cut][0] == N.F_TRUNCATED for cut in range(8)) and exp[12][0] == 0
    assert {f for f, _ in exp} <= {0, N.F_TRUNCATED, N.F_CORRUPT}
    if which != "narrow":
        assert N.F_CORRUPT in {f for f, _ in exp}
    for shift in (0, 9):
        dec, fd = run_decode(model, codes, counts, shift, seed=61 + shift)
        for k, (f, want) in enumerate(exp):
            assert int(fd[k]) == f, (k, len(codes[k]), fd[k], f)
            assert np.array_equal(dec[k][:len(want)], want), (k, f)
            if f == 0:
                assert len(want) == counts[k]


# ---------------------------------------------------------------- 6. the tight code rings
@pytest.mark.parametrize("name", ["pow2", "magic"])
def test_tight_ring_streams(ctx, name):
    """tests/golden/ring_tight.json as an n = 256 wide16 model (the symbols widened to 16 bits):
    at every head some stream was steered for, and as a launch of more than one workgroup."""
    with open(os.path.join(ROOT, "tests", "golden", "ring_tight.json")) as fh:
        fx = json.load(fh)
    md = fx["models"][name]
    chunks = [ch for ch in fx["chunks"] if ch["model"] == name]
    w = rc.Wide16StaticModel(np.array(md["c"], np.uint32), np.array(md["cum"], np.uint32),
                             md["total"])
    heads = sorted({ch["head"] for ch in chunks if ch["head"] <= 31} | {16})
    call = lambda *a: rc.decode_batch_wide16(w, *a)  # noqa: E731
    for off in sorted({(32 - h) % 32 for h in heads} | {0, 1, 3, 31}):
        s, sym_off, flags = ring_decode_at(call, chunks, off, wide=True)
        ring_check_exact(s, sym_off, flags, chunks)
    many = (chunks * (1280 // len(chunks) + 1))[:1280]
    s, sym_off, flags = ring_decode_at(call, many, 3, wide=True)
    ring_check_exact(s, sym_off, flags, many)


# ---------------------------------------------------------------- 7. kinds do not mix
def test_kinds_do_not_mix(ctx):
    c, cum, total = table(models()["n4096"])
    w16 = rc.Wide16StaticModel(c, cum, total)
    w = rc.WideStaticModel(c, cum, total)
    lib = ctx._lib
    zc, zcum, zt = synth.zipf_table()
    m = rc.StaticModel(zc, zcum, zt)
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
    h = w16.handle
    C = ctx.handle
    enc_args = (p(syms), p(off), 2, p(out), p(out_off), p(ol), p(fl))
    dec_args = (p(out), p(out_off), p(ol), p(syms), p(off), 2, p(fl))
    # a wide16 model to every other entry point that takes a model
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
        rc.encode_host(w16, np.zeros(256, np.uint8), np.array([0, 128, 256], np.uint64),
                       np.array([0, 2048, 4096], np.uint64))
    assert e.value.code == N.RC_E_ARG
    # every other model to the wide16 calls
    for other in (m, w, ms, o1, cs):
        assert lib.rc_encode_batch_wide16(C, other.handle, *enc_args) == N.RC_E_ARG
        assert lib.rc_decode_batch_wide16(C, other.handle, *dec_args) == N.RC_E_ARG
    # 16-bit symbols at an odd address
    odd = ctypes.c_void_p(syms.data_ptr() + 1)
    assert lib.rc_encode_batch_wide16(C, h, odd, p(off), 2, p(out), p(out_off), p(ol),
                                      p(fl)) == N.RC_E_ARG
    assert lib.rc_decode_batch_wide16(C, h, p(out), p(out_off), p(ol), odd, p(off), 2,
                                      p(fl)) == N.RC_E_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()  # nothing was launched
    with pytest.raises(TypeError):  # the Python mirror takes 16-bit tensors only
        rc.encode_batch_wide16(w16, syms, off, out, out_off)


# ---------------------------------------------------------------- 8. model building
@pytest.fixture(scope="module")
def odd_chunks():
    rng = np.random.default_rng(37)
    lens = 2 * rng.integers(0, 400, 37) + 1
    s = (rng.standard_normal(int(lens.sum())) * 3000).astype(np.int64) % 65536
    s[:4] = [0, 255, 256, 65535]
    s[lens[0]:lens[0] + 2] = [65535, 256]  # across a chunk start
    return s.astype(np.uint16), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def test_histogram16_is_bincount(ctx, odd_chunks):
    s, sym_off = odd_chunks
    for shift in (0, 1):  # 4-B aligned and 2-B aligned symbols
        syms, _keep = _sym_arena(s, shift)
        h = rc.histogram16(syms, dev(sym_off))
        assert h.shape == (65536,) and h.dtype == torch.int64
        assert np.array_equal(h.cpu().numpy(), np.bincount(s, minlength=65536))
    # chunks that leave symbols out
    part = np.array([3, 50, 50, 1001], np.int64)
    h = rc.histogram16(dev(s.view(np.int16)), dev(part)).cpu().numpy()
    assert np.array_equal(h, np.bincount(np.concatenate([s[3:50], s[50:1001]]), minlength=65536))


def test_build_wide16_model_round_trips_its_data(ctx, odd_chunks):
    s, sym_off = odd_chunks
    syms = dev(s.view(np.int16))
    model = rc.build_wide16_model(syms, dev(sym_off))
    assert model.n_symbols == 65536 and model.total == 65536
    assert ((model.c > 0) == (np.bincount(s, minlength=65536) > 0)).all()
    chunks = [s[sym_off[k]:sym_off[k + 1]] for k in range(len(sym_off) - 1)]
    codes = rc.encode_chunks_wide16(model, chunks)
    assert codes[0] == encode_ref(model.c, model.cum, model.total, chunks[0])[1]
    back = rc.decode_chunks_wide16(model, codes, [len(x) for x in chunks])
    assert all(np.array_equal(a, b) for a, b in zip(chunks, back))
    small = rc.build_wide16_model(syms, dev(sym_off), target_total=40000)
    assert small.total == 40000
    with pytest.raises(ValueError):  # a symbol outside the alphabet asked for
        rc.build_wide16_model(syms, dev(sym_off), n_symbols=65535)
    distinct = int((np.bincount(s, minlength=65536) > 0).sum())
    with pytest.raises(ValueError):  # more distinct symbols than the total
        rc.build_wide16_model(syms, dev(sym_off), target_total=distinct - 1)
    with pytest.raises(rc.ZeroFrequencyError):
        absent = int(np.flatnonzero(model.c == 0)[0])
        rc.encode_chunks_wide16(model, [[absent]])


# ---------------------------------------------------------------- 9. the C++ example
def test_cpp_wide16_impl(ctx):
    """examples/wide16_impl: a FreqTable over all 65536 symbols through rc::Wide16Model, against
    the per-call rc::Encoder given the same table, and back."""
    exe = os.path.join(ROOT, "examples", "wide16_impl")
    assert os.path.exists(exe), "examples/wide16_impl not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "round trip ok" in r.stdout and "test passed" in r.stdout
