"""Static chunk sets on the device: chunk k of a launch is coded exactly as the
single-table calls code it with row class_of[k].  Each case is checked three ways: against the
oracle with the chunk's row, against the library's own rc_encode_batch / rc_decode_batch with that
row's static model, and by the round trip.  Then the kernels that fit the classes, against NumPy,
and fit_chunk_set against tests/chunk_fit_ref.py."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from range_coder_rust_amd import model_build as MB  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import dev, ring_check_exact, ring_decode_at, run_decode, run_encode  # noqa: E402
import chunk_fit_cases as C  # noqa: E402
import chunk_fit_ref as R  # noqa: E402
import static_cases as S  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 300]
SENT = 0xEE


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def pad256(c):
    out = np.zeros(256, np.uint32)
    out[:len(c)] = c
    return out


def make_set(rows, total, ctx=None):
    c = np.ascontiguousarray(np.stack([pad256(r) for r in rows]), np.uint32)
    return rc.ChunkModelSet(c, None, total, ctx=ctx)


def draw_chunks(cs, class_of, seed, lengths=LENGTHS):
    """chunk k: symbols of its row's support, by the row's probabilities (a class id that names
    no row draws from row 0); the lengths cycle through `lengths`"""
    rng = np.random.default_rng(seed)
    out = []
    for k, r in enumerate(class_of):
        c = cs.c[r if r < cs.n_models else 0].astype(np.float64)
        L = lengths[int(rng.integers(0, len(lengths)))]
        out.append(rng.choice(256, L, p=c / c.sum()).astype(np.uint8))
    return out


def encode_cs(cs, class_of, chunks, caps, misalign=True, seed=0):
    """gpu_helpers.run_encode for a chunk set: ragged contiguous chunks, slots at an arbitrary
    alignment, the arena filled with a sentinel"""
    rng = np.random.default_rng(seed)
    lens = np.array([len(c) for c in chunks], np.int64)
    base_s = int(rng.integers(0, 16)) if misalign else 0
    sym_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + base_s
    syms = np.concatenate([rng.integers(0, 256, base_s).astype(np.uint8)] +
                          [np.asarray(c, np.uint8) for c in chunks] + [np.zeros(1, np.uint8)])
    caps = np.asarray(caps, np.int64)
    base_o = int(rng.integers(0, 16)) if misalign else 0
    out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + base_o
    out = torch.full((int(out_off[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_len, flags = rc.encode_batch_chunk_set(cs, dev(np.asarray(class_of, np.uint8)), dev(syms),
                                               dev(sym_off), out, dev(out_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:base_o] == SENT).all() and (h[out_off[-1]:] == SENT).all()
    return h, out_off, out_len.cpu().numpy(), flags.cpu().numpy()


def decode_cs(cs, class_of, codes, counts, misalign=True, seed=0):
    rng = np.random.default_rng(seed)
    n = len(codes)
    gaps = rng.integers(0, 16, n) if misalign else np.zeros(n, np.int64)
    coff = np.zeros(n, np.int64)
    parts, pos = [], 0
    for k, c in enumerate(codes):
        parts.append(rng.integers(0, 256, int(gaps[k])).astype(np.uint8))
        pos += int(gaps[k])
        coff[k] = pos
        parts.append(np.frombuffer(bytes(c), np.uint8))
        pos += len(c)
    parts.append(np.zeros(16, np.uint8))
    clen = np.array([len(c) for c in codes], np.int64)
    counts = np.asarray(counts, np.int64)
    base = int(rng.integers(0, 16)) if misalign else 0
    sym_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) + base
    syms = torch.full((int(sym_off[-1]) + 16,), SENT, dtype=torch.uint8, device="cuda")
    flags = rc.decode_batch_chunk_set(cs, dev(np.asarray(class_of, np.uint8)),
                                      dev(np.concatenate(parts)), dev(coff), dev(clen), syms,
                                      dev(sym_off))
    torch.cuda.synchronize()
    s = syms.cpu().numpy()
    assert (s[:base] == SENT).all() and (s[sym_off[-1]:] == SENT).all()
    return [s[sym_off[k]:sym_off[k + 1]] for k in range(n)], flags.cpu().numpy()


def check_three_ways(cs, class_of, chunks, seed=1):
    """the chunk-set calls against the oracle per chunk, against the single-table calls per row,
    and the round trip; every class id must name a row"""
    class_of = np.asarray(class_of, np.uint8)
    n = len(chunks)
    caps = [rc.slot_capacity(len(ch), cs.max_bits_per_symbol() + 1) for ch in chunks]
    out, out_off, ol, fl = encode_cs(cs, class_of, chunks, caps, seed=seed)
    want = [cpu.encode(cs.c[r], cs.cum[r], cs.total, ch) for r, ch in zip(class_of, chunks)]
    for k, (f, b, L) in enumerate(want):
        assert (fl[k], ol[k]) == (f, L), (k, class_of[k], fl[k], f, ol[k], L)
        if f == 0:
            assert bytes(out[out_off[k]:out_off[k] + L]) == b, (k, class_of[k])
    dec, fd = decode_cs(cs, class_of, [b for _, b, _ in want], [len(ch) for ch in chunks],
                        seed=seed + 1)
    launch = last_launch(cs)  # (the decoder's: lanes, LUT, workgroups)
    for k, ch in enumerate(chunks):
        if want[k][0] == 0:
            assert fd[k] == 0 and (dec[k] == ch).all(), (k, class_of[k], fd[k])
    for r in range(cs.n_models):  # the library's own single-table calls with that row
        ids = np.flatnonzero(class_of == r)
        if not len(ids):
            continue
        m = rc.StaticModel(cs.c[r], cs.cum[r], cs.total, ctx=cs.ctx)
        o1, off1, ol1, fl1 = run_encode(m, [chunks[k] for k in ids], [caps[k] for k in ids],
                                        misalign=True, seed=seed)
        for j, k in enumerate(ids):
            assert (fl1[j], ol1[j]) == (fl[k], ol[k]), (k, r)
            if fl[k] == 0:
                assert bytes(o1[off1[j]:off1[j] + ol1[j]]) == \
                    bytes(out[out_off[k]:out_off[k] + ol[k]]), (k, r)
        d1, fd1 = run_decode(m, [want[k][1] for k in ids], [len(chunks[k]) for k in ids],
                             misalign=True, seed=seed)
        for j, k in enumerate(ids):
            assert fd1[j] == fd[k] and (d1[j] == dec[k]).all(), (k, r)
        m.close()
    return launch


def last_launch(cs):
    """(lanes per workgroup, decoder LUT or 0 for an encoder, workgroups) of the context's last
    chunk-set coder launch"""
    out = (ctypes.c_uint32 * 3)()
    assert cs.ctx._lib.rc_chunk_last_(cs.ctx.handle, out) == N.RC_OK
    return int(out[0]), int(out[1]), int(out[2])


def rows_for(total):
    """three rows of the total from tests/static_cases.py tables, and rotations of them"""
    if total == 256:
        return [S.table("t256_flat")[0], S.table("t256_not_flat")[0],
                np.roll(pad256(S.table("t256_seam")[0]), 50)]
    if total == 65535:
        base = S.alloc(S.zipf_w(256), total)
        zeros = pad256(S.alloc(S.zeros_w("cs65535", 200), total))
        return [base, np.roll(base, 85), np.roll(zeros, 170)]
    names = {512: ("t512_seam",), 513: ("t513_seam", "t513_zeros"),
             2048: ("t2048_seam", "t2048_zeros"), 2049: ("t2049_seam",),
             65536: ("t65536_seam",)}[total]
    tabs = [pad256(S.table(nm)[0]) for nm in names]
    return [tabs[0], np.roll(tabs[0], 85), np.roll(tabs[-1], 170)]


@pytest.mark.parametrize("total", (256, 512, 513, 2048, 2049, 65535, 65536))
def test_every_class_seam(ctx, total):
    cs = make_set(rows_for(total), total)
    k = np.arange(1300, dtype=np.uint64)
    class_of = ((k * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(3)).astype(np.uint8)
    W, lut, grid = check_three_ways(cs, class_of, draw_chunks(cs, class_of, total),
                                    seed=total & 0xFF)
    want_lut, want_w = (2, 256) if total <= 512 else (1, 256) if total <= 2048 else \
        (4, 256) if total == 2049 else (4, 512)
    assert (W, lut, grid) == (want_w, want_lut, (1300 + want_w - 1) // want_w + 3)
    cs.close()


def zipf_rows(k, total):
    base = S.alloc(S.zipf_w(256), total)
    return [np.roll(base, (j * 256) // k) for j in range(k)]


@pytest.mark.parametrize("total,W,lut,pair", ((4096, 256, 4, "0"), (65536, 512, 4, "4"),
                                              (65536, 1024, 6, "6")))
def test_workgroup_seams(ctx, knob_ctx, total, W, lut, pair):
    """class sizes {0, 1, W, W + 1} for the decoder's workgroup size W (256 and 512 lanes of the
    buckets, 1,024 of the q-to-symbol table; the encoder's is 256: classes of W and W + 1 are
    whole and whole-plus-one workgroups of its too), then all chunks in one class, one row, and
    the empty launch in both directions"""
    kctx = knob_ctx(RC_DEC_PAIR=pair)
    cs = make_set(zipf_rows(4, total), total, ctx=kctx)
    rng = np.random.default_rng(W)
    class_of = rng.permutation(np.repeat([1, 2, 3], [1, W, W + 1]).astype(np.uint8))
    assert check_three_ways(cs, class_of, draw_chunks(cs, class_of, 1)) == \
        (W, lut, (2 * W + 2 + W - 1) // W + 4)
    one = np.full(300, 2, np.uint8)
    check_three_ways(cs, one, draw_chunks(cs, one, 2))
    cs.close()
    cs1 = make_set(zipf_rows(1, total), total, ctx=kctx)
    zero = np.zeros(300, np.uint8)
    check_three_ways(cs1, zero, draw_chunks(cs1, zero, 3))
    # n_chunks = 0: accepted, nothing touched
    byte, off = dev(np.zeros(1, np.uint8)), dev(np.zeros(1, np.int64))
    buf = torch.full((64,), SENT, dtype=torch.uint8, device="cuda")
    ol, fl = rc.encode_batch_chunk_set(cs1, byte, byte, off, buf, off)
    fd = rc.decode_batch_chunk_set(cs1, byte, byte, off[:0], off[:0], buf, off)
    torch.cuda.synchronize()
    assert ol.numel() == 0 and fl.numel() == 0 and fd.numel() == 0
    assert (buf.cpu().numpy() == SENT).all()
    cs1.close()


def test_64_classes_one_chunk_each(ctx):
    cs = make_set(zipf_rows(64, 65536), 65536)
    class_of = np.random.default_rng(64).permutation(64).astype(np.uint8)
    check_three_ways(cs, class_of, draw_chunks(cs, class_of, 64))
    cs.close()


def test_the_row_is_really_used(ctx):
    """symbol 7 has c = 0 in row 0 only: a chunk holding a 7 is RC_F_ZERO_FREQ in class 0 and codes
    in class 1, and its neighbours stay bit-exact"""
    base = S.alloc(S.zipf_w(256), 4096)
    r0 = base.copy()
    r0[8] += r0[7]
    r0[7] = 0
    cs = make_set([r0, base], 4096)
    rng = np.random.default_rng(7)
    chunks = [rng.choice(np.r_[0:7, 8:256], 100).astype(np.uint8) for _ in range(9)]
    chunks[4][50] = 7
    for cls4, flag in ((0, N.F_ZERO_FREQ), (1, 0)):
        class_of = np.array([0, 1, 0, 1, cls4, 0, 1, 0, 1], np.uint8)
        caps = [rc.slot_capacity(100, 13) for _ in chunks]
        out, out_off, ol, fl = encode_cs(cs, class_of, chunks, caps, seed=cls4)
        for k, ch in enumerate(chunks):
            f, b, L = cpu.encode(cs.c[class_of[k]], cs.cum[class_of[k]], 4096, ch)
            assert fl[k] == f == (flag if k == 4 else 0), (k, fl[k], f)
            if f == 0:
                assert ol[k] == L and bytes(out[out_off[k]:out_off[k] + L]) == b, k
    cs.close()


@pytest.mark.parametrize("alone", (False, True))
def test_bad_class_ids(ctx, alone):
    """ids K and 255: RC_F_BAD_MODEL, the slot and the symbols untouched, every other chunk exact"""
    cs = make_set(zipf_rows(3, 4096), 4096)
    if alone:
        class_of = np.array([3], np.uint8)
    else:
        class_of = (np.arange(200) % 3).astype(np.uint8)
        class_of[[37, 100]] = (3, 255)  # (in the middle of a wave)
    bad = np.flatnonzero(class_of >= 3)
    chunks = draw_chunks(cs, class_of, 5, [64, 65, 17])
    caps = [rc.slot_capacity(len(ch), 13) for ch in chunks]
    out, out_off, ol, fl = encode_cs(cs, class_of, chunks, caps, seed=3)
    codes = []
    for k, ch in enumerate(chunks):
        if k in bad:
            assert (fl[k], ol[k]) == (N.F_BAD_MODEL, 0), (k, fl[k], ol[k])
            assert (out[out_off[k]:out_off[k + 1]] == SENT).all(), k
            codes.append(b"\0" * 16)
            continue
        f, b, L = cpu.encode(cs.c[class_of[k]], cs.cum[class_of[k]], 4096, ch)
        assert (fl[k], ol[k]) == (0, L) and bytes(out[out_off[k]:out_off[k] + L]) == b, k
        codes.append(b)
    dec, fd = decode_cs(cs, class_of, codes, [len(ch) for ch in chunks], seed=4)
    for k, ch in enumerate(chunks):
        if k in bad:
            assert fd[k] == N.F_BAD_MODEL and (dec[k] == SENT).all(), (k, fd[k])
        else:
            assert fd[k] == 0 and (dec[k] == ch).all(), k
    cs.close()


def test_capacity(ctx):
    """slots cut short among exact ones: RC_F_CAPACITY with the exact length, the first cap bytes
    the oracle's, as the static encoder gives"""
    cs = make_set(zipf_rows(3, 65536), 65536)
    class_of = (np.arange(40) % 3).astype(np.uint8)
    chunks = draw_chunks(cs, class_of, 9, [64, 129, 300])
    want = [cpu.encode(cs.c[r], cs.cum[r], 65536, ch) for r, ch in zip(class_of, chunks)]
    short = {1: 1, 6: 1, 13: 17, 20: 1, 39: 17}
    caps = [L - short.get(k, 0) for k, (_, _, L) in enumerate(want)]
    out, out_off, ol, fl = encode_cs(cs, class_of, chunks, caps, seed=2)
    for k, (f, b, L) in enumerate(want):
        assert ol[k] == L and fl[k] == (N.F_CAPACITY if k in short else 0), (k, fl[k], ol[k], L)
        assert bytes(out[out_off[k]:out_off[k] + caps[k]]) == b[:caps[k]], k
    cs.close()


def test_bad_streams(ctx):
    """64 garbage streams, and sound streams cut short, per row, on tables with zeros: flags and
    symbols are the oracle's for that row"""
    name = "t2048_zeros"
    tab = pad256(S.table(name)[0])
    cs = make_set([tab, np.roll(tab, 31), np.roll(tab, 100)], 2048)
    codes, counts = S.garbage(name)
    class_of = (np.arange(len(codes)) % 3).astype(np.uint8)
    chunks = draw_chunks(cs, class_of, 12, [64, 65, 300])
    cut = []
    for r, ch, x in zip(class_of, chunks, S.cuts(name)):
        _, b, L = cpu.encode(cs.c[r], cs.cum[r], 2048, ch)
        cut.append(b[:max(8, L - int(x))])
    assert len(cut) >= 32  # (one cut per chunk of the case: fewer than the garbage streams)
    for streams, ns in ((codes, counts), (cut, [len(ch) for ch in chunks[:len(cut)]])):
        dec, fd = decode_cs(cs, class_of[:len(streams)], streams, ns, seed=6)
        for k, r in enumerate(class_of[:len(streams)]):
            f, d = cpu.decode(cs.c[r], cs.cum[r], 2048, streams[k], ns[k])
            assert fd[k] == f, (k, r, fd[k], f)
            if f == 0:
                assert (dec[k] == d).all(), (k, r)
    cs.close()


@pytest.mark.parametrize("env,launch", (({"RC_DEC_PAIR": "6"}, (1024, 6, 5)),
                                        ({"RC_DEC_PAIR": "4"}, (512, 4, 6)),
                                        ({"RC_DEC_PAIR": "1024"}, (512, 4, 6)),
                                        ({"RC_PRIO": "off"}, (512, 4, 6))))
def test_decoder_variants(ctx, knob_ctx, env, launch):
    """RC_DEC_PAIR=6 runs the direct q-to-symbol table (1,024 lanes) at a small size, =4 the
    buckets, =1024 finds no pair table and runs the buckets; RC_PRIO=off"""
    cs = make_set(zipf_rows(3, 65536), 65536, ctx=knob_ctx(**env))
    class_of = (np.arange(1100) % 3).astype(np.uint8)
    class_of[:40] = 1
    got = check_three_ways(cs, class_of, draw_chunks(cs, class_of, 21, [0, 17, 64, 65, 130]))
    assert got == launch  # (lanes, LUT, workgroups: which decoder the switch really selected)
    cs.close()


@pytest.mark.parametrize("pair", ("0", "6", "4"))
@pytest.mark.parametrize("name", ("pow2", "magic"))
def test_tight_ring_fixtures(ctx, knob_ctx, name, pair):
    """tests/golden/ring_tight.json as four identical rows with scattered classes: the grouped
    decoder runs the static ring schedule position for position, so every stream decodes
    byte-exact at its own head and at the others'"""
    with open(os.path.join(HERE, "golden", "ring_tight.json")) as f:
        fx = json.load(f)
    md = fx["models"][name]
    c = np.array(md["c"], np.uint32)
    cs = make_set([c] * 4, md["total"], ctx=knob_ctx(RC_DEC_PAIR=pair))
    chunks = [ch for ch in fx["chunks"] if ch["model"] == name]
    class_of = dev(((np.arange(len(chunks)) * 7 + 3) % 4).astype(np.uint8))
    for head in sorted({ch["head"] for ch in chunks} | {16, 48}):
        s, sym_off, flags = ring_decode_at(
            lambda *a: rc.decode_batch_chunk_set(cs, class_of, *a), chunks, (64 - head) % 64)
        ring_check_exact(s, sym_off, flags, chunks)
    cs.close()


@pytest.mark.parametrize("W", (256, 512, 1024))
def test_device_grouping_is_the_rule(ctx, W):
    """the device step writes what the host mirror of the rule writes: stable, padded, ~0 marks"""
    rng = np.random.default_rng(W)
    for n, K in ((0, 3), (1, 1), (5000, 64), (3 * W + 1, 4), (2048 * 3 + 77, 7)):
        cls = rng.integers(0, K + 2, max(n, 1)).astype(np.uint8)[:n]
        grid = (n + W - 1) // W + K
        order = np.zeros(grid * W, np.uint32)
        wg_row = np.zeros(grid, np.uint32)
        L = N.load()
        assert L.rc_chunk_group_plan_(ctypes.c_void_p(cls.ctypes.data) if n else None, n, K, W,
                                      ctypes.c_void_p(order.ctypes.data),
                                      ctypes.c_void_p(wg_row.ctypes.data)) == N.RC_OK
        d_cls = dev(cls if n else np.zeros(1, np.uint8))
        d_order = torch.zeros(grid * W, dtype=torch.int32, device="cuda")
        d_row = torch.zeros(grid, dtype=torch.int32, device="cuda")
        d_flags = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        ctx.bind_stream()
        assert L.rc_chunk_group_(ctx.handle, rc.api._ptr(d_cls), n, K, W, rc.api._ptr(d_order),
                                 rc.api._ptr(d_row), rc.api._ptr(d_flags)) == N.RC_OK
        torch.cuda.synchronize()
        assert np.array_equal(d_order.cpu().numpy().view(np.uint32), order), (n, K, W)
        assert np.array_equal(d_row.cpu().numpy().view(np.uint32), wg_row), (n, K, W)
        assert np.array_equal(d_flags.cpu().numpy()[:n] == N.F_BAD_MODEL, cls >= K)


def test_a_context_that_changes_streams(ctx):
    """two chunk-set launches of different sizes on one context under two torch streams, the
    second issued while the first still runs: the context's grouping scratch is ordered between
    the streams (a launch on another stream waits for the last launch's coder before it
    regroups), so both code what they code alone"""
    cs = make_set(zipf_rows(5, 65536), 65536)
    rng = np.random.default_rng(2)
    jobs = []
    for n, L in ((6000, 3000), (700, 64)):  # (a long launch, then a short one of another shape)
        class_of = rng.integers(0, 5, n).astype(np.uint8)
        p = cs.c[0].astype(np.float64)
        syms = rng.choice(256, n * L, p=p / p.sum()).astype(np.uint8)
        cap = rc.slot_capacity(L, 17.0)
        jobs.append((dev(class_of), dev(syms), dev(np.arange(n + 1, dtype=np.int64) * L),
                     dev(np.arange(n + 1, dtype=np.int64) * cap), n, cap))
    alone = []
    for cls, syms, so, oo, n, cap in jobs:
        out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        ol, fl = rc.encode_batch_chunk_set(cs, cls, syms, so, out, oo)
        torch.cuda.synchronize()
        assert int(fl.abs().sum()) == 0
        alone.append((out, ol))
    for rep in range(3):
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        got = []
        for st, (cls, syms, so, oo, n, cap) in zip(streams, jobs):
            with torch.cuda.stream(st):
                out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
                ol, fl = rc.encode_batch_chunk_set(cs, cls, syms, so, out, oo)
                dec = torch.zeros_like(syms)
                fd = rc.decode_batch_chunk_set(cs, cls, out, oo[:-1].contiguous(), ol, dec, so)
                got.append((out, ol, fl, fd, dec))
        torch.cuda.synchronize()
        for (out, ol, fl, fd, dec), (want, wl), job in zip(got, alone, jobs):
            assert int(fl.abs().sum()) == 0 and int(fd.abs().sum()) == 0, rep
            assert torch.equal(ol, wl) and torch.equal(out, want), rep
            assert torch.equal(dec, job[1]), rep
    cs.close()


def test_cpp_chunk_set_impl(ctx):
    """examples/chunk_set_impl: four chunks against two FreqTables through rc::ChunkSet, against
    the per-call rc::Encoder given each chunk's table; rc::cost_table"""
    exe = os.path.join(os.path.dirname(HERE), "examples", "chunk_set_impl")
    assert os.path.exists(exe), "examples/chunk_set_impl not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test passed" in r.stdout


# ---------------------------------------------------------------------------- fitting
def cost_rows(K, n_symbols, rng, none_at=()):
    t = rng.integers(0, 1 << 20, (K, n_symbols)).astype(np.uint32)
    for r, s in none_at:
        t[r % K, s] = R.COST_NONE
    return t


@pytest.mark.parametrize("n_symbols", (256, 100))
@pytest.mark.parametrize("K", (1, 8, 64))
def test_costs_and_class_sums_match_numpy(ctx, K, n_symbols):
    rng = np.random.default_rng(K * 1000 + n_symbols)
    for n in (0, 1, 65, 1300):
        h = np.zeros((max(n, 1), 256), np.int32)
        h[:, :n_symbols] = rng.integers(0, 5000, (max(n, 1), n_symbols))
        h[:, 3] = 0  # a COST_NONE entry nobody hits ...
        h[::5, 9] = 0
        t = cost_rows(K, n_symbols, rng, none_at=((0, 3), (1, 3), (0, 9), (K - 1, 9)))
        if K > 1:
            t[1] = t[0]  # ... and ties: rows 0 and 1 cost the same
        h = h[:n]
        best, cost, costs = MB.chunk_set_costs(dev(h.reshape(-1, 256)) if n else
                                               torch.zeros((0, 256), dtype=torch.int32,
                                                           device="cuda"), t, all_costs=True)
        torch.cuda.synchronize()
        want = R.chunk_costs(h, list(t))
        wb, wc = R.assign(h, list(t))
        assert np.array_equal(costs.cpu().numpy().view(np.uint64).reshape(n, K), want), (n, K)
        assert np.array_equal(best.cpu().numpy(), wb) and \
            np.array_equal(cost.cpu().numpy().view(np.uint64), wc), (n, K)
        if n >= 65:  # (both kinds of COST_NONE entry occur: one that is hit, one that is not)
            assert (want == np.iinfo(np.uint64).max).any() and (wc != np.iinfo(np.uint64).max).any()
        cls = rng.integers(0, K + 3, max(n, 1)).astype(np.uint8)[:n]  # (ids >= K are skipped)
        into = torch.full((K, 256), 5, dtype=torch.int64, device="cuda")  # ADDED into
        if n:
            MB.histogram_by_class(dev(h), dev(cls), K, class_hist=into)
            torch.cuda.synchronize()
        assert np.array_equal(into.cpu().numpy().view(np.uint64), R.by_class(h, cls, K) + 5), (n, K)


_fit_ref = {}


def fit_case(name):
    """the mixture on the device, its reference fits (computed once) and the quantiser"""
    if name not in _fit_ref:
        chunks, labels = C.two_source() if name == "two" else C.four_source()
        _fit_ref[name] = (chunks, labels, {})
    return _fit_ref[name]


def lib_quant(counts):
    return MB.quantize_counts(np.asarray(counts, np.uint64), 1 << 16, all_symbols=True)[0]


@pytest.mark.parametrize("K", (2, 4, 8))
@pytest.mark.parametrize("name", ("two", "four"))
def test_fit_equals_the_reference(ctx, name, K):
    chunks, labels, refs = fit_case(name)
    n, L = chunks.shape
    syms = dev(chunks.reshape(-1))
    sym_off = dev(np.arange(n + 1, dtype=np.int64) * L)
    cs, cls = rc.fit_chunk_set(syms, sym_off, n_models=K)
    torch.cuda.synchronize()
    if K not in refs:  # (the library's own host cost table: see chunk_fit_ref's docstring)
        refs[K] = R.fit(C.histograms(chunks), K, 1 << 16, 8, lib_quant, cost_table=MB.cost_table)
    rows, want = refs[K]
    assert np.array_equal(cs.c, rows), (name, K)
    assert np.array_equal(cls.cpu().numpy(), want), (name, K)
    if name == "two" and K == 2:
        assert np.array_equal(want, labels) or np.array_equal(want, 1 - labels)
        # coded bytes under the fitted set against build_model's single table
        cap = rc.slot_capacity(L, 16.0)
        out_off = dev(np.arange(n + 1, dtype=np.int64) * cap)
        out = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
        ol2, fl2 = rc.encode_batch_chunk_set(cs, cls, syms, sym_off, out, out_off)
        m = rc.build_model(syms, sym_off)
        ol1, fl1 = rc.encode_batch(m, syms, sym_off, out, out_off)
        torch.cuda.synchronize()
        assert int(fl1.abs().sum()) == 0 and int(fl2.abs().sum()) == 0
        b1, b2 = int(ol1.sum()), int(ol2.sum())
        print(f"coded bytes: one table {b1}, fitted K=2 set {b2} ({b2 / b1:.4f})")
        assert b2 < b1
    cs.close()
