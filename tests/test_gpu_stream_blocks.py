"""The two seams of the one-stream host calls' request blocks (rc_stream_encode_host /
rc_stream_decode_host, rc_resume.hip: EncBlock / DecBlock) against the C oracle's orc_stream_*:

- service / launch: the largest call whose block still fits the service's 64-KiB mailbox block
  and the next larger one, with the path each took read off rc_svc_probe_;
- one copy / two phases: encodes whose worst-case output lies on either side of 256 KiB, the
  early stop on a sticky flag among them (fewer counts come back than symbols went in);

and the order of the row encoder's checks where two of them hold for one symbol."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import dev  # noqa: E402

SVC_BLOCK = 64 << 10      # rc_resume.hip: the mailbox's request / result block
TWO_PHASE = 256 << 10     # rc_resume.hip, kTwoPhaseBytes: above it the bytes come back second
GUARD = 64


def a16(x):
    return (x + 15) & ~15


def enc_block_bytes(n, finish):
    """EncBlock: state | offsets | out_len | flags (128 B) | triples || nbytes | out"""
    need = N.stream_max_bytes(n, finish)
    return 128 + a16(12 * n) + a16(a16(n) + need)


def dec_block_bytes(n, fresh):
    """DecBlock: state | offsets | flags | c | cum (2160 B) | window || syms, the window being
    Decoder::new's 8 bytes on a fresh state and 12 per symbol (the code is long enough)"""
    return 2160 + a16((8 if fresh else 0) + 12 * n) + a16(n)


def largest_fitting(block_bytes):
    n = max(k for k in range(1, 8000) if block_bytes(k) <= SVC_BLOCK)
    assert block_bytes(n) <= SVC_BLOCK < block_bytes(n + 1)
    return n


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def service_calls(ctx):
    """the context's service calls since the last look (rc_svc_probe_'s out[0])"""
    fn = ctx._lib.rc_svc_probe_
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    fn.restype = ctypes.c_int
    out = (ctypes.c_uint64 * 5)()
    assert fn(ctx.handle, out) == N.RC_OK
    return int(out[0])


def fields(st):
    return tuple(getattr(st, f) for f, _ in N.StreamState._fields_)


def table(counts):
    c = np.asarray(counts, np.uint32)
    cum = np.concatenate([[0], np.cumsum(c.astype(np.uint64))[:-1]]).astype(np.uint32)
    return c, cum, int(c.astype(np.uint64).sum())


def triples(tab, syms):
    c, cum, total = tab
    s = np.asarray(syms, np.int64)
    return np.ascontiguousarray(np.stack([c[s], cum[s], np.full(len(s), total, np.uint32)], axis=1),
                                dtype=np.uint32)


def encode_host(ctx, st, trip, finish):
    """one rc_stream_encode_host call into guarded buffers: (status, bytes, counts, flags)"""
    n = len(trip)
    cap = N.stream_max_bytes(n, finish)
    out = np.full(cap + GUARD, 0xEE, np.uint8)
    nb = np.full(n + GUARD, 0xEE, np.uint8)
    ol, fl = ctypes.c_uint64(), ctypes.c_uint32()
    n0 = st.n
    status = ctx._lib.rc_stream_encode_host(ctx.handle, ctypes.byref(st), trip.ctypes.data, n,
                                            out.ctypes.data, cap, ctypes.byref(ol),
                                            nb.ctypes.data, finish, ctypes.byref(fl))
    got = st.n - n0
    assert (out[ol.value:] == 0xEE).all() and (nb[got:] == 0xEE).all()
    return status, out[:ol.value].tobytes(), nb[:got].tolist(), fl.value


def check_encode(ctx, trip, finish, warm=0):
    """the first `warm` symbols in one call, the rest in the call under test, against the oracle;
    returns the flag of the second call"""
    st, ref = N.StreamState.fresh(), cpu.Stream.fresh()
    if warm:
        status, b, nb, fl = encode_host(ctx, st, trip[:warm], 0)
        f, rb, rnb = cpu.stream_encode(ref, trip[:warm])
        assert (status, b, nb, fl) == (N.RC_OK, rb, rnb.tolist(), f) and f == 0
    status, b, nb, fl = encode_host(ctx, st, trip[warm:], finish)
    f, rb, rnb = cpu.stream_encode(ref, trip[warm:], finish=bool(finish))
    assert fl == f and status == (N.RC_E_CHUNK if f else N.RC_OK)
    assert b == rb and nb == rnb.tolist()  # bytes and out_len, counts and how many
    assert fields(st) == ref.tuple()
    return fl


def decode_host(ctx, st, tab, code, n):
    c, cum, total = tab
    out = np.full(n + GUARD, 0xEE, np.uint8)
    fl = ctypes.c_uint32()
    n0 = st.n
    status = ctx._lib.rc_stream_decode_host(ctx.handle, c.ctypes.data, cum.ctypes.data, len(c),
                                            total, ctypes.byref(st), code.ctypes.data, len(code),
                                            out.ctypes.data, n, ctypes.byref(fl))
    got = st.n - n0
    assert (out[got:] == 0xEE).all()
    return status, out[:got].tolist(), fl.value


ZIPF = table([1 + 60000 // (k + 1) for k in range(200)])


@pytest.mark.parametrize("finish", [0, 1])
def test_encode_service_launch_seam(knob_ctx, finish):
    ctx = knob_ctx(RC_STREAM_SERVICE=1)
    fit = largest_fitting(lambda n: enc_block_bytes(n, finish))
    assert 2600 < fit < 2630  # (o_nb + tail <= 65536 falls at 2616 symbols without finish)
    rng = np.random.default_rng(5 + finish)
    service_calls(ctx)
    for n, through_service in ((fit, 1), (fit + 1, 0)):
        trip = triples(ZIPF, rng.integers(0, 200, 7 + n))
        # (the 7 symbols before: a state in mid-stream; a small call, through the service)
        assert check_encode(ctx, trip, finish, warm=7) == 0
        assert service_calls(ctx) == 1 + through_service, n


@pytest.mark.parametrize("fresh", [True, False])
def test_decode_service_launch_seam(knob_ctx, fresh):
    ctx = knob_ctx(RC_STREAM_SERVICE=1)
    fit = largest_fitting(lambda n: dec_block_bytes(n, fresh))
    rng = np.random.default_rng(9 + fresh)
    warm = 0 if fresh else 5
    syms = rng.integers(0, 200, warm + fit + 1)
    _, code, _ = cpu.stream_encode(cpu.Stream.fresh(), triples(ZIPF, syms), finish=True)
    # bytes behind the stream, so that the window is the 12 bytes per symbol the layout allows
    code = np.frombuffer(code + bytes(12 * len(syms) + 64), np.uint8)
    service_calls(ctx)
    for n, through_service in ((fit, 1), (fit + 1, 0)):
        st, ref = N.StreamState.fresh(), cpu.Stream.fresh()
        if warm:  # a state in mid-stream: the window starts at its position
            status, got, fl = decode_host(ctx, st, ZIPF, code, warm)
            f, want = cpu.stream_decode(ref, *ZIPF, code, warm)
            assert (status, got, fl) == (N.RC_OK, want.tolist(), 0) and st.pos > 8
        status, got, fl = decode_host(ctx, st, ZIPF, code, n)
        f, want = cpu.stream_decode(ref, *ZIPF, code, n)
        assert (status, fl, f) == (N.RC_OK, 0, 0)
        assert got == want.tolist() == syms[warm:warm + n].tolist()
        assert fields(st) == ref.tuple()
        assert service_calls(ctx) == (1 if warm else 0) + through_service, n


# symbol 0 nearly always: few bytes written; symbol 3 has no frequency
SKEWED = table([(1 << 16) - 3, 2, 1, 0])


@pytest.mark.parametrize("service", [0, 1])
@pytest.mark.parametrize("n,finish,stop_at", [
    (21845, 0, None),    # 262,140 worst-case bytes: one copy of the whole region
    (21846, 0, None),    # 262,152: the state first, then the bytes written
    (21845, 1, None),    # 262,148 with finish's 8
    (21846, 0, 10923),   # two phases, a zero-frequency symbol in the middle: got < n counts
    (21845, 0, 10922),   # the same through the one copy
])
def test_encode_two_phase_seam(knob_ctx, service, n, finish, stop_at):
    need = N.stream_max_bytes(n, finish)
    assert (need > TWO_PHASE) == ((n, finish) != (21845, 0)) and abs(need - TWO_PHASE) <= 8
    ctx = knob_ctx(RC_STREAM_SERVICE=service)
    rng = np.random.default_rng(n + finish)
    syms = rng.choice(3, n, p=[0.98, 0.015, 0.005])
    if stop_at is not None:
        syms[stop_at] = 3
    st, ref = N.StreamState.fresh(), cpu.Stream.fresh()
    trip = triples(SKEWED, syms)
    status, b, nb, fl = encode_host(ctx, st, trip, finish)
    f, rb, rnb = cpu.stream_encode(ref, trip, finish=bool(finish))
    assert fl == f == (0 if stop_at is None else N.F_ZERO_FREQ)
    assert status == (N.RC_E_CHUNK if f else N.RC_OK)
    assert st.n == (n if stop_at is None else stop_at)
    assert b == rb and len(b) < need // 20
    assert nb == rnb.tolist()
    assert fields(st) == ref.tuple()
    assert service_calls(ctx) == 0  # (far above the mailbox's block: the launch path, always)


def test_row_encoder_check_order():
    """Two checks hold for one symbol: the row comes first, then the symbol, then the row's total
    (rc_stream_encode_rows, rc_rows.hip).  One stream of four symbols against two rows of four
    symbols, row 1 with total 0; test_gpu_rows.py has each check alone."""
    ctx = rc.default_context(0)
    c = np.array([[3, 1, 2, 2], [0, 0, 0, 0]], np.uint32)
    cum = np.array([[0, 3, 4, 6], [0, 0, 0, 0]], np.uint32)
    total = np.array([8, 0], np.uint32)
    T = tuple(dev(a.view(np.int32)) for a in (c, cum, total))
    ahead = triples((c[0], cum[0], 8), [2, 0])
    for row, sym, want in ((2, 4, N.F_BAD_MODEL),    # row >= n_rows and sym >= n_symbols
                           (1, 4, N.F_BAD_SYMBOL),   # sym >= n_symbols on the total == 0 row
                           (1, 3, N.F_BAD_MODEL)):   # the total == 0 row alone
        row_of = np.array([0, 0, row, 0], np.uint32)
        syms = np.array([2, 0, sym, 1], np.uint8)
        st = rc.stream_states(1)
        out = torch.full((48 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        nb = torch.full((4 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        ol, fl = rc.stream_encode_rows_batch(ctx, *T, dev(row_of.view(np.int32)), dev(syms), st,
                                             dev(np.array([0, 4], np.int64)), out,
                                             dev(np.array([0, 48], np.int64)), nbytes=nb)
        torch.cuda.synchronize()
        ref = cpu.Stream.fresh()
        f, rb, rnb = cpu.stream_encode(ref, ahead)  # the two symbols before it are encoded
        assert f == 0
        ref.flags = want
        assert int(fl[0]) == want, (row, sym)
        h, w = out.cpu().numpy(), int(ol[0])
        assert h[:w].tobytes() == rb and (h[w:] == 0xEE).all()
        assert nb.cpu().numpy().tolist() == rnb.tolist() + [0xEE] * (2 + GUARD)
        t = ref.tuple()
        assert t[4] == 2  # state.n counts the symbols before it only
        assert st.cpu().numpy().view(np.uint64)[0].tolist() == list(t[:5]) + [t[5] | t[6] << 32]
