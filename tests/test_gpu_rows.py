"""rc_stream_decode_rows / rc_stream_encode_rows on the GPU (rc_rows.hip) against the reference of
tests/rows_ref.py: byte-exact, and state-exact on all seven state fields.  Every alphabet size at
a ballot-group seam, 64-symbol block seams, every code alignment mod 16, resumption through carried
states, identity with the one-table kernels, inconsistent tables, every error at the block seams,
garbage streams, and guard bytes around everything the kernels write."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import dev  # noqa: E402
import rows_ref as RR  # noqa: E402

M64 = (1 << 64) - 1
LENS = (0, 1, 63, 64, 65, 200)  # symbols per stream: the 64-symbol block seams
GUARD_FLAG = cpu.F_TRUNCATED    # the sticky flag of the guard streams (the kernels skip them)


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def dtab(tab):
    """the table in exactly sized device tensors"""
    return tuple(dev(np.ascontiguousarray(a).view(np.int32)) for a in tab)


def fresh(n):
    st = np.zeros((n, 6), np.uint64)
    st[:, 1] = M64
    return st


def as_stream(row):
    lo, r, d, pos, n, fs = (int(x) for x in row)
    return cpu.Stream(lo, r, d, pos, n, fs & 0xFFFFFFFF, fs >> 32)


def as_row(st):
    t = st.tuple()
    return np.array(list(t[:5]) + [t[5] | t[6] << 32], np.uint64)


def _guarded_states(st_in, guards):
    """the states on the device between two 0xEE rows; with guards, a flagged stream behind every
    real one.  Returns (whole tensor, the slice the call gets, host copy of the slice)."""
    n = len(st_in)
    rows = []
    for k in range(n):
        rows.append(st_in[k])
        if guards:
            rows.append(np.array([0, M64, 0, 0, 0, GUARD_FLAG | 1 << 32], np.uint64))
    body = np.array(rows, np.uint64).reshape(-1, 6)
    ee = np.full((1, 6), 0xEEEEEEEEEEEEEEEE, np.uint64)
    whole = dev(np.concatenate([ee, body, ee]).view(np.int64))
    return whole, whole[1:1 + len(body)], body


def _check_guarded_states(whole, body, guards):
    h = whole.cpu().numpy().view(np.uint64)
    assert (h[0] == 0xEEEEEEEEEEEEEEEE).all() and (h[-1] == 0xEEEEEEEEEEEEEEEE).all()
    got = h[1:-1]
    if guards:
        assert np.array_equal(got[1::2], body[1::2]), "a guard stream's state changed"
        return got[0::2]
    return got


def _interleave(lens, guards):
    """symbol counts of the launch's streams, 64 guard symbols behind every real stream"""
    out = []
    for L in lens:
        out.append(int(L))
        if guards:
            out.append(64)
    off = np.zeros(len(out) + 1, np.int64)
    off[1:] = np.cumsum(out)
    return off, (2 if guards else 1)


def gpu_decode(ctx, T, rows, codes, st_in=None, guards=True):
    """One rc_stream_decode_rows launch: stream k decodes len(rows[k]) symbols from codes[k], which
    lies at alignment k mod 16 in an exactly sized arena.  Returns (the symbol slot of every
    stream, flags, states) after checking every guard."""
    n = len(rows)
    st_in = fresh(n) if st_in is None else st_in
    sym_off, step = _interleave([len(r) for r in rows], guards)
    row_of = np.zeros(max(int(sym_off[-1]), 1), np.uint32)
    for k, r in enumerate(rows):
        row_of[sym_off[step * k]: sym_off[step * k] + len(r)] = r
    blob, coff, clen = bytearray(), np.zeros(step * n, np.int64), np.zeros(step * n, np.int64)
    for k, c in enumerate(codes):
        blob += b"\xa5" * ((k % 16 - len(blob)) % 16)
        coff[step * k], clen[step * k] = len(blob), len(c)
        blob += c
    blob = np.frombuffer(bytes(blob) or b"\0", np.uint8)
    syms = torch.full((int(sym_off[-1]) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    whole, sts, body = _guarded_states(st_in, guards)
    flags = torch.full((step * n + 16,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
    rc.stream_decode_rows_batch(ctx, *T, dev(row_of.view(np.int32)), sts, dev(blob), dev(coff),
                                dev(clen), syms, dev(sym_off), flags=flags)
    torch.cuda.synchronize()
    h, fl = syms.cpu().numpy(), flags.cpu().numpy()
    assert (h[sym_off[-1]:] == 0xEE).all() and (fl[step * n:] == 0x6E6E6E6E).all()
    if guards:
        for k in range(n):
            assert (h[sym_off[2 * k + 1]: sym_off[2 * k + 2]] == 0xEE).all(), k
        assert (fl[1:2 * n:2] == GUARD_FLAG).all()
    slots = [h[sym_off[step * k]: sym_off[step * k + 1]] for k in range(n)]
    return slots, fl[0:step * n:step].astype(np.uint32), _check_guarded_states(whole, body, guards)


def gpu_encode(ctx, T, rows, syms, finish, st_in=None, guards=True, slack=0):
    """One rc_stream_encode_rows launch with nbytes.  Output slots of RC_STREAM_MAX_BYTES + slack
    and 64 guard bytes each.  Returns (new bytes, byte counts, flags, states)."""
    n = len(rows)
    st_in = fresh(n) if st_in is None else st_in
    sym_off, step = _interleave([len(r) for r in rows], guards)
    tot = max(int(sym_off[-1]), 1)
    row_of, sy = np.zeros(tot, np.uint32), np.zeros(tot, np.uint8)
    for k, (r, s) in enumerate(zip(rows, syms)):
        row_of[sym_off[step * k]: sym_off[step * k] + len(r)] = r
        sy[sym_off[step * k]: sym_off[step * k] + len(r)] = s
    caps = np.diff(sym_off) * 12 + (8 if finish else 0) + slack
    out_off = np.zeros(step * n + 1, np.int64)
    out_off[1:] = np.cumsum(caps + 64)
    out = torch.full((int(out_off[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
    nb = torch.full((tot + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    whole, sts, body = _guarded_states(st_in, guards)
    ol, fl = rc.stream_encode_rows_batch(ctx, *T, dev(row_of.view(np.int32)), dev(sy), sts,
                                         dev(sym_off), out, dev(out_off), nbytes=nb, finish=finish)
    torch.cuda.synchronize()
    h, ol, fl, nbh = out.cpu().numpy(), ol.cpu().numpy(), fl.cpu().numpy(), nb.cpu().numpy()
    st = _check_guarded_states(whole, body, guards)
    assert (nbh[sym_off[-1]:] == 0xEE).all()
    codes, counts = [], []
    for k in range(n):
        j = step * k
        assert ol[j] <= caps[j]
        assert (h[out_off[j] + ol[j]: out_off[j + 1]] == 0xEE).all(), k
        codes.append(h[out_off[j]: out_off[j] + ol[j]].tobytes())
        done = int(st[k, 4]) - int(st_in[k, 4])
        assert (nbh[sym_off[j] + done: sym_off[j + 1]] == 0xEE).all(), k
        counts.append(nbh[sym_off[j]: sym_off[j] + done].tolist())
        if guards:
            assert (h[out_off[j + 1]: out_off[j + 2]] == 0xEE).all() and ol[j + 1] == 0
            assert (nbh[sym_off[j + 1]: sym_off[j + 2]] == 0xEE).all()
            assert fl[j + 1] == GUARD_FLAG
    return codes, counts, fl[0:step * n:step].astype(np.uint32), st


def ref_decode(tab, rows, code, st_row=None):
    st = cpu.Stream.fresh() if st_row is None else as_stream(st_row)
    f, s = RR.decode_rows(st, *tab, rows, code)
    return f, s, as_row(st)


def ref_encode(tab, rows, syms, finish, st_row=None, cap=None):
    st = cpu.Stream.fresh() if st_row is None else as_stream(st_row)
    f, b, nb = RR.encode_rows(st, *tab, rows, syms, finish=finish, cap=cap)
    return f, b, nb.tolist(), as_row(st)


def check_decode(got, want, what=""):
    slots, fl, st = got
    for k, (f, s, row) in enumerate(want):
        assert fl[k] == f, (what, k, fl[k], f)
        assert slots[k][:len(s)].tolist() == s.tolist(), (what, k)
        assert (slots[k][len(s):] == 0xEE).all(), (what, k)
        assert st[k].tolist() == row.tolist(), (what, k, st[k], row)


def check_encode(got, want, what=""):
    codes, counts, fl, st = got
    for k, (f, b, nb, row) in enumerate(want):
        assert fl[k] == f, (what, k, fl[k], f)
        assert codes[k] == b and counts[k] == nb, (what, k)
        assert st[k].tolist() == row.tolist(), (what, k, st[k], row)


def _streams(tab, seed, n_streams=67, rare=False):
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, RR.N_ROWS, LENS[k % len(LENS)]).astype(np.uint32)
            for k in range(n_streams)]
    syms = [RR.live_symbols(tab[0], r, rng, rare_bias=rare) for r in rows]
    return rows, syms


@pytest.mark.parametrize("shape", ["mixed", "rare"])
@pytest.mark.parametrize("n_symbols", RR.SIZES)
def test_round_trip_against_the_reference(ctx, n_symbols, shape):
    """67 streams of 0 / 1 / 63 / 64 / 65 / 200 symbols against 37 rows: one launch of 67, of 3
    and of 1 streams, and the same streams cut into 1 to 5 calls each."""
    tab = (RR.mixed_table if shape == "mixed" else RR.rare_table)(n_symbols, 100 + n_symbols)
    T = dtab(tab)
    rows, syms = _streams(tab, 40 + n_symbols, rare=shape == "rare")
    want_e = [ref_encode(tab, r, s, True) for r, s in zip(rows, syms)]
    assert all(w[0] == 0 for w in want_e)
    codes = [w[1] for w in want_e]
    want_d = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    assert all(w[0] == 0 and w[1].tolist() == s.tolist() for w, s in zip(want_d, syms))
    for ns in (67, 3, 1):
        g = ns != 67  # (guard streams behind every stream of the small launches)
        check_encode(gpu_encode(ctx, T, rows[:ns], syms[:ns], True, guards=g), want_e[:ns], ns)
        check_decode(gpu_decode(ctx, T, rows[:ns], codes[:ns], guards=g), want_d[:ns], ns)
    # resumption: every stream cut at random symbol indexes into 1 to 5 calls
    rng = np.random.default_rng(n_symbols)
    cuts = []
    for r in rows:
        inner = sorted(rng.integers(0, len(r) + 1, int(rng.integers(0, 5))).tolist())
        cuts.append([0] + inner + [len(r)] * (5 - len(inner)))
    st_e, st_d = fresh(67), fresh(67)
    got_b, got_nb, got_s = [b""] * 67, [[] for _ in rows], [[] for _ in rows]
    for part in range(5):
        pr = [r[c[part]:c[part + 1]] for r, c in zip(rows, cuts)]
        ps = [s[c[part]:c[part + 1]] for s, c in zip(syms, cuts)]
        cs, nbs, fl, st_e = gpu_encode(ctx, T, pr, ps, part == 4, st_in=st_e, guards=False,
                                       slack=part)
        assert not fl.any()
        slots, fl, st_d = gpu_decode(ctx, T, pr, codes, st_in=st_d, guards=False)
        assert not fl.any()
        for k in range(67):
            got_b[k] += cs[k]
            got_nb[k] += nbs[k]
            got_s[k] += slots[k].tolist()
    for k in range(67):
        assert got_b[k] == codes[k] and got_nb[k] == want_e[k][2], k
        assert st_e[k].tolist() == want_e[k][3].tolist(), k
        assert got_s[k] == syms[k].tolist() and st_d[k].tolist() == want_d[k][2].tolist(), k


@pytest.mark.parametrize("n_symbols", [2, 65, 256])
def test_one_row_equals_the_one_table_kernels(ctx, n_symbols):
    """Every row_of = 0: symbols, flags and states are rc_stream_decode's on row 0; the encoder's
    bytes, counts and states are rc_stream_encode's on the gathered triples."""
    tab = RR.mixed_table(n_symbols, 100 + n_symbols)
    T = dtab(tab)
    rng = np.random.default_rng(7)
    rows = [np.zeros(L, np.uint32) for L in (200, 65, 0, 64, 1)]
    syms = [RR.live_symbols(tab[0], r, rng) for r in rows]
    n = len(rows)
    for finish in (True, False):
        codes, counts, fl, st = gpu_encode(ctx, T, rows, syms, finish, guards=False)
        sym_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        trip = np.concatenate([RR.gather(*tab, r, s)[2] for r, s in zip(rows, syms)])
        caps = np.diff(sym_off) * 12 + (8 if finish else 0)
        out_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        out = torch.zeros(int(out_off[-1]) + 16, dtype=torch.uint8, device="cuda")
        nb = torch.zeros(int(sym_off[-1]) + 1, dtype=torch.uint8, device="cuda")
        states = rc.stream_states(n)
        ol, fl1 = rc.stream_encode_batch(ctx, states, dev(trip.reshape(-1).view(np.int32)),
                                         dev(sym_off), out, dev(out_off), nbytes=nb, finish=finish)
        torch.cuda.synchronize()
        h, ol, nbh = out.cpu().numpy(), ol.cpu().numpy(), nb.cpu().numpy()
        st1 = states.cpu().numpy().view(np.uint64)
        assert fl.tolist() == fl1.cpu().numpy().astype(np.uint32).tolist()
        assert np.array_equal(st, st1)
        for k in range(n):
            assert codes[k] == h[out_off[k]: out_off[k] + ol[k]].tobytes(), k
            assert counts[k] == nbh[sym_off[k]: sym_off[k] + len(counts[k])].tolist(), k
    # decode: valid streams (finish) and two garbage ones
    codes = [ref_encode(tab, r, s, True)[1] for r, s in zip(rows, syms)]
    codes[1] = bytes(rng.integers(0, 256, 90).astype(np.uint8))
    codes[3] = b"\xff" * 30
    slots, fl, st = gpu_decode(ctx, T, rows, codes, guards=False)
    clen = np.array([len(c) for c in codes], np.int64)
    coff = np.concatenate([[0], np.cumsum(clen)[:-1]]).astype(np.int64)
    sym_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    out = torch.full((int(sym_off[-1]) + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    states = rc.stream_states(n)
    fl1 = rc.stream_decode_batch(ctx, dev(tab[0][0].view(np.int32)), dev(tab[1][0].view(np.int32)),
                                 int(tab[2][0]), states, dev(np.frombuffer(b"".join(codes), np.uint8)),
                                 dev(coff), dev(clen), out, dev(sym_off))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert fl.tolist() == fl1.cpu().numpy().astype(np.uint32).tolist()
    assert np.array_equal(st, states.cpu().numpy().view(np.uint64))
    for k in range(n):
        assert np.array_equal(slots[k], h[sym_off[k]: sym_off[k + 1]]), k


@pytest.mark.parametrize("n_symbols", [2, 63, 64, 65, 129, 256])
def test_inconsistent_tables_give_the_bisection_symbol(ctx, n_symbols):
    """Rows whose cum is shuffled (not monotone): the decoder's symbol is the one the reference's
    bisection reaches, flag or not."""
    good = RR.mixed_table(n_symbols, 100 + n_symbols)
    tab = RR.shuffled_table(n_symbols, 100 + n_symbols)
    rows, syms = _streams(good, 50 + n_symbols, n_streams=24)
    codes = [ref_encode(good, r, s, True)[1] for r, s in zip(rows, syms)]
    codes[5::6] = RR.garbage_streams(n_symbols, 4)
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    assert sum(len(w[1]) for w in want) > 200
    check_decode(gpu_decode(ctx, dtab(tab), rows, codes), want)


ERR_AT = (0, 63, 64, 129)  # symbol 0, the block seam's two sides, the last of 130


def _error_table(n_symbols=65):
    c, cum, total = RR.mixed_table(n_symbols, 100 + n_symbols)
    c, cum, total = c.copy(), cum.copy(), total.copy()
    total[5] = 0             # a row of total 0
    c[6], cum[6], total[6] = 0, cum[2], total[2]  # row 2's intervals, every c_freq 0
    return c, cum, total


def test_decode_errors_at_the_block_seams(ctx):
    tab = _error_table()
    T = dtab(tab)
    rng = np.random.default_rng(3)
    usable = np.array([r for r in range(RR.N_ROWS) if r not in (5, 6)])
    rows, codes = [], []
    for kind in ("row=n_rows", "row=2^32-1", "total=0", "c=0", "none"):
        for at in ERR_AT:
            enc_rows = usable[rng.integers(0, len(usable), 130)].astype(np.uint32)
            enc_rows[at] = 2
            codes.append(ref_encode(tab, enc_rows, RR.live_symbols(tab[0], enc_rows, rng), True)[1])
            r = enc_rows.copy()
            if kind != "none":
                r[at] = {"row=n_rows": RR.N_ROWS, "row=2^32-1": 0xFFFFFFFF, "total=0": 5,
                         "c=0": 6}[kind]
            rows.append(r)
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    for j, (f, s, row) in enumerate(want[:16]):
        assert f == (cpu.F_CORRUPT if j >= 12 else cpu.F_BAD_MODEL)
        assert len(s) == ERR_AT[j % 4] == int(row[4])
    assert all(w[0] == 0 and len(w[1]) == 130 for w in want[16:])  # the others are untouched
    slots, fl, st = got = gpu_decode(ctx, T, rows, codes)
    check_decode(got, want)
    # the flag is sticky: one more symbol from the same states changes nothing
    more = [np.array([2], np.uint32)] * len(rows)
    want2 = [ref_decode(tab, r, c, st_row=row) for r, c, row in zip(more, codes, st)]
    assert [w[0] for w in want2[:16]] == [w[0] for w in want[:16]]
    check_decode(gpu_decode(ctx, T, more, codes, st_in=st), want2, "again")


def test_truncated_at_every_length(ctx):
    """One 40-symbol stream cut at every length from 0 to its own: RC_F_TRUNCATED at the oracle's
    symbol (for fewer than 8 bytes at Decoder::new, the state untouched)."""
    tab = RR.mixed_table(256, 356)
    rng = np.random.default_rng(8)
    r = rng.integers(0, RR.N_ROWS, 40).astype(np.uint32)
    code = ref_encode(tab, r, RR.live_symbols(tab[0], r, rng), True)[1]
    codes = [code[:L] for L in range(len(code) + 1)]
    rows = [r] * len(codes)
    want = [ref_decode(tab, r, c) for c in codes]
    assert want[-1][0] == 0 and want[0][0] == cpu.F_TRUNCATED
    assert len({len(w[1]) for w in want}) > 20
    T = dtab(tab)
    slots, fl, st = got = gpu_decode(ctx, T, rows, codes)
    check_decode(got, want)
    want2 = [ref_decode(tab, r[:1], c, st_row=row) for c, row in zip(codes, st)]
    check_decode(gpu_decode(ctx, T, [r[:1]] * len(codes), codes, st_in=st), want2, "again")


def test_encode_errors_at_the_block_seams(ctx):
    tab = _error_table()
    T = dtab(tab)
    rng = np.random.default_rng(4)
    usable = np.array([r for r in range(RR.N_ROWS) if r not in (5, 6)])
    rows, syms = [], []
    for kind in ("sym=n_symbols", "c=0", "row=n_rows", "row=2^32-1", "total=0", "none"):
        for at in ERR_AT:
            r = usable[rng.integers(0, len(usable), 130)].astype(np.uint32)
            r[at] = 2
            s = RR.live_symbols(tab[0], r, rng)
            if kind == "sym=n_symbols":
                s[at] = 65
            elif kind == "c=0":
                s[at] = np.flatnonzero(tab[0][2] == 0)[0]
            elif kind != "none":
                r[at] = {"row=n_rows": RR.N_ROWS, "row=2^32-1": 0xFFFFFFFF, "total=0": 5}[kind]
            rows.append(r)
            syms.append(s)
    for finish in (True, False):
        want = [ref_encode(tab, r, s, finish) for r, s in zip(rows, syms)]
        flags = [w[0] for w in want]
        assert flags == [cpu.F_BAD_SYMBOL] * 4 + [cpu.F_ZERO_FREQ] * 4 + [cpu.F_BAD_MODEL] * 12 + \
            [0] * 4
        assert [int(w[3][4]) for w in want[:20]] == list(ERR_AT) * 5
        codes, counts, fl, st = got = gpu_encode(ctx, T, rows, syms, finish)
        check_encode(got, want, finish)
        one = [np.array([2], np.uint32)] * len(rows)
        s1 = [RR.live_symbols(tab[0], o, rng) for o in one]
        want2 = [ref_encode(tab, o, s, finish, st_row=row) for o, s, row in zip(one, s1, st)]
        assert [w[0] for w in want2[:20]] == flags[:20]  # sticky
        check_encode(gpu_encode(ctx, T, one, s1, finish, st_in=st), want2, "again")


def test_encode_capacity_rule(ctx):
    """A slot one byte short of RC_STREAM_MAX_BYTES: RC_F_CAPACITY, not sticky, nothing changed."""
    tab = RR.mixed_table(64, 164)
    T = dtab(tab)
    r = np.arange(10, dtype=np.uint32)
    s = RR.live_symbols(tab[0], r, np.random.default_rng(1))
    # (gpu_encode's slots are 64 guard bytes longer than what it names their capacity)
    codes, counts, fl, st = gpu_encode(ctx, T, [r, r], [s, s], True, slack=-65)
    assert fl.tolist() == [N.F_CAPACITY] * 2 and codes == [b"", b""]
    assert np.array_equal(st, fresh(2))
    check_encode(gpu_encode(ctx, T, [r, r], [s, s], True, st_in=st), [ref_encode(tab, r, s, True)] * 2)


@pytest.mark.parametrize("n_symbols", RR.SIZES)
def test_garbage_streams(ctx, n_symbols):
    tab = RR.mixed_table(n_symbols, 100 + n_symbols)
    codes = RR.garbage_streams(n_symbols)
    rows = list(RR.garbage_rows(n_symbols))
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    if n_symbols >= 2:
        flagged = sum(w[0] != 0 for w in want)
        assert flagged >= 4 and len(want) - flagged >= 4
    check_decode(gpu_decode(ctx, dtab(tab), rows, codes), want)


def test_host_side_refusals(ctx):
    lib, h = ctx._lib, ctx.handle
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = N.ctypes.c_void_p(t.data_ptr())
    dargs = [h, p, p, p, 1, 1, p, p, p, p, p, p, p, 1, p]
    eargs = [h, p, p, p, 1, 1, p, p, p, p, 1, p, p, p, p, 0, p]
    for fn, args, ptrs, ns, nbytes in (
            (lib.rc_stream_decode_rows, dargs, (1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 14), 13, None),
            (lib.rc_stream_encode_rows, eargs, (1, 2, 3, 6, 7, 8, 9, 11, 12, 13, 16), 10, 14)):
        for i in ptrs:
            a = list(args)
            a[i] = None
            assert fn(*a) == N.RC_E_ARG, (fn.__name__, i)
            a[ns] = 0
            assert fn(*a) == N.RC_OK, (fn.__name__, i)  # no stream: nothing is read
        for bad in (0, 257):
            a = list(args)
            a[5] = bad
            assert fn(*a) == N.RC_E_BAD_MODEL
        a = list(args)
        a[4] = 0
        assert fn(*a) == N.RC_E_ARG  # no rows, but a stream
        a[ns] = 0
        assert fn(*a) == N.RC_OK
        a = list(args)
        a[0] = None
        assert fn(*a) == N.RC_E_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        rc.stream_decode_rows_batch(ctx, t[:4].view(torch.int32), t[:4].view(torch.int32),
                                    t[:1].view(torch.int32), t.view(torch.int32), t, t, t, t, t, t)
    with pytest.raises(rc.BadModelError):
        rc.RowTable(np.zeros((2, 257), np.uint32), np.zeros((2, 257), np.uint32), [1, 1], ctx=ctx)


def test_chunks_round_trip_and_raised_flags(ctx):
    rng = np.random.default_rng(21)
    counts = rng.integers(0, 500, (300, 100))
    counts[np.arange(300), rng.integers(0, 100, 300)] += 1
    counts[7, 3], counts[7, 50] = 0, 9
    table = rc.RowTable.from_counts(counts, ctx=ctx)
    assert (table.n_rows, table.n_symbols) == (300, 100)
    rows = [rng.integers(0, 300, L).astype(np.uint32) for L in (0, 1, 64, 777)]
    chunks = [RR.live_symbols(counts, r, rng) for r in rows]
    codes = rc.encode_chunks_rows(table, chunks, rows)
    c, cum, total = rc.RowTable.tables_from_counts(counts)
    for k in range(4):
        assert codes[k] == ref_encode((c, cum, total), rows[k], chunks[k], True)[1]
    back = rc.decode_chunks_rows(table, codes, rows)
    assert all(np.array_equal(b, ch) for b, ch in zip(back, chunks))
    with pytest.raises(rc.BadSymbolError):
        rc.encode_chunks_rows(table, [bytes([100])], [[0]])
    with pytest.raises(rc.BadModelError):
        rc.encode_chunks_rows(table, [bytes([1])], [[300]])
    zero = int(np.flatnonzero(counts[7] == 0)[0])
    with pytest.raises(rc.ZeroFrequencyError):
        rc.encode_chunks_rows(table, [bytes([zero])], [[7]])
    assert rc.encode_chunks_rows(table, [bytes([zero])], [[7]], raise_on_error=False) == [b""]
    with pytest.raises(rc.TruncatedStreamError):
        rc.decode_chunks_rows(table, [codes[3][:100]], [rows[3]])
    with pytest.raises(rc.BadModelError):
        rc.decode_chunks_rows(table, [codes[2]], [[1, 2, 300]])
    part = rc.decode_chunks_rows(table, [codes[3][:100]], [rows[3]], raise_on_error=False)[0]
    assert 0 < len(part) < 777 and np.array_equal(part, chunks[3][:len(part)])
    with pytest.raises(ValueError):
        rc.encode_chunks_rows(table, [bytes(3)], [[0, 1]])
