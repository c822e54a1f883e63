"""k_stream_decode_rows_lane (rc_rows.hip): rc_stream_decode_rows with a lane per
stream, forced through rc_rows_decoder_, against the reference of tests/rows_ref.py: byte-exact,
and state-exact on all seven state fields, with test_gpu_rows.py's guards behind every slot.  With
guards=True a flagged guard stream sits behind every real one, so flagged and live streams are
neighbour lanes of one wave.  The forced wave-per-stream kernel is the second yardstick (identity,
interchangeable states), and the default call is checked on both sides of the rule."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from oracle import cpu  # noqa: E402
import rows_ref as RR  # noqa: E402
from test_gpu_rows import (as_row, check_decode, dtab, fresh, gpu_decode, gpu_encode,  # noqa: E402
                           ref_decode, ref_encode)

TABLES = {"mixed": RR.mixed_table, "rare": RR.rare_table, "shuffled": RR.shuffled_table}
COUNTS = (1, 3, 63, 64, 65, 129)  # real streams of a launch: the 64-lane workgroup seams
LENS = (0, 1, 5, 17, 40, 64, 65)  # symbols per stream of the table tests


@pytest.fixture(scope="module")
def ctxs():
    """contexts of their own, so that no other module sees a forced decoder: auto (the rule),
    wave, lane"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}
    try:
        for which, name in enumerate(("auto", "wave", "lane")):
            made[name] = rc.Context(0)
            assert made[name]._lib.rc_rows_decoder_(made[name].handle, which) == N.RC_OK
        yield made
    finally:
        torch.cuda.synchronize()
        for c in made.values():
            c.close()


@pytest.fixture(scope="module")
def lane(ctxs):
    return ctxs["lane"]


def test_the_choice_hook_on_a_context(ctxs):
    c = ctxs["lane"]
    assert c._lib.rc_rows_decoder_(c.handle, 3) == N.RC_E_ARG
    assert c._lib.rc_rows_decoder_(c.handle, 2) == N.RC_OK


def _table_case(n_symbols, shape):
    """129 streams of 0..65 symbols: (table, rows, codes, expected decode)"""
    tab = TABLES[shape](n_symbols, 100 + n_symbols)
    good = RR.mixed_table(n_symbols, 100 + n_symbols) if shape == "shuffled" else tab
    rng = np.random.default_rng(900 + n_symbols)
    rows = [rng.integers(0, RR.N_ROWS, LENS[k % len(LENS)]).astype(np.uint32) for k in range(129)]
    syms = [RR.live_symbols(good[0], r, rng, rare_bias=shape == "rare") for r in rows]
    codes = [ref_encode(good, r, s, True)[1] for r, s in zip(rows, syms)]
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    if shape != "shuffled":
        assert all(w[0] == 0 and w[1].tolist() == s.tolist() for w, s in zip(want, syms))
    return tab, rows, codes, want


@pytest.mark.parametrize("shape", sorted(TABLES))
@pytest.mark.parametrize("n_symbols", RR.SIZES)
def test_every_alphabet_at_the_workgroup_seams(lane, n_symbols, shape):
    """Launches of 1, 3, 63, 64, 65 and 129 streams (a last workgroup of one live lane), and the
    small ones again with a flagged stream in every second lane."""
    tab, rows, codes, want = _table_case(n_symbols, shape)
    T = dtab(tab)
    for ns in COUNTS:
        check_decode(gpu_decode(lane, T, rows[:ns], codes[:ns], guards=False), want[:ns], ns)
    for ns in (1, 3, 65):
        check_decode(gpu_decode(lane, T, rows[:ns], codes[:ns], guards=True), want[:ns], (ns, "g"))


def test_lengths_mixed_in_one_wave(lane):
    """Streams of 0..200 symbols in the lanes of one wave, an empty one, a flagged one and flagged
    guards between them: the lanes that end early keep their slots, states and guards."""
    tab = RR.mixed_table(256, 356)
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 201, 32)
    lens[:4] = (0, 200, 1, 0)
    rows = [rng.integers(0, RR.N_ROWS, int(L)).astype(np.uint32) for L in lens]
    codes = [ref_encode(tab, r, RR.live_symbols(tab[0], r, rng), True)[1] for r in rows]
    st_in = fresh(32)
    st_in[5] = np.array([1, 2, 3, 9, 4, cpu.F_CORRUPT | 1 << 32], np.uint64)  # flagged earlier
    st_in[6] = as_row(cpu.Stream.fresh())
    want = [ref_decode(tab, r, c, st_row=s) for r, c, s in zip(rows, codes, st_in)]
    assert want[5][0] == cpu.F_CORRUPT and len(want[5][1]) == 0
    assert sum(len(w[1]) for w in want) == int(lens.sum()) - int(lens[5])
    T = dtab(tab)
    for guards in (True, False):
        check_decode(gpu_decode(lane, T, rows, codes, st_in=st_in, guards=guards), want, guards)


def test_code_window_edges(lane):
    """Every alignment mod 16 of a stream's first byte, with code lengths that put the stream's
    last byte at the end of an aligned 8-byte window and at the start of a new one."""
    tab = RR.mixed_table(65, 165)
    rng = np.random.default_rng(17)
    rows, codes = [], []
    for k in range(32):  # gpu_decode puts stream k at alignment k mod 16
        while True:
            r = rng.integers(0, RR.N_ROWS, int(rng.integers(8, 40))).astype(np.uint32)
            code = ref_encode(tab, r, RR.live_symbols(tab[0], r, rng), True)[1]
            if (k % 16 + len(code)) % 8 == k // 16:  # end: 0 a window's last byte, 1 a first byte
                break
        rows.append(r)
        codes.append(code)
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    assert all(w[0] == 0 and int(w[2][3]) == len(c) for w, c in zip(want, codes))  # read to the end
    check_decode(gpu_decode(lane, dtab(tab), rows, codes, guards=False), want)
    # one byte short: the last window is never asked for where it holds no byte of the stream
    short = [c[:-1] for c in codes]
    want = [ref_decode(tab, r, c) for r, c in zip(rows, short)]
    assert all(w[0] == cpu.F_TRUNCATED for w in want)
    check_decode(gpu_decode(lane, dtab(tab), rows, short, guards=False), want, "short")


def test_resumption_and_interchangeable_states(ctxs):
    """40 streams cut into up to five calls: every call by the lane kernel, and the same cuts with
    the calls alternating between the wave and the lane kernel on the same states."""
    tab = RR.mixed_table(129, 229)
    T = dtab(tab)
    rng = np.random.default_rng(5)
    rows = [rng.integers(0, RR.N_ROWS, int(L)).astype(np.uint32)
            for L in rng.integers(0, 161, 40)]
    syms = [RR.live_symbols(tab[0], r, rng) for r in rows]
    codes = [ref_encode(tab, r, s, True)[1] for r, s in zip(rows, syms)]
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    cuts = []
    for r in rows:
        inner = sorted(rng.integers(0, len(r) + 1, int(rng.integers(0, 5))).tolist())
        cuts.append([0] + inner + [len(r)] * (5 - len(inner)))
    trace = {}
    for order in ("lane", "mixed"):
        st, got = fresh(40), [[] for _ in rows]
        for part in range(5):
            name = "lane" if order == "lane" else ("wave", "lane")[part % 2]
            pr = [r[c[part]:c[part + 1]] for r, c in zip(rows, cuts)]
            slots, fl, st = gpu_decode(ctxs[name], T, pr, codes, st_in=st, guards=False)
            assert not fl.any()
            trace.setdefault(part, []).append(st.copy())
            for k in range(40):
                got[k] += slots[k].tolist()
        for k in range(40):
            assert got[k] == syms[k].tolist() and st[k].tolist() == want[k][2].tolist(), (order, k)
    for part in range(5):
        assert np.array_equal(*trace[part]), part


ERR_AT = (0, 1, 63, 64, 129)  # of 130 symbols


def _error_table(n_symbols=65):
    c, cum, total = (a.copy() for a in RR.mixed_table(n_symbols, 100 + n_symbols))
    total[5] = 0                                   # a row of total 0
    c[6], cum[6], total[6] = 0, cum[2], total[2]   # row 2's intervals, every c_freq 0
    return c, cum, total


def test_errors_beside_healthy_lanes(lane):
    """A bad row index, a row of total 0 and a c_freq of 0 at symbols 0, 1, 63, 64 and the last,
    beside untouched streams; the flags are sticky."""
    tab = _error_table()
    T = dtab(tab)
    rng = np.random.default_rng(3)
    usable = np.array([r for r in range(RR.N_ROWS) if r not in (5, 6)])
    kinds = {"row=n_rows": RR.N_ROWS, "row=2^32-1": 0xFFFFFFFF, "total=0": 5, "c=0": 6,
             "none": None}
    rows, codes = [], []
    for kind, bad in kinds.items():
        for at in ERR_AT:
            enc_rows = usable[rng.integers(0, len(usable), 130)].astype(np.uint32)
            enc_rows[at] = 2
            codes.append(ref_encode(tab, enc_rows, RR.live_symbols(tab[0], enc_rows, rng), True)[1])
            r = enc_rows.copy()
            if bad is not None:
                r[at] = bad
            rows.append(r)
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    for j, (f, s, row) in enumerate(want[:20]):
        assert f == (cpu.F_CORRUPT if j >= 15 else cpu.F_BAD_MODEL)
        assert len(s) == ERR_AT[j % 5] == int(row[4])
    assert all(w[0] == 0 and len(w[1]) == 130 for w in want[20:])
    slots, fl, st = got = gpu_decode(lane, T, rows, codes)
    check_decode(got, want)
    more = [np.array([2], np.uint32)] * len(rows)
    want2 = [ref_decode(tab, r, c, st_row=row) for r, c, row in zip(more, codes, st)]
    assert [w[0] for w in want2[:20]] == [w[0] for w in want[:20]]
    check_decode(gpu_decode(lane, T, more, codes, st_in=st), want2, "again")


@pytest.mark.parametrize("n_symbols", [2, 256])
def test_totals_of_one_and_of_2_32_minus_1(lane, n_symbols):
    """Rows 0 (total 2^32 - 1) and 1 (total 1) of the mixed table, alone and beside other rows."""
    tab = RR.mixed_table(n_symbols, 100 + n_symbols)
    assert int(tab[2][0]) == 0xFFFFFFFF and int(tab[2][1]) == 1
    rng = np.random.default_rng(12)
    rows = [rng.choice(pool, 100).astype(np.uint32)
            for pool in ([0], [1], [0, 1], [0, 1, 2, 3]) for _ in range(3)]
    codes = [ref_encode(tab, r, RR.live_symbols(tab[0], r, rng), True)[1] for r in rows]
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    assert all(w[0] == 0 and len(w[1]) == 100 for w in want)
    check_decode(gpu_decode(lane, dtab(tab), rows, codes), want)


def test_truncated_at_every_length(lane):
    """One 40-symbol stream cut at every length from 0 to its own, each cut a lane."""
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
    for guards in (True, False):
        slots, fl, st = got = gpu_decode(lane, T, rows, codes, guards=guards)
        check_decode(got, want, guards)
    want2 = [ref_decode(tab, r[:1], c, st_row=row) for c, row in zip(codes, st)]
    check_decode(gpu_decode(lane, T, [r[:1]] * len(codes), codes, st_in=st), want2, "again")


@pytest.mark.parametrize("n_symbols", [1, 2, 64, 129, 256])
def test_garbage_streams(lane, n_symbols):
    tab = RR.mixed_table(n_symbols, 100 + n_symbols)
    codes = RR.garbage_streams(n_symbols)
    rows = list(RR.garbage_rows(n_symbols))
    want = [ref_decode(tab, r, c) for r, c in zip(rows, codes)]
    if n_symbols >= 2:
        flagged = sum(w[0] != 0 for w in want)
        assert flagged >= 4 and len(want) - flagged >= 4
    check_decode(gpu_decode(lane, dtab(tab), rows, codes), want)


def _encoded_on_the_gpu(ctx, tab, T, lens, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, RR.N_ROWS, int(L)).astype(np.uint32) for L in lens]
    syms = [RR.live_symbols(tab[0], r, rng) for r in rows]
    codes, _, fl, _ = gpu_encode(ctx, T, rows, syms, True, guards=False)
    assert not fl.any()
    return rows, syms, codes


def _same(a, b):
    (sa, fa, ta), (sb, fb, tb) = a, b
    assert np.array_equal(fa, fb) and np.array_equal(ta, tb)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))


def test_identical_to_the_wave_kernel(ctxs):
    """One launch of 300 streams of 0..300 symbols, some cut short or replaced by garbage: symbols
    (the untouched slot bytes included), flags and states of the two kernels are the same."""
    tab = RR.mixed_table(200, 300)
    T = dtab(tab)
    lens = np.random.default_rng(77).integers(0, 301, 300)
    rows, syms, codes = _encoded_on_the_gpu(ctxs["auto"], tab, T, lens, 78)
    garbage = RR.garbage_streams(200, 30)
    for j in range(30):
        codes[10 * j + 3] = garbage[j]
        codes[10 * j + 7] = codes[10 * j + 7][:len(codes[10 * j + 7]) // 2]
    got = {name: gpu_decode(ctxs[name], T, rows, codes, guards=False) for name in ("wave", "lane")}
    _same(got["wave"], got["lane"])
    slots, fl, st = got["lane"]
    assert (fl != 0).sum() >= 30
    for k in range(300):
        if k % 10 not in (3, 7):  # the streams left as they were encoded
            assert fl[k] == 0 and slots[k].tolist() == syms[k].tolist(), k


def test_the_default_call_on_both_sides_of_the_rule(ctxs):
    """The smallest launch that the rule gives to the lane kernel on this device, 8 symbols a
    stream: the forced wave kernel's output, and the reference's on 64 sampled streams.  A launch
    of 67 streams (the wave kernel, as in every other rows test) equals the reference too."""
    auto = ctxs["auto"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = auto._lib.rc_rows_decode_plan_
    assert plan(1 << 24, 256, cus) == 1
    lo, hi = 64, 1 << 24  # plan(lo) == 0 < plan(hi) == 1, and the rule is monotone
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan(mid, 256, cus) else (mid, hi)
    ns = hi
    assert plan(ns, 256, cus) == 1 and plan(ns - 1, 256, cus) == 0 and ns <= 1 << 17
    tab = RR.mixed_table(256, 356)
    T = dtab(tab)
    rows, syms, codes = _encoded_on_the_gpu(auto, tab, T, [8] * ns, 91)
    got = gpu_decode(auto, T, rows, codes, guards=False)
    _same(got, gpu_decode(ctxs["wave"], T, rows, codes, guards=False))
    _same(got, gpu_decode(ctxs["lane"], T, rows, codes, guards=False))
    pick = np.random.default_rng(92).choice(ns, 64, replace=False)
    for k in pick:
        f, s, row = ref_decode(tab, rows[k], codes[k])
        assert f == 0 == got[1][k] and got[0][k].tolist() == s.tolist() == syms[k].tolist(), k
        assert got[2][k].tolist() == row.tolist(), k
    want = [ref_decode(tab, r, c) for r, c in zip(rows[:67], codes[:67])]
    check_decode(gpu_decode(auto, T, rows[:67], codes[:67], guards=False), want, 67)
    check_decode(gpu_decode(auto, T, rows[:67], codes[:67], guards=True), want, "67g")
