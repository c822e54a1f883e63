"""CPU checks for the per-symbol row tables (rc_stream_decode_rows / rc_stream_encode_rows): the
tests' reference (tests/rows_ref.py) against the literal restatement of the reference crate with a
different FreqTable at every call, the new entry points in the header, the library and the
binding, RowTable.from_counts against numpy, and the garbage generator's spread."""
import re
import os
import subprocess

import numpy as np
import pytest

import range_coder_rust_amd as rc
from range_coder_rust_amd import _native as N
from oracle import cpu, ref_literal as R
import rows_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rc_stream_decode_rows", "rc_stream_encode_rows")


def test_reference_against_the_literal_coder_with_a_table_per_call():
    n = 2000
    c, cum, total = RR.mixed_table(64, 11)
    rng = np.random.default_rng(12)
    rows = rng.integers(0, RR.N_ROWS, n).astype(np.uint32)
    syms = RR.live_symbols(c, rows, rng)
    tabs = [R.FreqTable.from_counts([int(x) for x in c[r]]) for r in range(RR.N_ROWS)]
    for r in range(RR.N_ROWS):  # the rows are the tables calc_cum gives
        assert [tabs[r].cum_freq(i) for i in range(64)] == cum[r].tolist()
        assert tabs[r].total_freq() == int(total[r])
    enc = R.Encoder()
    counts = [enc.encode(tabs[r], int(s)) for r, s in zip(rows, syms)]
    code = bytes(enc.finish())
    st = cpu.Stream.fresh()
    f, b, nb = RR.encode_rows(st, c, cum, total, rows, syms, finish=True)
    assert f == 0 and b == code and nb.tolist() == counts
    assert (st.n, st.pos, st.stage) == (n, len(code), 2)
    dec = R.Decoder(code)
    want = [dec.decode(tabs[r]) for r in rows]
    assert want == syms.tolist()
    st = cpu.Stream.fresh()
    f, got = RR.decode_rows(st, c, cum, total, rows, code)
    assert f == 0 and got.tolist() == want
    assert (st.lower_bound, st.range, st.data) == (dec.range_coder.lower_bound,
                                                   dec.range_coder.range, dec.data)
    # in pieces: the same state and symbols
    st2 = cpu.Stream.fresh()
    parts = [RR.decode_rows(st2, c, cum, total, rows[a:b], code)[1]
             for a, b in ((0, 0), (0, 63), (63, 64), (64, 1500), (1500, n))]
    assert np.concatenate(parts).tolist() == want and st2.tuple() == st.tuple()


def test_reference_new_checks_come_first():
    c, cum, total = RR.mixed_table(5, 3)
    code = b"\x00" * 64
    st = cpu.Stream.fresh()
    f, got = RR.decode_rows(st, c, cum, total, [2, RR.N_ROWS, 0], code)
    assert f == cpu.F_BAD_MODEL and len(got) == 1 and st.n == 1 and st.stage == 1
    assert RR.decode_rows(st, c, cum, total, [0], code)[0] == cpu.F_BAD_MODEL  # sticky
    live = int(np.flatnonzero(c[2])[0])
    st = cpu.Stream.fresh()
    f, b, nb = RR.encode_rows(st, c, cum, total, [2, 2, 2], [live, 5, live], finish=True)
    assert f == cpu.F_BAD_SYMBOL and st.n == 1 and st.stage == 1 and len(nb) == 1
    st = cpu.Stream.fresh()
    f, b, nb = RR.encode_rows(st, c, cum, total, [2, 0xFFFFFFFF], [live, 9], finish=True)
    assert f == cpu.F_BAD_MODEL and st.n == 1  # the row check comes before the symbol check


def test_entry_points_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "range_coder.h")) as f:
        h = f.read()
    lib = N.load()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"^rc_status %s\(rc_ctx\* ctx," % name, h, re.M), name
        assert name in N.EXPORTS
        assert re.search(r"\bT %s\b" % name, out), name
        assert len(getattr(lib, name).argtypes) == h[h.index("rc_status " + name):].split(
            ";")[0].count(",") + 1
    for name in ("RowTable", "stream_decode_rows_batch", "stream_encode_rows_batch",
                 "encode_chunks_rows", "decode_chunks_rows"):
        assert hasattr(rc, name) and name in rc.api.__all__, name
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "rc_rows.hip" in f.read()


def test_host_side_refusals_need_no_device():
    lib = N.load()
    assert lib.rc_stream_decode_rows(None, None, None, None, 1, 1, None, None, None, None, None,
                                     None, None, 0, None) == N.RC_E_ARG
    assert lib.rc_stream_encode_rows(None, None, None, None, 1, 1, None, None, None, None, 0,
                                     None, None, None, None, 0, None) == N.RC_E_ARG


def test_row_table_from_counts_against_numpy():
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 1 << 20, (9, 77))
    counts[3] = 0
    c, cum, total = rc.RowTable.tables_from_counts(counts)
    assert c.dtype == cum.dtype == total.dtype == np.uint32
    assert np.array_equal(c, counts)
    assert np.array_equal(total, counts.sum(axis=1))
    for r in range(9):  # calc_cum: cum[0] = 0, cum[i] = cum[i - 1] + c[i - 1]
        t = rc.FreqTable.from_counts([int(x) for x in counts[r]])
        assert cum[r].tolist() == [t.cum_freq(i) for i in range(77)]
    big = np.zeros((2, 3), np.int64)
    big[1] = ((1 << 32) - 1, 0, 0)
    assert rc.RowTable.tables_from_counts(big)[2].tolist() == [0, (1 << 32) - 1]
    big[1, 2] = 1
    with pytest.raises(rc.BadModelError):
        rc.RowTable.tables_from_counts(big)
    with pytest.raises(rc.BadModelError):
        rc.RowTable.tables_from_counts([[-1, 2]])
    with pytest.raises(ValueError):
        rc.RowTable.tables_from_counts([1, 2, 3])


@pytest.mark.parametrize("n_symbols", [s for s in RR.SIZES if s >= 2])
def test_garbage_generator_leaves_both_sides_populated(n_symbols):
    """Of each table's 32 garbage streams the reference flags at least 4 and decodes at least 4
    without a flag, so the GPU test of them checks both outcomes."""
    c, cum, total = RR.mixed_table(n_symbols, 100 + n_symbols)
    rows = RR.garbage_rows(n_symbols)
    flagged = 0
    for code, r in zip(RR.garbage_streams(n_symbols), rows):
        st = cpu.Stream.fresh()
        f, _ = RR.decode_rows(st, c, cum, total, r, code)
        flagged += f != 0
    print(n_symbols, "flagged", flagged, "clean", 32 - flagged)
    assert flagged >= 4 and 32 - flagged >= 4


def test_tables_have_the_shapes_the_gpu_tests_rely_on():
    for ns in RR.SIZES:
        c, cum, total = RR.mixed_table(ns, 100 + ns)
        assert c.shape == (RR.N_ROWS, ns) and (total > 0).all() and int(total[1]) == 1
        assert ns < 2 or int(total[0]) == (1 << 32) - 1
        t = total[2:].astype(np.uint64)
        assert ((t & (t - 1)) != 0).all()
        if ns >= 8:
            live = (c[2:] > 0).mean()
            assert 0.55 < live < 0.85
        c, cum, total = RR.rare_table(ns, 200 + ns)
        assert ((c == 1 << 31).sum(axis=1) == 1).all() and (total >= 1 << 31).all()
        c2, cum2, _ = RR.shuffled_table(ns, 300 + ns)
        if ns >= 63:
            assert (np.diff(cum2.astype(np.int64), axis=1) < 0).any()
