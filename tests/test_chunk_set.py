"""Static chunk sets without a device: what rc_model_create_chunk_set accepts,
the plan its launchers follow at every class seam of the total, the grouping rule against a few
lines of NumPy, and rc_cost_table against NumPy."""
import ctypes

import numpy as np
import pytest

from range_coder_rust_amd import _native as N
from range_coder_rust_amd import model_build as MB
import static_cases as S
import chunk_fit_ref as R

TOTALS = (256, 512, 513, 2048, 2049, 65535, 65536)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def rows_of(total, k=3, complete=True):
    """k rows of 256 symbols and the given total: Zipf weights, rotated (row 1 loses symbol 7 when
    the set is to be incomplete)"""
    base = S.alloc(S.zipf_w(256), total)
    rows = [np.roll(base, 85 * j) for j in range(k)]
    if not complete:
        r = rows[min(1, k - 1)].copy()
        r[8] += r[7]
        r[7] = 0
        rows[min(1, k - 1)] = r
    c = np.ascontiguousarray(np.stack(rows), np.uint32)
    assert (c.sum(axis=1) == total).all()
    return c, np.stack([S.cum_of(r) for r in c]).astype(np.uint32)


def check(k, n, c, cum, total):
    return N.load().rc_chunk_set_check_(k, n, _p(c), _p(cum), ctypes.c_uint32(total))


def test_creation_checks():
    c, cum = rows_of(4096, 64)
    assert check(1, 256, c, cum, 4096) == N.RC_OK
    assert check(64, 256, c, cum, 4096) == N.RC_OK
    assert check(0, 256, c, cum, 4096) == N.RC_E_BAD_MODEL
    assert check(65, 256, np.tile(c, (2, 1)), np.tile(cum, (2, 1)), 4096) == N.RC_E_BAD_MODEL
    for total, want in ((255, N.RC_E_BAD_MODEL), (256, N.RC_OK), (65536, N.RC_OK),
                        (65537, N.RC_E_BAD_MODEL)):
        if want == N.RC_OK:
            ct, cumt = rows_of(total, 2)
        else:  # (rows that do sum to the refused total)
            ct = np.zeros((2, 256), np.uint32)
            ct[:, 0] = total
            cumt = np.stack([S.cum_of(r) for r in ct]).astype(np.uint32)
        assert check(2, 256, ct, cumt, total) == want, total
    bad = c.copy()
    bad[3, 0] += 1  # a row that does not sum to the total
    assert check(64, 256, bad, cum, 4096) == N.RC_E_BAD_MODEL
    badcum = cum.copy()
    badcum[5, 0] = 1  # cum[0] != 0
    assert check(64, 256, c, badcum, 4096) == N.RC_E_BAD_MODEL
    assert check(64, 0, c, cum, 4096) == N.RC_E_BAD_MODEL
    assert N.load().rc_chunk_set_check_(1, 256, None, None, 4096) == N.RC_E_ARG


def static_plan(c, total):
    out = np.zeros(9, np.uint32)
    assert N.load().rc_model_static_plan_(len(c), _p(c), _p(S.cum_of(c)), total, _p(out)) == N.RC_OK
    return out


@pytest.mark.parametrize("total", TOTALS)
def test_plan_follows_the_total(total):
    for complete in (True, False):
        c, cum = rows_of(total, 3, complete)
        out = np.zeros(10, np.uint32)
        assert N.load().rc_chunk_set_plan_(3, 256, _p(c), _p(cum), total, _p(out)) == N.RC_OK
        smv, lut, lanes, has_symof, div, tab_b, lut_b, symof_b, has_pair, flat = (int(x) for x in out)
        sp = static_plan(np.ascontiguousarray(c[0]), total)
        # the LUT of a row of that total: 16-B direct entries, 4-B direct entries, buckets
        want_lut = {2: 2, 1: 1, 0: 4}[int(sp[1])]
        assert lut == want_lut and div == int(sp[7]) and has_symof == int(sp[4])
        assert smv == (2 if complete else 1)
        assert has_pair == 0 and flat == 0
        assert tab_b == 2048
        n_lut = 1 << (total - 1).bit_length()
        if total <= 512:
            assert lut_b == 16 * n_lut and symof_b == 0 and lanes == 256
        elif total <= 2048:
            assert lut_b == 4 * n_lut and symof_b == 0 and lanes == 256
        else:
            buckets = 1 << min(12, (total - 1).bit_length() - 3)
            assert lut_b == 8 * buckets and symof_b == n_lut
            assert lanes == (512 if buckets > 2048 else 256)


def test_all_ones_row_is_not_flat():
    """total 256, every c = 1: the static model is flat (encoder variant 3, LUT 5); as a row of a
    chunk set it runs the general LUT 2 step and the complete encoder"""
    ones = np.ones(256, np.uint32)
    assert static_plan(ones, 256)[2] == 1
    c = np.ascontiguousarray(np.stack([ones, ones]))
    cum = np.stack([S.cum_of(r) for r in c]).astype(np.uint32)
    out = np.zeros(10, np.uint32)
    assert N.load().rc_chunk_set_plan_(2, 256, _p(c), _p(cum), 256, _p(out)) == N.RC_OK
    assert (int(out[0]), int(out[1]), int(out[9])) == (2, 2, 0)


def group_ref(cls, K, W):
    """the grouping rule in NumPy: stable by chunk id inside a class, classes padded to whole
    workgroups of the grid ceil(n / W) + K, ~0 for dead lanes and unused workgroups"""
    grid = (len(cls) + W - 1) // W + K
    order = np.full(grid * W, 0xFFFFFFFF, np.uint32)
    wg_row = np.full(grid, 0xFFFFFFFF, np.uint32)
    at = 0
    for c in range(K):
        ids = np.flatnonzero(cls == c)
        order[at:at + len(ids)] = ids
        wgs = (len(ids) + W - 1) // W
        wg_row[at // W:at // W + wgs] = c
        at += wgs * W
    return order, wg_row


def group_plan(cls, K, W):
    cls = np.ascontiguousarray(cls, np.uint8)
    grid = (len(cls) + W - 1) // W + K
    order = np.zeros(grid * W, np.uint32)
    wg_row = np.zeros(grid, np.uint32)
    rc = N.load().rc_chunk_group_plan_(_p(cls) if len(cls) else None, len(cls), K, W, _p(order),
                                       _p(wg_row))
    assert rc == N.RC_OK
    return order, wg_row


def group_cases(W):
    rng = np.random.default_rng(W)
    yield "empty", np.zeros(0, np.uint8), 3
    yield "one class", np.zeros(W + 5, np.uint8), 1
    yield "one of four", np.full(2 * W + 1, 2, np.uint8), 4
    gap = np.concatenate([np.zeros(7), np.full(9, 2)]).astype(np.uint8)  # class 1 stays empty
    yield "empty class between", rng.permutation(gap), 3
    sizes = np.repeat(np.arange(4), [1, W - 1, W, W + 1]).astype(np.uint8)
    yield "1, W-1, W, W+1", rng.permutation(sizes), 4
    bad = rng.integers(0, 8, 3 * W + 17).astype(np.uint8)
    bad[::11] = 255
    yield "ids >= K", bad, 5  # (5, 6, 7 and 255 are no class)
    yield "64 classes", rng.integers(0, 64, 5000).astype(np.uint8), 64


@pytest.mark.parametrize("W", (256, 512, 1024))
def test_grouping_rule(W):
    for name, cls, K in group_cases(W):
        order, wg_row = group_plan(cls, K, W)
        want_o, want_w = group_ref(cls, K, W)
        assert np.array_equal(order, want_o), (name, W)
        assert np.array_equal(wg_row, want_w), (name, W)
        live = order[order != 0xFFFFFFFF]
        assert np.array_equal(np.sort(live), np.flatnonzero(cls < K)), name


def test_cost_table_matches_numpy():
    rng = np.random.default_rng(3)
    for total in TOTALS:
        c = S.alloc(S.zipf_w(200), total)
        c = np.concatenate([c, np.zeros(3, np.uint32)]).astype(np.uint32)
        got = MB.cost_table(c, total).astype(np.int64)
        want = R.cost_table(c, total).astype(np.int64)
        assert (got[c == 0] == 0xFFFFFFFF).all() and (want[c == 0] == 0xFFFFFFFF).all()
        assert np.abs(got - want)[c > 0].max() <= 1, total
        assert (got == want).mean() > 0.99
        # exact where the answer is: c = total costs nothing, a power-of-two ratio whole bits
        assert MB.cost_table(np.array([total], np.uint32), total)[0] == 0
    assert list(MB.cost_table(np.array([1, 2, 65536, 0], np.uint32), 65536)) == \
        [16 << 16, 15 << 16, 0, 0xFFFFFFFF]
    assert rng is not None
