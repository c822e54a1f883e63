"""The conditions that keep test_gpu_high_offsets.py from passing by accident, checked on the
host for every layout that module uses (both import the table in high_arena.py).

A GPU case proves something only if a truncating kernel could not pass it: every chunk at or
above the boundary must get another address under each 32-bit mistake, and that address must
hold sentinels (or lie before the arena), never another chunk."""
import numpy as np
import pytest

import high_arena as H

NAMES = list(H.CASES)
B32 = 1 << 32


def spans(off, eb):
    return off[:-1] * eb, off[1:] * eb


def check_placement(off, eb, boundary, mode, lens):
    a, b = spans(off, eb)
    assert off[0] * eb < boundary
    assert np.array_equal(np.diff(off), lens)
    if mode == "straddle":
        assert ((a < boundary) & (b > boundary)).any()
    else:
        full = np.asarray(lens) > 0
        assert ((a == boundary) & full).any() and ((b == boundary) & full).any()
    above = a >= boundary
    assert (a > boundary).sum() * 3 >= len(lens), "a third of the chunks wholly above"
    return above


def check_truncations(off, eb, boundary, crosses, arena_bytes):
    """every chunk at or above the boundary: each mistake that the placement exposes moves it,
    into the sentinels of the same arena or before the arena, never onto a chunk"""
    a, _ = spans(off, eb)
    lo, hi = int(off[0]) * eb, int(off[-1]) * eb
    t = H.truncations(off[:-1], eb)
    kinds = ["byte_mod", "byte_sext"] + (["index_mod"] if "index" in crosses else [])
    for k in np.flatnonzero(a >= boundary):
        for kind in kinds:
            w = int(t[kind][k])
            assert w != int(a[k]), (kind, k)
            assert w < 0 or w + 4096 <= lo or (hi <= w and w + 4096 <= arena_bytes), (kind, k, w)
    if "index" not in crosses:  # the element index fits 32 bits there: nothing to catch
        assert (t["index_mod"] == a).all()


@pytest.mark.parametrize("name", NAMES)
def test_symbol_arenas(name):
    case = H.CASES[name]
    lens = H.case_lens(name)
    assert 36 <= len(lens) <= 44 and set(H.BASE_LENS) <= set(lens.tolist())
    for which in ("enc", "dec"):
        eb, boundary, crosses = H.PLACEMENTS[case["place" if which == "enc" else "dec_place"]]
        off = H.case_layout(name, which)
        check_placement(off, eb, boundary, case[which], lens)
        check_truncations(off, eb, boundary, crosses, H.arena_elems(off[-1], eb) * eb)
        # the chunks are at most 4096 bytes (300 symbols of 2 bytes), so a truncated chunk of
        # any length lies in the sentinels whole (the 4096 in check_truncations)
        assert int(lens.max()) * eb <= 4096
    # a family sees the boundary inside a chunk in one direction and between two in the other
    assert {case["enc"], case["dec"]} == {"straddle", "exact"} or len(case["peak"]) == 1 and \
        case["peak"][0][1] == 1


def test_both_modes_reach_every_placement():
    seen = {}
    for name, case in H.CASES.items():
        seen.setdefault(case["place"], set()).update((case["enc"], case["dec"]))
    for place in ("u8", "u16", "u16_index"):
        assert seen[place] == {"straddle", "exact"}, place


@pytest.mark.parametrize("mode", ["straddle", "exact"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_slot_layout(mode, seed):
    rng = np.random.default_rng(seed)
    caps = rng.integers(8, 700, 41)
    off, used = H.slot_layout(caps, mode=mode)
    assert off[0] % 2 == 1 and (used[1:] == caps[1:]).all() and 0 <= used[0] - caps[0] <= 1
    check_placement(off, 1, B32, mode, used)
    check_truncations(off, 1, B32, ("byte", "index"), H.arena_elems(off[-1], 1))


@pytest.mark.parametrize("seed", range(1, 28))
def test_code_layout(seed):
    rng = np.random.default_rng(100 + seed)
    lens = rng.integers(8, 700, 41)
    off = H.code_layout(lens, seed=seed)
    end = off + lens
    assert len(set(off.tolist())) == len(off) and (np.diff(off) < 0).any()  # not monotone
    low, high = off < (1 << 30), off > B32
    assert low.sum() >= 1 and ((off < B32) & (end > B32)).sum() == 1
    assert high.sum() * 3 >= len(off)
    assert {int(x) % 16 for x in off[high]} == set(range(16))
    # streams do not overlap and keep 16 sentinels between them
    order = np.argsort(off)
    assert (off[order][1:] - end[order][:-1] >= 16).all()
    # a high stream's truncated address: sentinels below the low streams
    t = H.truncations(off, 1)
    for k in np.flatnonzero(off >= B32):
        for kind in ("byte_mod", "byte_sext", "index_mod"):
            w = int(t[kind][k])
            assert w != off[k] and 0 <= w and w + int(lens[k]) + 16 <= off[low].min(), (kind, k)
    assert H.arena_elems(int(end.max()), 1) - int(end.max()) >= H.TAIL_BYTES


def test_filler_layout():
    """the containers' slots: the filler's copy runs aligned, every other slot lies past the
    boundary, and what a 32-bit offset would read instead of it, in the slots and in the
    container (payload from a 16-byte aligned offset below 64 KiB), is the filler's sentinels"""
    caps = np.array([40] + [8 + 9 * k for k in range(40)])
    off = H.filler_layout(caps)
    assert off[0] % 16 == 0 and off[1] % 2 == 1 and off[1] - off[0] >= H.FILLER_BYTES
    assert (off[1:] > B32).all() and (np.diff(off)[1:] == caps[1:]).all()
    t = H.truncations(off[1:-1], 1)
    for kind in t:
        assert ((t[kind] >= off[0] + 2048) & (t[kind] + caps[1:] < B32)).all(), kind
    padded = (np.concatenate([[H.FILLER_BYTES], caps[1:]]) + 15) // 16 * 16
    for payload_off in (64 + 1024 + 16 * 41, 65536):
        inside = payload_off + np.cumsum(padded)[:-1]
        t = H.truncations(inside, 1)
        for kind in t:
            assert ((t[kind] >= payload_off + 2048) & (t[kind] + 4096 < payload_off + B32)).all()


@pytest.mark.parametrize("place", list(H.PLACEMENTS))
def test_every_placement_is_reachable(place):
    """the table of DESIGN.md: the element index each arena is laid around, and what passes
    2^32 there"""
    eb, boundary, crosses = H.PLACEMENTS[place]
    lens = H.chunk_lens(3)
    off = H.layout(lens, eb, boundary)
    check_placement(off, eb, boundary, "straddle", lens)
    check_truncations(off, eb, boundary, crosses, H.arena_elems(off[-1], eb) * eb)
    want = {"u8": 1 << 32, "u16": 1 << 31, "u16_index": 1 << 32, "row_of": 1 << 30,
            "triples": (1 << 32) // 12}[place]
    assert abs(int(off[len(off) // 2]) - want) < 4096
    assert ("index" in crosses) == (want >= 1 << 32)


@pytest.mark.parametrize("eb", [1, 2, 4])
def test_phase_is_kept(eb):
    lens = H.chunk_lens(5)
    for phase in range(0, 64, eb):
        off = H.layout(lens, eb, phase=phase)
        assert off[0] * eb % 64 == phase
        check_placement(off, eb, B32, "straddle", lens)


def test_truncations_by_hand():
    t = H.truncations(np.array([5, (1 << 31) + 5, (1 << 32) + 5]), 2)
    assert t["byte_mod"].tolist() == [10, 10, 10 + 0]  # 2^32 + 10 and 2^33 + 10 both wrap to 10
    assert t["byte_sext"].tolist() == [10, 10, 10]
    assert t["index_mod"].tolist() == [10, (1 << 32) + 10, 10]
    t = H.truncations(np.array([(1 << 31) + 7, (1 << 32) - 1]), 1)
    assert t["byte_sext"].tolist() == [7 - (1 << 31), -1]
    assert t["byte_mod"].tolist() == [(1 << 31) + 7, (1 << 32) - 1]


def test_merged_ranges():
    assert H.merged([(5, 9), (0, 3), (3, 5), (20, 20), (30, 31)]) == [(0, 9), (30, 31)]


@pytest.mark.parametrize("name", NAMES)
def test_memory_cap(name):
    assert H.peak_bytes(name) <= H.MEM_CAP


def test_rows_launch_passes_the_boundary():
    """chunk_hist[k * 256 + tid] of 4-byte counts: row k begins at byte 1024 k, so the real
    chunks at the end of the launch have their rows past 2^32, and a row index or byte offset
    narrowed to 32 bits puts them on the rows of the first chunks, which are compared as empty"""
    first_real = H.ROWS_CHUNKS - H.ROWS_REAL
    assert first_real * 1024 >= B32
    t = H.truncations(np.arange(first_real, H.ROWS_CHUNKS), 1024)
    assert (t["byte_mod"] < H.ROWS_REAL * 1024).all() and (t["byte_sext"] >= 0).all()
    assert H.ROWS_CHUNKS * 1024 + (8 << 20) <= H.MEM_CAP


def test_untouched_counts_outside_the_kept_ranges(monkeypatch):
    """on a host tensor, in slices far smaller than the ranges"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(H, "SLICE_BYTES", 64)
    for dtype, sent in ((torch.uint8, 0xEE), (torch.int16, 0xEEEE), (torch.int32, 0xEEEEEEEE)):
        t = torch.full((1000,), H._sentinel(dtype, sent), dtype=dtype)
        t[5], t[999], t[500] = 1, 7, 9
        t[100:200] = 3
        assert H.untouched(t, [], sent) == 103
        assert H.untouched(t, [(100, 200)], sent) == 3
        assert H.untouched(t, [(150, 200), (100, 150), (499, 501)], sent) == 2
        assert H.untouched(t, [(0, 6), (100, 200), (400, 1000)], sent) == 0
        assert H.untouched(t, [(0, 1000)], sent) == 0
