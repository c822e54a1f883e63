"""The order-1 reference (order1_ref.py) against itself and against the indexed reference, on the
CPU oracle only: what the GPU tests of the order-1 coders compare with."""
import numpy as np

import indexed_ref
from order1_ref import decode_ref, derive_idx, draw_markov, encode_ref, markov_rows, tables
from oracle import cpu


def test_round_trip_on_markov_data():
    rng = np.random.default_rng(1)
    K, n, total = 8, 256, 65536
    c, cum = tables(markov_rows(rng, K, n, total))
    ctx_map = (np.arange(n) >> 5).astype(np.uint8)
    for L in (0, 1, 2, 17, 300, 2000):
        s = draw_markov(rng, c, ctx_map, 7, L)
        f, b = encode_ref(c, cum, total, ctx_map, 7, s)
        assert f == 0 and len(b) >= 8
        fd, d = decode_ref(c, cum, total, ctx_map, 7, b, L)
        assert fd == 0 and np.array_equal(d, s), L


def test_encode_equals_the_indexed_reference_on_hand_derived_indexes():
    rng = np.random.default_rng(2)
    K, n, total = 5, 100, 40000
    c, cum = tables(markov_rows(rng, K, n, total))
    ctx_map = rng.integers(0, K, n).astype(np.uint8)
    s = draw_markov(rng, c, ctx_map, 3, 500)
    idx = [3] + [int(ctx_map[int(s[i - 1])]) for i in range(1, len(s))]
    assert derive_idx(ctx_map, 3, s, n).tolist() == idx
    assert encode_ref(c, cum, total, ctx_map, 3, s) == indexed_ref.encode_ref(c, cum, total, s, idx)
    # and the indexed decoder, given those indexes as side information, reads the same stream
    f, b = encode_ref(c, cum, total, ctx_map, 3, s)
    assert indexed_ref.decode_ref(c, cum, total, b, idx)[1].tolist() == s.tolist()


def test_three_symbols_two_rows_by_hand():
    """Rows: 0 = (200, 50, 6), 1 = (6, 50, 200).  Map: 0 -> 1, 1 -> 0, 2 -> 1; first_row 1.
    Symbols 2 0 1 1 2 are coded with rows 1 1 1 0 0."""
    c, cum = tables([[200, 50, 6], [6, 50, 200]])
    ctx_map = np.array([1, 0, 1], np.uint8)
    s = np.array([2, 0, 1, 1, 2], np.uint8)
    rows = [1, 1, 1, 0, 0]
    assert derive_idx(ctx_map, 1, s, 3).tolist() == rows
    tri = np.array([[c[j, x], cum[j, x], 256] for j, x in zip(rows, s)], np.uint32)
    f, want, _ = cpu.stream_encode(cpu.Stream.fresh(), tri, finish=True)
    assert f == 0
    assert encode_ref(c, cum, 256, ctx_map, 1, s) == (0, want)
    assert decode_ref(c, cum, 256, ctx_map, 1, want, 5)[1].tolist() == s.tolist()
    # the other first row is another stream
    assert encode_ref(c, cum, 256, ctx_map, 0, s)[1] != want


def test_flags_of_the_reference():
    c, cum = tables([[255, 1, 0], [1, 0, 255]])
    ctx_map = np.array([0, 1, 1], np.uint8)
    # symbol 1 after symbol 0 is fine (row 0), after symbol 1 it has c = 0 (row 1)
    assert encode_ref(c, cum, 256, ctx_map, 0, [0, 1, 2])[0] == 0
    assert encode_ref(c, cum, 256, ctx_map, 0, [0, 1, 1])[0] == cpu.F_ZERO_FREQ
    assert encode_ref(c, cum, 256, ctx_map, 0, [0, 3, 1])[0] == cpu.F_BAD_SYMBOL
    # row 0 after a symbol outside the alphabet
    assert derive_idx(ctx_map, 1, [2, 7, 0], 3).tolist() == [1, 1, 0]
    # Decoder::new runs even for an empty chunk
    assert decode_ref(c, cum, 256, ctx_map, 0, b"\0" * 7, 0)[0] == cpu.F_TRUNCATED
    f, d = decode_ref(c, cum, 256, ctx_map, 0, b"\0" * 8, 0)
    assert f == 0 and len(d) == 0
