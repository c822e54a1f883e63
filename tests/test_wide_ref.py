"""tests/wide_ref.py (the expected results of the wide batch coders) pinned to the C oracle where
the two overlap: for alphabets of at most 256 symbols encode_ref must equal cpu.encode and
decode_ref must equal cpu.decode, flags and symbols, on clean, truncated and garbage streams."""
import numpy as np
import pytest

from oracle import cpu, ref_literal as ref

from wide_ref import decode_ref, encode_ref, literal_table, table

# 40 symbols, total 256, with zero-frequency symbols inside, in front and behind
C_SMALL = [0, 0, 30, 1, 0, 0, 0, 12, 9, 1, 1, 1, 40, 0, 25, 3, 3, 3, 0, 0,
           0, 0, 68, 2, 2, 2, 2, 1, 1, 1, 1, 20, 0, 7, 5, 5, 5, 5, 0, 0]


def _draw(rng, c, n):
    p = np.asarray(c, np.float64)
    return rng.choice(len(c), size=n, p=p / p.sum())


def test_small_table_shape():
    c, cum, total = table(C_SMALL)
    assert total == 256 and c[0] == 0 and c[-1] == 0


@pytest.mark.parametrize("n", [0, 1, 17, 3000])
def test_encode_matches_the_c_oracle(n):
    c, cum, total = table(C_SMALL)
    syms = _draw(np.random.default_rng(50 + n), C_SMALL, n)
    f, b, _ = cpu.encode(c, cum, total, syms.astype(np.uint8))
    assert (f, b) == (0, encode_ref(c, cum, total, syms)[1])
    assert encode_ref(c, cum, total, syms)[0] == 0


def test_encode_errors_match_the_c_oracle():
    c, cum, total = table(C_SMALL)
    syms = _draw(np.random.default_rng(3), C_SMALL, 64)
    z = syms.copy()
    z[10] = 4  # c == 0
    assert encode_ref(c, cum, total, z)[0] == cpu.F_ZERO_FREQ
    assert cpu.encode(c, cum, total, z.astype(np.uint8))[0] == cpu.F_ZERO_FREQ
    b = syms.copy()
    b[20] = len(C_SMALL)
    assert encode_ref(c, cum, total, b)[0] == cpu.F_BAD_SYMBOL
    assert cpu.encode(c, cum, total, b.astype(np.uint8))[0] == cpu.F_BAD_SYMBOL
    # the earliest wins, whatever its kind; 16-bit values far outside the alphabet included
    zb = z.copy()
    zb[20] = 65535
    assert encode_ref(c, cum, total, zb)[0] == cpu.F_ZERO_FREQ
    bz = b.copy()
    bz[40] = 4
    assert encode_ref(c, cum, total, bz)[0] == cpu.F_BAD_SYMBOL


def _same_as_c_oracle(c, cum, total, code, n, lit):
    f, out = decode_ref(c, cum, total, code, n, lit)
    fc, outc = cpu.decode(c, cum, total, code, n)
    assert f == fc, (f, fc, len(code), n)
    assert list(out) == list(outc[:len(out)])
    if f == 0:
        assert len(out) == n
    return f


def test_decode_matches_the_c_oracle_on_clean_truncated_and_garbage_streams():
    c, cum, total = table(C_SMALL)
    lit = literal_table(c)
    rng = np.random.default_rng(11)
    seen = set()
    # clean streams and every truncation of one of them
    for n in (0, 1, 5, 400):
        syms = _draw(rng, C_SMALL, n)
        f, code = encode_ref(c, cum, total, syms)
        assert f == 0
        f, out = decode_ref(c, cum, total, code, n, lit)
        assert f == 0 and list(out) == list(syms)
        assert _same_as_c_oracle(c, cum, total, code, n, lit) == 0
    syms = _draw(rng, C_SMALL, 40)
    _, code = encode_ref(c, cum, total, syms)
    for cut in range(len(code)):
        f = _same_as_c_oracle(c, cum, total, code[:cut], 40, lit)
        assert f in (0, cpu.F_TRUNCATED) and (cut >= 8 or f == cpu.F_TRUNCATED)
    # garbage: the mapping of the literal decoder's panics must not be checked vacuously
    for k in range(96):
        code = rng.integers(0, 256, int(rng.integers(8, 120)), dtype=np.uint8).tobytes()
        seen.add(_same_as_c_oracle(c, cum, total, code, int(rng.integers(1, 200)), lit))
    assert {0, cpu.F_TRUNCATED, cpu.F_CORRUPT} <= seen, seen


def test_wide_alphabet_round_trips_through_the_literal_reference():
    rng = np.random.default_rng(21)
    cw = rng.integers(0, 60, 1000)
    cw[rng.integers(0, 1000, 300)] = 0
    cw[5] += 65536 - int(cw.sum())
    c, cum, total = table(cw)
    assert total == 65536
    syms = _draw(rng, cw, 2000)
    f, code = encode_ref(c, cum, total, syms)
    assert f == 0
    lit = literal_table(c)
    assert code == ref.encode_stream(lit, [int(s) for s in syms])
    assert ref.decode_stream(lit, code, len(syms)) == [int(s) for s in syms]
    f, out = decode_ref(c, cum, total, code, len(syms), lit)
    assert f == 0 and out.dtype == np.uint16 and list(out) == list(syms)
