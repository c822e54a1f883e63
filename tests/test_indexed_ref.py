"""tests/indexed_ref.py (the expected results of the indexed batch coders, built on the C
oracle's stream calls) against the literal port of the reference (oracle/ref_literal.py), whose
Encoder and Decoder take the model on every call: a different FreqTable per symbol."""
import numpy as np
import pytest

from oracle import cpu, ref_literal as ref

from indexed_ref import decode_ref, encode_ref, tables

N_SYM = 12
C_ROWS = [
    [40, 30, 20, 10, 9, 8, 7, 6, 50, 40, 20, 16],    # plain
    [1, 1, 1, 200, 1, 1, 1, 1, 1, 1, 1, 46],          # a spike
    [60, 0, 0, 0, 70, 30, 20, 10, 30, 20, 10, 6],     # a zero-frequency bin (symbols 1..3)
]


def _draw(rng, n):
    c, cum = tables(C_ROWS)
    idx = rng.integers(0, len(C_ROWS), n)
    syms = np.array([rng.choice(N_SYM, p=c[j] / c[j].sum()) for j in idx], np.int64)
    return c, cum, int(c[0].sum()), syms, idx


def test_rows_share_the_total():
    c, _ = tables(C_ROWS)
    assert set(c.sum(axis=1)) == {256}


@pytest.mark.parametrize("n", [0, 1, 17, 2000])
def test_encode_and_decode_match_the_literal_reference(n):
    rng = np.random.default_rng(1000 + n)
    c, cum, total, syms, idx = _draw(rng, n)
    lit = [ref.FreqTable.from_counts([int(x) for x in row]) for row in C_ROWS]
    enc = ref.Encoder()
    for s, j in zip(syms, idx):
        enc.encode(lit[j], int(s))
    want = bytes(enc.finish())
    f, got = encode_ref(c, cum, total, syms, idx)
    assert f == 0 and got == want
    dec = ref.Decoder(want)
    back = [dec.decode(lit[j]) for j in idx]
    assert back == list(syms)
    f, out = decode_ref(c, cum, total, want, idx)
    assert f == 0 and list(out) == back


def test_first_error_wins():
    rng = np.random.default_rng(7)
    c, cum, total, syms, idx = _draw(rng, 64)
    K = len(C_ROWS)
    # a zero-frequency symbol of its row, a symbol outside the alphabet, a row outside the set
    z, b, m = syms.copy(), syms.copy(), idx.copy()
    z[10], idx_z = 2, idx.copy()
    idx_z[10] = 2
    assert encode_ref(c, cum, total, z, idx_z)[0] == cpu.F_ZERO_FREQ
    b[20] = N_SYM
    assert encode_ref(c, cum, total, b, idx)[0] == cpu.F_BAD_SYMBOL
    m[30] = K
    assert encode_ref(c, cum, total, syms, m)[0] == cpu.F_BAD_MODEL
    # the earliest wins, whatever its kind; at one symbol the model is looked up first
    z2 = z.copy()
    z2[20] = N_SYM
    assert encode_ref(c, cum, total, z2, idx_z)[0] == cpu.F_ZERO_FREQ
    b2 = b.copy()
    b2[40], iz = 2, idx.copy()
    iz[40] = 2
    assert encode_ref(c, cum, total, b2, iz)[0] == cpu.F_BAD_SYMBOL
    both_s, both_i = syms.copy(), idx.copy()
    both_s[5], both_i[5] = N_SYM, K
    assert encode_ref(c, cum, total, both_s, both_i)[0] == cpu.F_BAD_MODEL


def test_decode_errors():
    rng = np.random.default_rng(8)
    c, cum, total, syms, idx = _draw(rng, 200)
    f, code = encode_ref(c, cum, total, syms, idx)
    assert f == 0
    bad = idx.copy()
    bad[50] = len(C_ROWS)
    f, out = decode_ref(c, cum, total, code, bad)
    assert f == cpu.F_BAD_MODEL and list(out) == list(syms[:50])
    # a truncated stream runs dry first
    f, out = decode_ref(c, cum, total, code[:12], bad)
    assert f == cpu.F_TRUNCATED and len(out) < 50
    # Decoder::new needs 8 bytes even for an empty chunk
    assert decode_ref(c, cum, total, b"\0" * 7, [])[0] == cpu.F_TRUNCATED
    assert decode_ref(c, cum, total, b"\0" * 8, [])[0] == 0
