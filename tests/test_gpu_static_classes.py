"""The single-table static coders at every model class, on both sides of every threshold of
rc_model_create_static and for totals above 2^16 (the wide bucket class: both divisions, the
rare-heavy worst case of its ring margins, the split seam of its bucket entries, total 2^32 - 1):
the cases of tests/static_cases.py against the oracle, bit-exact.  tests/test_static_cases.py
shows without a device that each case reaches the class and the table entries it is meant to."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import run_decode, run_encode  # noqa: E402
import static_cases as S  # noqa: E402

NAMES = [c.name for c in S.CASES]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


_ref = {}


def oracle_codes(name, chunks=None, key=None):
    """[(flags, bytes, length)] of the case's chunks from the oracle (computed once)."""
    key = key or ("case", name)
    if key not in _ref:
        c, cum, total = S.table(name)
        _ref[key] = [cpu.encode(c, cum, total, ch) for ch in (chunks or S.chunks(name))]
    return _ref[key]


def _seed(name):
    return S.seed_of(name) & 0xFFFF


def _check_both_ways(name, chunks, want, misalign):
    """Encoder flags, lengths and bytes equal the oracle's for every chunk; the decoder returns
    flag 0 and the symbols."""
    c, cum, total = S.table(name)
    m = rc.StaticModel(c, cum, total)
    lens = [len(ch) for ch in chunks]
    caps = [rc.slot_capacity(L, m.max_bits_per_symbol() + 1) for L in lens]
    out, out_off, ol, fl = run_encode(m, chunks, caps, misalign=misalign, seed=_seed(name))
    for k, (f, b, L) in enumerate(want):
        assert f == 0 and (fl[k], ol[k]) == (0, L), (name, k, fl[k], ol[k], L)
        assert bytes(out[out_off[k]:out_off[k] + L]) == b, (name, k)
    dec, fd = run_decode(m, [b for _, b, _ in want], lens, misalign=misalign,
                         seed=_seed(name) + 1)
    for k, ch in enumerate(chunks):
        assert fd[k] == 0 and (dec[k] == ch).all(), (name, k, fd[k])
    m.close()


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_case_matches_the_oracle(ctx, name, misalign):
    _check_both_ways(name, S.chunks(name), oracle_codes(name), misalign)


@pytest.mark.parametrize("name", S.GARBAGE_CASES)
def test_garbage_and_truncated_streams(ctx, name):
    """Arbitrary bytes, and sound streams cut by 0 .. 5 bytes (never below 8): the flags are the
    oracle's, and so are the symbols wherever the oracle decodes."""
    c, cum, total = S.table(name)
    m = rc.StaticModel(c, cum, total)
    codes, counts = S.garbage(name)
    chunks = S.chunks(name)
    cut = [b[:max(8, L - x)] for (_, b, L), x in zip(oracle_codes(name), S.cuts(name))]
    for streams, ns, mis in ((codes, counts, False), (codes, counts, True),
                             (cut, [len(ch) for ch in chunks], True)):
        dec, fd = run_decode(m, streams, ns, misalign=mis, seed=_seed(name) + 2)
        for k in range(len(streams)):
            f, d = cpu.decode(c, cum, total, streams[k], ns[k])
            assert fd[k] == f, (name, k, fd[k], f)
            if f == 0:
                assert (dec[k] == d).all(), (name, k)
    m.close()


def test_capacity_above_2_16(ctx):
    """The rare-heavy model at total 2^32 - 1 (4 bytes per symbol) into slots one byte and 17
    bytes short of the stream among exact ones: RC_F_CAPACITY with the exact length, the first
    cap bytes as the oracle's, and the chunks next to a short one untouched (the slots lie back
    to back, the last one is short too, and run_encode checks the bytes around them)."""
    name = "t4294967295_rare"
    c, cum, total = S.table(name)
    m = rc.StaticModel(c, cum, total)
    chunks = S.chunks(name)
    want = oracle_codes(name)
    short = {1: 1, 6: 1, 13: 1, 3: 17, 8: 17, 12: 17}
    caps = [L - short.get(k, 0) for k, (_, _, L) in enumerate(want)]
    assert min(caps) >= 7 and len(chunks) == 14
    for mis in (False, True):
        out, out_off, ol, fl = run_encode(m, chunks, caps, misalign=mis, seed=5)
        for k, (f, b, L) in enumerate(want):
            assert f == 0 and ol[k] == L, (k, ol[k], L)
            assert fl[k] == (rc.api.N.F_CAPACITY if k in short else 0), (k, fl[k])
            # (the oracle itself, given the short slot)
            assert cpu.encode(c, cum, total, chunks[k], cap=caps[k])[0] == fl[k], k
            assert bytes(out[out_off[k]:out_off[k] + caps[k]]) == b[:caps[k]], k
    m.close()


@pytest.mark.parametrize("pair", S.SEAM_PAIRS, ids=["255|256", "512|513", "2048|2049",
                                                    "65536|65537"])
def test_seam_pairs(ctx, pair):
    """The same symbols under the two totals next to a threshold, each against the oracle:
    neither side borrowed the other's table format."""
    chunks = S.seam_chunks(pair)
    for name in pair:
        want = oracle_codes(name, chunks, key=("seam", name))
        _check_both_ways(name, chunks, want, misalign=True)
    a, b = (_ref["seam", n] for n in pair)
    assert any(x[1] != y[1] for x, y in zip(a, b))  # (the two tables do code differently)
