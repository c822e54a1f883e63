"""tests/adaptive_ref.py against the C oracle, and what the directed adaptive inputs reach.

The GPU tests of tests/test_gpu_adaptive_directed.py are named for branches of rc_adaptive.hip
(range_reduction_expansion mid-stream, halvings, the clamp of the exact target to total - 1).
Whether an input reaches such a branch is decided here, on the CPU, from the event reference:
the committed fixtures must replay to their recorded events and meet their coverage
conditions, and the bad streams must reach the clamp on every decoder variant."""
import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_ref as ar
from oracle import cpu


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return ac.load_fixtures(golden_dir)


def chunk_lengths(rng, params):
    period = params[3]
    lens = [0, 1, 2, period - 1, period, period + 1, 2 * period + 1]
    lens += list(rng.integers(0, 700, 16))
    if params[1:] == ac.C4:
        lens.append(2000)  # the first halving of C4 comes after ~1,790 symbols
    return [int(L) for L in lens if L >= 0]


@pytest.mark.parametrize("params", ac.PARAMS)
def test_ref_vs_oracle(params):
    """Bytes, lengths and flags of ~24 chunks per parameter set (264 in all), with lengths 0, 1
    and period +- 1, and the decode of each code and of its truncations."""
    n = params[0]
    rng = np.random.default_rng(n * 1000 + params[1])
    halved = 0
    for L in chunk_lengths(rng, params):
        syms = ac.zipf_syms(rng, n, L, s=float(rng.uniform(0.0, 1.6)))
        f, code, ol = cpu.encode_adaptive(*params, syms)
        e = ar.encode(*params, syms)
        assert (e.flag, e.code, e.out_len) == (f, code, ol) and f == 0, L
        assert sum(k + m for k, m in e.km) == len(code) - 8
        assert len(e.km) == len(e.totals) == L
        assert all(i % params[3] == params[3] - 1 for i in e.halve_at)
        # the total starts at n and grows by inc per symbol, except across a halving
        assert e.totals[:1] == [n][:L]
        assert all(b - a == params[1] for i, (a, b) in enumerate(zip(e.totals, e.totals[1:]))
                   if i not in e.halve_at)
        assert all(t < 65536 - params[1] for t in e.totals)  # what the u16 counts rely on
        assert all(e.totals[i + 1] < e.totals[i] for i in e.halve_at if i + 1 < L)
        halved += len(e.halve_at)
        for cut in {len(code), len(code) - 1, len(code) // 2, 7}:
            fo, do = cpu.decode_adaptive(*params, code[:cut], L)
            fr, dr, clamp = ar.decode(*params, code[:cut], L)
            assert fr == fo and not clamp, (L, cut)
            if fo == 0:
                assert dr == list(do) == list(syms)
    assert halved > 0  # every parameter set halves within these lengths


def test_ref_flags():
    """A symbol outside the alphabet and a slot too small, as the oracle reports them."""
    params = (100, *ac.C4)
    rng = np.random.default_rng(5)
    syms = ac.zipf_syms(rng, 100, 300)
    for p in (0, 1, 7, 8, 299):
        bad = syms.copy()
        bad[p] = 100 + p % 100
        f, code, ol = cpu.encode_adaptive(*params, bad)
        e = ar.encode(*params, bad)
        assert (e.flag, e.code, e.out_len) == (f, code, ol) and f == ar.F_BAD_SYMBOL
    for cap in (0, 1, 8, 63):
        f, code, ol = cpu.encode_adaptive(*params, syms, cap=cap)
        e = ar.encode(*params, syms, cap=cap)
        assert (e.flag, e.code[:cap], e.out_len) == (f, code, ol) and f == ar.F_CAPACITY


def test_fixtures_replay(fixtures):
    """The committed fixtures replay to their recorded events and code, through the reference
    and through the oracle, and meet the coverage conditions of their sets."""
    cond, sets = fixtures
    assert cond == ac.CONDITIONS and set(sets) == set(ac.SETS)
    # the conditions themselves: A, B and C 32 mid-stream events over every residue mod 16 (A
    # with a pair at consecutive indices); D and E 16 events, 8 halvings and an event within 2
    # symbols after a halving
    assert ac.CONDITIONS["A"] == dict(events=32, residues=16, pairs=1)
    assert ac.CONDITIONS["B"] == ac.CONDITIONS["C"] == dict(events=32, residues=16)
    assert ac.CONDITIONS["D"] == ac.CONDITIONS["E"] == dict(events=16, halvings=8,
                                                           after_halving=1)
    for name, s in sets.items():
        assert (s["params"], s["decoder"]) == ac.SETS[name]
        n = s["params"][0]
        assert s["decoder"] == ("<1, 256>" if n == 256 else "<0, 128>" if n <= 128
                                else "<0, 256>")  # rc_adaptive_decode_launch
        events = []
        for c in s["chunks"]:
            assert len(c["symbols"]) <= 2000
            e = ar.encode(*s["params"], c["symbols"])
            assert e.flag == 0 and e.code == c["code"]
            assert e.rare_at == c["rare_at"] and e.halve_at == c["halve_at"]
            assert c["rare_count"] == sum(1 for i in e.rare_at if i > 0)
            f, code, ol = cpu.encode_adaptive(*s["params"], c["symbols"])
            assert f == 0 and code == c["code"]
            f, d = cpu.decode_adaptive(*s["params"], c["code"], len(c["symbols"]))
            assert f == 0 and bytes(d) == bytes(c["symbols"])
            f, d, clamp = ar.decode(*s["params"], c["code"], len(c["symbols"]))
            assert f == 0 and d == list(c["symbols"]) and not clamp
            events.append((e.rare_at, e.halve_at))
        got = ac.measure(events)
        print(name, got)
        assert ac.holds(got, ac.CONDITIONS[name]), (name, got)


def test_measure():
    got = ac.measure([([0, 5, 6, 40], [3, 38]), ([0], [])])
    assert got == dict(events=3, residues=3, pairs=1, halvings=2, after_halving=2)


@pytest.mark.parametrize("params", ac.BAD_VARIANTS)
def test_bad_streams_reach_the_clamp(fixtures, params):
    """The streams of the GPU test's group (d): the reference's flags and symbols equal the
    oracle's, and x / r >= total (the kernels' qe = total - 1) occurs on this variant: at
    symbol 0 of the 20 streams that begin with 8 0xFF bytes, and on one stream or more past
    symbol 0."""
    garbage, truncated = ac.bad_streams(params, fixtures[1], cpu.encode_adaptive)
    assert len(garbage) == 64 and all(40 <= len(g) <= 600 for g in garbage)
    at0 = later = 0
    for g in garbage:
        fo, do = cpu.decode_adaptive(*params, g, ac.BAD_COUNT)
        fr, dr, clamp = ar.decode(*params, g, ac.BAD_COUNT)
        assert fr == fo
        if fo == 0:
            assert dr == list(do)
        assert (g[:8] == b"\xff" * 8) == (0 in clamp)
        at0 += 0 in clamp
        later += any(i > 0 for i in clamp)
    assert at0 == 20 and later >= 1
    assert [len(c) for c, _ in truncated][:25] == list(range(25))
    flags = []
    for code, count in truncated:
        fo, do = cpu.decode_adaptive(*params, code, count)
        fr, dr, clamp = ar.decode(*params, code, count)
        assert fr == fo and not clamp
        flags.append(fo)
    assert flags[:8] == [ar.F_TRUNCATED] * 8 and ar.F_TRUNCATED in flags[8:]
