"""Cases shared by tests/test_adaptive_ref.py (CPU) and tests/test_gpu_adaptive_directed.py:
the steered fixtures of tests/golden/adaptive_fixtures.json with the coverage they must reach,
and the bad streams (garbage, saturated, truncated) that both decode.  The CPU test proves from
adaptive_ref which branches these inputs reach; the GPU test runs the very same inputs.

Nothing here imports the package under test.
"""
import json
import os

import numpy as np

C4 = (32, 57343, 256)  # increment, limit, period

# the parameter sets of test_gpu_adaptive.PARAMS (test_gpu_adaptive_directed asserts they agree)
PARAMS = [(256, *C4), (2, 1, 300, 1), (17, 5, 1000, 4), (1, 7, 600, 8), (256, 255, 8160, 16),
          (40, 32, 8192, 64), (256, 1, 300, 1), (128, *C4), (100, *C4), (129, *C4),
          (128, 255, 8160, 16)]

# fixture sets: (n, inc, limit, period) and the decoder instantiation they select
SETS = {
    "A": ((256, *C4), "<1, 256>"),
    "B": ((200, *C4), "<0, 256>"),
    "C": ((100, *C4), "<0, 128>"),
    "D": ((256, 255, 8160, 16), "<1, 256>"),   # a halving at every period end
    "E": ((128, 255, 8160, 16), "<0, 128>"),
}

# What each set's chunks must reach together, in the terms of measure().  E's event count is
# the count asked of D: the search reaches 40 within 540 symbols, so nothing was lowered.
CONDITIONS = {
    "A": dict(events=32, residues=16, pairs=1),
    "B": dict(events=32, residues=16),
    "C": dict(events=32, residues=16),
    "D": dict(events=16, halvings=8, after_halving=1),
    "E": dict(events=16, halvings=8, after_halving=1),
}


def measure(chunks):
    """The coverage of chunks given as (rare_at, halve_at) pairs: mid-stream events (m > 0 at
    an index > 0), the residues mod 16 of their indices (hence every FIFO slot mod 8), pairs of
    events at consecutive indices, halvings, and events within 2 symbols after a halving."""
    ev = pairs = halv = after = 0
    seen = set()
    for rare_at, halve_at in chunks:
        mid = [i for i in rare_at if i > 0]
        ms, hs = set(mid), set(halve_at)
        ev += len(mid)
        seen.update(i % 16 for i in mid)
        pairs += sum(1 for i in mid if i + 1 in ms)
        halv += len(halve_at)
        after += sum(1 for i in mid if i - 1 in hs or i - 2 in hs)
    return dict(events=ev, residues=len(seen), pairs=pairs, halvings=halv, after_halving=after)


def holds(got, want):
    return all(got[k] >= v for k, v in want.items())


def load_fixtures(golden_dir):
    """{set name: dict(params, chunks)} with each chunk's symbols (u8 array) and code (bytes)
    beside its recorded rare_at, halve_at and rare_count."""
    with open(os.path.join(golden_dir, "adaptive_fixtures.json")) as f:
        raw = json.load(f)
    out = {}
    for name, s in raw["sets"].items():
        chunks = [dict(symbols=np.frombuffer(bytes.fromhex(c["symbols_hex"]), np.uint8),
                       code=bytes.fromhex(c["encoded_hex"]), rare_at=c["rare_at"],
                       halve_at=c["halve_at"], rare_count=c["rare_count"])
                  for c in s["chunks"]]
        out[name] = dict(params=(s["n_alpha"], s["inc"], s["limit"], s["period"]),
                         decoder=s["decoder"], chunks=chunks)
    return raw["conditions"], out


def zipf_syms(rng, n_alpha, n, s=1.2):
    w = 1.0 / np.arange(1, n_alpha + 1) ** s
    return rng.choice(n_alpha, size=n, p=w / w.sum()).astype(np.uint8)


# ---- bad streams: one entry per decoder variant and halving rhythm ----
BAD_VARIANTS = [(n, *q) for n in (256, 200, 100) for q in (C4, (255, 8160, 16))]
BAD_COUNT = 500  # symbols decoded from every garbage stream


def valid_stream(params, fixtures, encode):
    """One valid stream of the variant: its fixture set's shortest chunk where a set has these
    parameters, else a Zipf chunk of 300 symbols coded by `encode` (the oracle)."""
    for name, (p, _) in SETS.items():
        if p == tuple(params):
            ch = min(fixtures[name]["chunks"], key=lambda c: len(c["symbols"]))
            return ch["symbols"], ch["code"]
    rng = np.random.default_rng(params[0] + params[1])
    syms = zipf_syms(rng, params[0], 300)
    f, code, _ = encode(*params, syms)
    assert f == 0
    return syms, code


def bad_streams(params, fixtures, encode):
    """(garbage, truncated) for one variant.  garbage: 64 streams of 40-600 bytes, each decoded
    for BAD_COUNT symbols: 44 of random bytes, 6 of 0xFF bytes only, 14 of 8-20 0xFF bytes before
    a valid tail.  Data of 8 0xFF bytes is x = 2^64 - 1 >= r * total at symbol 0, whatever the
    total, so the 20 streams that start with them reach the clamp.  truncated: (code, count) of
    the valid stream cut to 0..24 bytes and to len - 1, len - 2, len - 3 and len // 2."""
    n, inc = params[0], params[1]
    rng = np.random.default_rng(7000 + n + inc)
    syms, code = valid_stream(params, fixtures, encode)
    garbage = [bytes(rng.integers(0, 256, int(rng.integers(40, 601))).astype(np.uint8))
               for _ in range(44)]
    garbage += [b"\xff" * L for L in (40, 41, 63, 64, 333, 600)]
    for j in range(14):
        pre = 8 + (j % 13)
        tail = code[int(rng.integers(0, 8)):]
        garbage.append((b"\xff" * pre + tail)[:600])
    order = rng.permutation(len(garbage))
    garbage = [garbage[i] for i in order]
    L = len(code)
    cuts = list(range(25)) + [L - 1, L - 2, L - 3, L // 2]
    truncated = [(code[:c], len(syms)) for c in cuts]
    return garbage, truncated
