"""Generates tests/golden/adaptive_fixtures.json (committed).  Run from the repo root:

    python tests/golden/make_adaptive_fixtures.py

Directed streams for the adaptive coder (rc_adaptive.hip).  Random data meets a
range_reduction_expansion (range_coder.rs:126-135) about once per 2,000 symbols, nearly always
at symbol 0 of a chunk, so the decoder's `while (d.range < TOP16)` loop and the encoder's
enc_reduce inside the unrolled FIFO step run mid-stream a few times per launch, at whatever
phase chance gives.  These streams are steered into them: after a warm-up of one repeated
symbol (which raises the total, so that every other symbol narrows the range by ~2^-15), each
next symbol is picked greedily against tests/adaptive_ref.py: the symbols are tried in a seeded
order and the first whose step ends in m > 0 rare bytes is taken, else the first tried.  Where
a set wants events at consecutive indices, the pick looks two symbols ahead: of the symbols
with m > 0 it prefers one after which some symbol has m > 0 again.

Each set runs until its conditions (tests/adaptive_cases.py: CONDITIONS, asserted again over the
committed file by tests/test_adaptive_ref.py) hold over its chunks, within 2,000 symbols per
chunk.  The code of every chunk comes from the C oracle and must equal the Python reference's.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import cpu  # noqa: E402
import adaptive_ref as ar  # noqa: E402
from adaptive_cases import CONDITIONS, SETS as SET_PARAMS, holds, measure  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_CHUNK = 2000

# the chunks of each set (parameters: adaptive_cases.SETS) as (seed, warm-up length, warm-up
# symbol, fewest steered symbols)
CHUNKS = {
    "A": [(11, 1500, 3, 300), (12, 700, 255, 200), (13, 0, 0, 150)],
    "B": [(21, 1500, 199, 300), (22, 600, 0, 200), (23, 0, 0, 150)],
    "C": [(31, 1500, 50, 300), (32, 900, 99, 300), (33, 0, 0, 150)],
    "D": [(41, 0, 0, 250), (42, 40, 128, 250)],
    "E": [(51, 0, 0, 250), (52, 40, 64, 250)],
}


class Stream:
    """One chunk being built: the model, the coder state and the events so far."""

    def __init__(self, params):
        self.md = ar.Model(*params)
        self.low, self.rng = 0, ar.M64
        self.syms, self.rare_at, self.halve_at = [], [], []

    def push(self, s):
        i = len(self.syms)
        self.low, self.rng, _, _, m = ar.param_update(self.low, self.rng, self.md.c[s],
                                                      sum(self.md.c[:s]), self.md.total)
        if m:
            self.rare_at.append(i)
        if self.md.update(s, i):
            self.halve_at.append(i)
        self.syms.append(s)

    def rare_symbols(self, order):
        """The symbols of `order` whose step from this state ends in m > 0."""
        cum = self.md.cum()
        return [s for s in order
                if ar.param_update(self.low, self.rng, self.md.c[s], cum[s], self.md.total)[4]]

    def after(self, s):
        t = Stream.__new__(Stream)
        t.md, t.low, t.rng = self.md.clone(), self.low, self.rng
        t.syms, t.rare_at, t.halve_at = list(self.syms), [], []
        t.push(s)
        return t


def pick(st, rs, want_pair):
    n = st.md.n
    order = rs.sample(range(n), n)
    hits = st.rare_symbols(order)
    if not hits:
        return order[0]
    if want_pair:  # two ahead: an event now after which another is possible at once
        for s in hits[:8]:
            if st.after(s).rare_symbols(range(n)):
                return s
    return hits[0]


def build_set(name):
    params, want = SET_PARAMS[name][0], CONDITIONS[name]
    done = []
    out = []
    for seed, warm, wsym, least in CHUNKS[name]:
        rs = random.Random(seed)
        st = Stream(params)
        for _ in range(warm):
            st.push(wsym)
        while len(st.syms) < MAX_CHUNK:
            got = measure(done + [(st.rare_at, st.halve_at)])
            if holds(got, want) and len(st.syms) - warm >= least:
                break
            st.push(pick(st, rs, want.get("pairs", 0) > got["pairs"]))
        done.append((st.rare_at, st.halve_at))
        out.append(st)
    got = measure(done)
    assert holds(got, want), (name, got, want)
    return out, got


def main():
    sets = {}
    for name, (params, decoder) in SET_PARAMS.items():
        streams, got = build_set(name)
        n, inc, limit, period = params
        chunks = []
        for st in streams:
            f, code, L = cpu.encode_adaptive(n, inc, limit, period, bytes(st.syms))
            e = ar.encode(n, inc, limit, period, st.syms)
            assert f == 0 and code == e.code and L == e.out_len
            assert e.rare_at == st.rare_at and e.halve_at == st.halve_at
            mid = [i for i in e.rare_at if i > 0]
            chunks.append(dict(symbols_hex=bytes(st.syms).hex(), encoded_hex=code.hex(),
                               rare_at=e.rare_at, halve_at=e.halve_at, rare_count=len(mid)))
            print(f"set {name}: {len(st.syms)} symbols, {len(code)} B, {len(mid)} mid-stream "
                  f"events, {len(e.halve_at)} halvings")
        print(f"set {name}: {got}")
        sets[name] = dict(n_alpha=n, inc=inc, limit=limit, period=period,
                          decoder=decoder, coverage=got, chunks=chunks)
    with open(os.path.join(HERE, "adaptive_fixtures.json"), "w") as f:
        json.dump(dict(conditions=CONDITIONS, sets=sets), f, separators=(",", ":"))
    print("bytes:", os.path.getsize(os.path.join(HERE, "adaptive_fixtures.json")))


if __name__ == "__main__":
    main()
