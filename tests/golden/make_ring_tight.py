"""Generates tests/golden/ring_tight.json (committed).  Run from the repo root:

    python tests/golden/make_ring_tight.py

Tight streams for the code rings of all four static-model decoders.  The older
ring fixtures (make_ring_fixtures.py) put a range_reduction_expansion at every span offset, but
at the head they were steered for their rings are never low when the heavy spans come: no
lowered ring need makes one of them under-run there.  These streams are steered the other way
round: each is built for one (schedule, align, head) of tests/ring_sim.py so that a ring check
finds just enough bytes staged to pass a lowered need and the symbols up to the next check then
settle more than that.  What a stream reaches is its tightness (ring_sim.tightness): the largest
need below the shipped one at which the replay under-runs.

What can be reached.  Symbols 1..255 (c = 1) narrow the range by the total, 2 bytes' worth, and
the range stays in [2^48, 2^64): s of them settle 2 s no-carry bytes, one more if the range was
below 2^56 before them and is not after.  A range_reduction_expansion stages its own bytes plus
the rare need before it reads them.  So the 8 symbols behind a span check settle at most 17 bytes
unchecked and the span need (24) binds at 16 at the most; the single symbol behind a head or
tail check settles 3, the 4 behind a rolled-path check 9: the need of 12 binds at 2, or at 8 on
the rolled path, whose span check is followed by 4 symbols and a check of 12, so that its span
need cannot bind at all.  The rare need binds only where a span holds expansions enough to
settle more than the 24 bytes its check staged; the search below has not met one (the values
reached are recorded as they come, 0 included).

The search (steer) is breadth first over the coder's next symbols, one stream kept per (staged
bytes, pending refills, range below 2^56 or not) of the replay with the lowered need: symbol 0
(settles nothing), one symbol per (bytes settled, range left low or not), and a symbol that ends
in an expansion (it leaves the range at another fraction of a byte, without which most
(align, head) never see a span check at exactly 16 bytes).  Wherever a check finds exactly the
lowered need staged, the symbols that settle the most bytes follow (probe).  A stream is steered
for the span need first (the rolled path's streams under the same kernel's unrolled schedule,
which they also run through), then for the need of 12 where checks of it are left, then for the
rare need at 0; the rest is the usual mix, with expansions at the span offsets its schedule's
streams lack.  Where no stream is found at the alignment wanted, the next one is taken.

Two models: the ring fixtures' table (n = 256, total 2^16, c = [65281, 1 x 255]) and the same
shape with total 65535, which the decoders divide by with their non-power-of-two code.  The
coder state comes from a u64 restatement of param_update (range_coder.rs:53-92), checked byte
for byte against the C oracle.
"""
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import cpu  # noqa: E402
import ring_sim  # noqa: E402

M64 = (1 << 64) - 1
TOP8 = 1 << 56
TOP16 = 1 << 48
U64 = np.uint64
HERE = os.path.dirname(os.path.abspath(__file__))
N = 256
MODELS = {"pow2": 65536, "magic": 65535}
ALIGNS = [0, 1, 31, 33, 63, 26, 47, 58]
# (schedule, heads) per model: head 0, an odd small head, the largest; wide heads are in 2-byte
# symbols, and 29 is the head of an output 3 symbols past a 64-B boundary
PLAN = {"pow2": [("static", (0, 5, 63)), ("indexed", (0, 5, 63)), ("indexed_rolled", (0, 5, 63)),
                 ("order1", (0, 5, 63)), ("wide", (0, 1, 29, 31))],
        "magic": [("static", (0, 63)), ("indexed", (5,)), ("indexed_rolled", (0, 63)),
                  ("order1", (5,)), ("wide", (1, 31))]}
# the lowered needs steered against, from the most each can bind at (the module docstring)
SPAN_NEED = 16
HEAD_NEEDS = {False: (2, 1), True: (8, 7, 6)}
# the rolled path is a path of k_decode_indexed: its streams are steered for the span need under
# that kernel's unrolled schedule, which the same streams also run through
UNROLLED = {"indexed_rolled": "indexed"}


def table(total):
    c = [total - 255] + [1] * 255
    return c, [0] + [total - 255 + i for i in range(255)]


class Model:
    def __init__(self, total):
        self.total = total
        self.c, self.cum = table(total)
        self.c_v = np.array(self.c, U64)
        self.cum_v = np.array(self.cum, U64)

    def step(self, low, rng, s):
        """param_update (range_coder.rs:53-92) for symbol s: (low, range, k no-carry bytes,
        m rare bytes)."""
        r = rng // self.total
        rng = r * self.c[s]
        low = low + r * self.cum[s]
        assert low <= M64
        k = 0
        while (low ^ (low + rng)) < TOP8:
            low = (low << 8) & M64
            rng = (rng << 8) & M64
            k += 1
        m = 0
        while rng < TOP16:
            rng = (~low & M64) & (TOP16 - 1)
            low = (low << 8) & M64
            rng = (rng << 8) & M64
            m += 1
        return low, rng, k, m

    def vstep(self, low, rng):
        """step() for all 256 symbols at once (numpy u64, wrapping like the reference's u64)."""
        r = U64(rng // self.total)
        R = r * self.c_v
        L = U64(low) + r * self.cum_v
        k = np.zeros(256, np.int64)
        m = np.zeros(256, np.int64)
        for _ in range(8):
            sh = (L ^ (L + R)) < U64(TOP8)
            k += sh
            L = np.where(sh, L << U64(8), L)
            R = np.where(sh, R << U64(8), R)
        for _ in range(8):
            sh = R < U64(TOP16)
            m += sh
            R2 = (~L) & U64(TOP16 - 1)
            L = np.where(sh, L << U64(8), L)
            R = np.where(sh, R2 << U64(8), R)
        return L, R, k, m


class Stream:
    """Coder state, the shipped schedule's replay and one replay with a lowered need."""

    def __init__(self, model, schedule, align, head):
        self.model = model
        self.low, self.rng = 0, M64
        self.syms, self.km = [], []
        self.where = (N, align, head)
        self.schedule = schedule
        self.shipped = ring_sim.Replay(N, align, head, schedule=schedule)
        self.aim = None

    def take_aim(self, arg, v, schedule=None):
        """Steer against need `arg` lowered to v from here on (the replay catches up)."""
        self.aim = ring_sim.Replay(*self.where, schedule=schedule or self.schedule, **{arg: v})
        self.aim_need = v
        for k, m in self.km:
            self.aim.step(k, m)

    def clone_fresh(self):
        """A copy of a stream that has not taken aim yet."""
        t = copy.copy(self)
        t.aim = self.shipped
        return t.clone()

    def clone(self):
        t = copy.copy(self)
        t.syms, t.km = list(self.syms), list(self.km)
        t.shipped = ring_clone(self.shipped)
        t.aim = ring_clone(self.aim)
        return t

    def push(self, s):
        self.low, self.rng, k, m = self.model.step(self.low, self.rng, s)
        self.syms.append(s)
        self.km.append((k, m))
        self.shipped.step(k, m)
        self.aim.step(k, m)
        return k, m

    def left(self):
        return N - len(self.syms)


def ring_clone(g):
    h = copy.copy(g)
    h.under, h.over = list(g.under), list(g.over)
    return h


def most_bytes(st, rs, rare_ok):
    """The symbol that settles the most no-carry bytes from this state, preferring one that
    leaves range < 2^56 (so that the next c = 1 symbol settles 3 bytes); ties at random.  A
    symbol that ends in a range_reduction_expansion refills the ring: only if rare_ok."""
    _, R, k, m = st.model.vstep(st.low, st.rng)
    score = 4 * k + ((R < U64(TOP8)) & (m == 0))
    score = score + 2 * m if rare_ok else score - 64 * (m > 0)
    return int(rs.choice(np.flatnonzero(score == score.max())))


def probe(st, rs, rare_ok):
    """The symbols that settle the most bytes, up to 8 of them: the advanced stream if the
    lowered replay under-runs on the way, else None."""
    t = st.clone()
    seen = len(t.aim.under)
    for _ in range(min(8, t.left())):
        t.push(most_bytes(t, rs, rare_ok))
        if len(t.aim.under) > seen:
            return t
    return None


def at_check(st, arg):
    """Whether a ring check of the need `arg` comes before the next symbol (the rare path's
    need is checked wherever an expansion falls)."""
    so = st.shipped.span_offset()
    if arg == "need_span":
        return so == 0
    if arg == "need_head":
        return so is None or (st.shipped.rolled and so % 4 == 0)
    return True


def moves(st, rs, rare_ok):
    """The kinds of next symbol this state offers, one symbol of each: symbol 0 (settles next to
    nothing), one symbol per (no-carry bytes, range left below 2^56 or not) among the others, and
    if rare_ok one that ends in the longest range_reduction_expansion."""
    _, R, k, m = st.model.vstep(st.low, st.rng)
    kind = np.where(m > 0, 8, 2 * k + (R < U64(TOP8)))
    kind[0] = 9
    out = [0]
    for q in np.unique(kind[1:]):
        if q == 8:
            if rare_ok:
                out.append(int(rs.choice(np.flatnonzero((m == m.max()) & (kind == 8)))))
        else:
            out.append(int(rs.choice(np.flatnonzero(kind == q))))
    return out


def steer(st, rs, arg, v, upto, rare_ok=False, schedule=None):
    """Search from st, breadth first, for a stream that under-runs with need `arg` lowered to
    v, among streams of at most `upto` symbols.  The frontier holds one stream per (staged
    bytes, pending refills, range below 2^56 or not) of the lowered replay, symbol by symbol;
    wherever a ring check finds just v bytes staged, a probe.  Returns (stream, found): the
    probe's stream, else st as it came."""
    st.take_aim(arg, v, schedule)
    front = [st]
    while front and len(front[0].syms) + 1 < upto:
        new = {}
        for f in front:
            for s in moves(f, rs, rare_ok):
                t = f.clone()
                t.push(s)
                key = (t.aim.unread(), t.aim.pend_ok, t.rng < TOP8)
                if key in new:
                    continue
                new[key] = t
                if at_check(t, arg) and t.aim.unread() == v and len(t.syms) + 1 < upto:
                    hit = probe(t, rs, rare_ok)
                    if hit is not None and len(hit.syms) <= upto:
                        return hit, True
        front = [new[k] for k in sorted(new)]
    return st, False


def fill(st, rs, upto, missing):
    """The usual mix up to `upto` symbols, taking a range_reduction_expansion where the state
    offers one: always at a span offset in `missing` (those the schedule's streams have no event
    at yet), else every other time."""
    while len(st.syms) < upto:
        _, _, _, m = st.model.vstep(st.low, st.rng)
        so = st.shipped.span_offset()
        if m.max() > 0 and (so in missing or rs.random() < 0.5):
            st.push(int(rs.choice(np.flatnonzero(m == m.max()))))
            missing.discard(so)
        else:
            s = 0 if rs.random() < 0.3 else int(rs.integers(1, 256))
            if so is not None and (so + 1) % ring_sim.DEC_CHECK_SPAN in missing:
                # one symbol ahead: a symbol after which the state offers an expansion
                for s1 in rs.permutation(256)[:32]:
                    low, rng, _, m1 = st.model.step(st.low, st.rng, int(s1))
                    if not m1 and st.model.vstep(low, rng)[3].max() > 0:
                        s = int(s1)
                        break
            st.push(s)
    return st


def chunk(seed, model, schedule, align, head, missing):
    """A stream steered for (schedule, align, head): the span need first (at 16, the most a
    span can reach; for the rolled path, whose span need cannot bind, under the same kernel's
    unrolled schedule), then the need of 12 where the schedule has such checks left (the rolled
    path's, every 4 symbols; else the tail's), then the rare path's need at 0."""
    rs = np.random.default_rng(seed)
    st = Stream(model, schedule, align, head)
    rolled = st.shipped.rolled
    unrolled = UNROLLED.get(schedule, schedule)
    ok = False
    if head >= 20:  # a long head: the need of 12 inside it first, if the span need binds after
        for v in HEAD_NEEDS[False]:
            t, ok = steer(st.clone_fresh(), rs, "need_head", v, head)
            if ok:
                t, ok = steer(t, rs, "need_span", SPAN_NEED, N, rare_ok=True, schedule=unrolled)
            if ok:
                st = t
                break
    if not ok:
        st, ok = steer(st, rs, "need_span", SPAN_NEED, N, rare_ok=True, schedule=unrolled)
    assert ok, "no span under-run found"
    tail = (N - head) % 16
    if not rolled and tail > 1:
        st.take_aim("need_span", SPAN_NEED)
        st = fill(st, rs, N - tail - 24, missing)
    if rolled or tail > 1:
        for v in HEAD_NEEDS[rolled]:
            st, ok = steer(st, rs, "need_head", v, N if not rolled else min(N, len(st.syms) + 96),
                           rare_ok=rolled)
            if ok:
                break
    if st.left() > 16:
        st, ok = steer(st, rs, "need_rare", 0, min(N, len(st.syms) + 40), rare_ok=True)
    st.take_aim("need_span", SPAN_NEED)
    st = fill(st, rs, N, missing)
    assert not st.shipped.under and not st.shipped.over
    return st


def main():
    models = {name: Model(total) for name, total in MODELS.items()}
    chunks = []
    reached = {}
    covered = {}  # per schedule: the span offsets at which its streams hold a rare event
    ci = 0
    for mname, model in models.items():
        for schedule, heads in PLAN[mname]:
            for head in heads:
                # the align wanted, else the next one at which the search finds a stream (the
                # span need binds only at some (align, head): DESIGN.md section 5.2)
                for j in range(len(ALIGNS)):
                    align = ALIGNS[(ci + j) % len(ALIGNS)]
                    try:
                        missing = set(range(ring_sim.DEC_CHECK_SPAN)) - covered.setdefault(
                            schedule, set())
                        st = chunk(2000 + ci, model, schedule, align, head, missing)
                        break
                    except AssertionError:
                        print(f"  ({schedule}, align {align}, head {head}): no stream found")
                else:
                    raise SystemExit("no align serves")
                ci += 1
                syms, km = st.syms, st.km
                f, code, L = cpu.encode(model.c, model.cum, model.total, syms)
                assert f == 0 and L == 8 + sum(k + m for k, m in km)
                assert km == ring_sim.settle(model.c, model.cum, model.total, syms)
                tight = {w: ring_sim.tightness(km, align, head, schedule, w)
                         for w in ring_sim.NEEDS}
                rec = dict(model=mname, schedule=schedule, align=align, head=head,
                           symbols=syms, encoded_hex=code.hex(),
                           rare_at=[i for i, (k, m) in enumerate(km) if m],
                           tight_span=tight["span"], tight_rare=tight["rare"],
                           tight_head=tight["head"])
                if schedule in UNROLLED:
                    assert tight["span"] == 0
                    rec["tight_span_unrolled"] = ring_sim.tightness(km, align, head,
                                                                    UNROLLED[schedule], "span")
                assert rec.get("tight_span_unrolled", tight["span"]) >= 16, rec
                chunks.append(rec)
                covered[schedule] |= {(i - head) % ring_sim.DEC_CHECK_SPAN
                                      for i in rec["rare_at"] if i >= head}
                r = reached.setdefault(schedule, dict(span=0, rare=0, head=0))
                for w, v in tight.items():
                    r[w] = max(r[w], v)
                print(f"chunk {ci - 1}: {mname} {schedule} align {align} head {head}: "
                      f"{len(code)} B, {len(rec['rare_at'])} rare events, tightness {tight}",
                      flush=True)
    for schedule, offs in covered.items():
        assert offs == set(range(ring_sim.DEC_CHECK_SPAN)), (schedule, offs)
    assert {ch["align"] for ch in chunks} >= {0, 1, 31, 33, 63}
    out = dict(n=N, models={k: dict(total=m.total, c=m.c, cum=m.cum) for k, m in models.items()},
               reached=reached, chunks=chunks)
    with open(os.path.join(HERE, "ring_tight.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("reached:", reached)


if __name__ == "__main__":
    main()
