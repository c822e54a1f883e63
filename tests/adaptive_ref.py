"""A plain-Python event reference of the adaptive order-0 model and its coder (test
infrastructure), written from oracle/rc_oracle.c: adapt_init, adapt_update, orc_param_update,
find_index, orc_encode_adaptive and orc_decode_adaptive.  Python integers masked to 64 bits.

Besides the bytes it reports the events that the GPU kernels (rc_adaptive.hip) treat on
separate branches, so that a test can prove which branch a given stream reaches:

* per symbol (k, m): k bytes settled by no_carry_expansion and m by range_reduction_expansion
  (range_coder.rs:110-116, :126-135), the convention of ring_sim.settle;
* the indices after which adapt_update halved the counts;
* the total before each symbol;
* on decode, the indices where find_index saw x / r >= total, which it answers with the last
  symbol (the kernels' clamp of the exact target to total - 1).  Only a stream that no encoder
  wrote gets there.

It imports nothing from the package under test.
"""
from bisect import bisect_right
from itertools import accumulate

M64 = (1 << 64) - 1
TOP8 = 1 << 56
TOP16 = 1 << 48

F_BAD_SYMBOL = 2
F_CAPACITY = 4
F_TRUNCATED = 8


class Model:
    """adapt_model: counts c (all 1 at first) and their total; cum is derived on demand."""

    def __init__(self, n, inc, limit, period):
        self.n, self.inc, self.limit, self.period = n, inc, limit, period
        self.c = [1] * n
        self.total = n

    def clone(self):
        m = Model.__new__(Model)
        m.n, m.inc, m.limit, m.period = self.n, self.inc, self.limit, self.period
        m.c, m.total = list(self.c), self.total
        return m

    def cum(self):
        """cum[0 .. n]: cum[s] = c[0] + ... + c[s - 1], cum[n] = total."""
        return list(accumulate(self.c, initial=0))

    def update(self, s, i):
        """adapt_update after symbol number i of the chunk; returns whether it halved."""
        self.c[s] += self.inc
        self.total += self.inc
        if (i + 1) % self.period == 0 and self.total > self.limit:
            self.c = [(v + 1) >> 1 for v in self.c]
            self.total = sum(self.c)
            return True
        return False


def param_update(low, rng, c, cum, total):
    """orc_param_update: (low, range, settled bytes, k, m)."""
    r = rng // total
    rng = r * c
    low = (low + r * cum) & M64
    out = bytearray()
    k = 0
    while (low ^ ((low + rng) & M64)) < TOP8:
        out.append(low >> 56)
        low, rng, k = (low << 8) & M64, (rng << 8) & M64, k + 1
    m = 0
    while rng < TOP16:
        rng = ~low & (TOP16 - 1)
        out.append(low >> 56)
        low, rng, m = (low << 8) & M64, (rng << 8) & M64, m + 1
    return low, rng, bytes(out), k, m


class Encoded:
    """The result of encode(): flag, code (the whole stream), out_len, km [(k, m)] per coded
    symbol, halve_at (indices after which a halving ran), totals (the total before each)."""

    def __init__(self):
        self.flag, self.code, self.out_len = 0, b"", 0
        self.km, self.halve_at, self.totals = [], [], []

    @property
    def rare_at(self):
        return [i for i, (_, m) in enumerate(self.km) if m]


def encode(n, inc, limit, period, syms, cap=None):
    """orc_encode_adaptive over one chunk.  code holds every byte (not cut at cap); flag and
    out_len are the oracle's for a slot of cap bytes (None: large enough)."""
    md = Model(n, inc, limit, period)
    low, rng = 0, M64
    e = Encoded()
    code = bytearray()
    for i, s in enumerate(syms):
        s = int(s)
        if s >= n:
            e.flag, e.code, e.out_len = F_BAD_SYMBOL, bytes(code), len(code)
            return e
        e.totals.append(md.total)
        low, rng, b, k, m = param_update(low, rng, md.c[s], sum(md.c[:s]), md.total)
        code += b
        e.km.append((k, m))
        if md.update(s, i):
            e.halve_at.append(i)
    code += low.to_bytes(8, "big")  # Encoder::finish: 8 x left_shift
    e.code, e.out_len = bytes(code), len(code)
    e.flag = F_CAPACITY if cap is not None and len(code) > cap else 0
    return e


def decode(n, inc, limit, period, code, count):
    """orc_decode_adaptive: (flag, symbols decoded before the flag was raised, clamp_at), with
    clamp_at the indices whose find_index saw x / r >= total."""
    code = bytes(code)
    if len(code) < 8:
        return F_TRUNCATED, [], []
    md = Model(n, inc, limit, period)
    low, rng = 0, M64
    data, pos = int.from_bytes(code[:8], "big"), 8
    syms, clamp_at = [], []
    for i in range(count):
        cum = md.cum()
        rfreq = ((data - low) & M64) // (rng // md.total)
        if rfreq >= md.total:
            clamp_at.append(i)
        s = min(bisect_right(cum, rfreq) - 1, n - 1)  # find_index: cum[s] <= rfreq < cum[s + 1]
        low, rng, b, _, _ = param_update(low, rng, md.c[s], cum[s], md.total)
        if pos + len(b) > len(code):
            return F_TRUNCATED, syms, clamp_at
        for _ in b:
            data = ((data << 8) | code[pos]) & M64
            pos += 1
        syms.append(s)
        md.update(s, i)
    return 0, syms, clamp_at
