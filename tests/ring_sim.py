"""A host model of the static decoder's code-ring schedule (test infrastructure).

k_decode_static (range_coder_rust_amd/csrc/rc_decode.inc) stages each lane's code stream
through a 64-B LDS ring: 64-B load bursts, committed 32 B at a time at phase boundaries and on
demand (dec_sync), with ring checks every DEC_CHECK_SPAN symbols.  This module replays that
schedule (positions only, no data) for one chunk, given each symbol's settled bytes split into
no_carry_expansion bytes k and range_reduction_expansion bytes m (range_coder.rs:83-89), and
reports the two ways the ring can go wrong:

* under-run: a symbol reads a code byte at or past the staged end (fillb).  The ring slot then
  holds bytes from 64 B earlier: wrong symbols, no flag;
* over-write: a commit overwrites bytes not yet consumed.

The family decoders (k_decode_indexed, k_decode_order1, k_decode_wide) stage their code the same
way; `schedule` picks one of them (SCHEDULES), and `tightness` measures how sharply a stream tests
one of the ring needs.  The indexed decoder's unrolled path, the order-1 decoder and the wide
decoder (its head in 2-byte symbols, 0..31) run the static schedule position for position and
are aliases of it; only the indexed decoder's rolled path ("indexed_rolled") is a schedule of
its own.

The constants mirror rc_static.h / rc_decode.inc for small (SM) models; `need_rare` is the
rare path's DEC_NEED_SM (12 before round 4, 3 * DEC_CHECK_SPAN = 24 after) and `need_span` the
in-phase checks' DEC_NEED_SPAN (24; scratch guard builds lower it to provoke under-runs).  `Replay` steps
one symbol at a time (so a search can steer a stream against it); `replay` runs a whole chunk.
"""
import copy

DEC_RING = 16        # dwords
DEC_PF = 2           # 16-B blocks per commit
DEC_LD = 4           # 16-B blocks per load burst
DEC_CHECK_SPAN = 8
NEED_HEAD = 12       # head and tail: a check after every symbol for the next 4
NEED_SPAN = 3 * DEC_CHECK_SPAN

# The decoders' schedules, each read off its kernel: (the schedule replayed, the largest head).
# Every decoder primes its ring, decodes its head and tail and crosses a phase boundary with the
# same statements as k_decode_static (rc_decode.inc:759-786, :796-799, :813-823), and all share
# dec_apply, dec_rare and dec_check4; what could differ is where a 16-symbol phase checks.
#
# * "static": k_decode_static; dec_phase16 (rc_decode.inc:633-646) checks the span need after
#   symbol 8 of a phase, and the caller after dec_phase (:796-799, :813-818).
# * "indexed": k_decode_indexed with every index < K.  The prologue and head are
#   rc_indexed.hip:430-455, a phase is RC_SET_PHASE (:465-471): set_phase16's unrolled path
#   (:357-366) checks after symbol 8, then dec_phase and the span check; the tail is :488-491.
#   Position for position the static schedule: an alias.
# * "indexed_rolled": the same kernel when some lane of the wave holds an index >= K among the
#   16 of the phase (rc_indexed.hip:331-356): every lane then checks DEC_NEED_HEAD after every 4
#   symbols (:345), the span need at the phase's end (:354), and RC_SET_PHASE goes on as above.
# * "order1": k_decode_order1, period 1 and periodic (one source).  Prologue and head
#   rc_order1.hip:408-434, a phase RC_O1_PHASE (:441-445) over o1_phase16 (:332-344, a check
#   after symbol 8), the tail :462-465.  The static schedule: an alias.
# * "wide": k_decode_wide.  Prologue and head rc_wide.hip:334-357; a phase is RC_WIDE_PHASE
#   (:361-367): wide_block8 (:264-274, no check inside at DEC_CHECK_SPAN 8), the span check,
#   wide_block8, dec_phase, the span check; the tail :385-388.  The static schedule with the
#   head counted in 2-byte symbols, so at most 31: an alias with that cap.
SCHEDULES = {"static": ("static", 63), "indexed": ("static", 63),
             "indexed_rolled": ("indexed_rolled", 63), "order1": ("static", 63),
             "wide": ("static", 31)}


class Replay:
    """The ring schedule of one chunk of n symbols whose code starts at `align` mod 64 and whose
    output needs `head` single symbols before it is 64-B aligned (rc_decode.inc:575-637)."""

    def __init__(self, n, align=0, head=0, need_rare=NEED_SPAN, need_span=NEED_SPAN,
                 schedule="static", need_head=NEED_HEAD):
        if schedule not in SCHEDULES:
            raise ValueError(f"schedule must be one of {sorted(SCHEDULES)}")
        if head > SCHEDULES[schedule][1]:
            raise ValueError(f"head {head} cannot occur in schedule {schedule!r}")
        self.rolled = SCHEDULES[schedule][0] == "indexed_rolled"
        self.need_head = need_head
        self.n = n
        self.need_span = need_span
        self.head = min(head, n)
        self.nph = (n - self.head) >> 4      # 16-symbol phases after the head
        self.need_rare = need_rare
        self.fillb = 0
        self.pend_ok = 0
        self.bpos = 8 * (align + 8)          # Decoder::new primes 8 bytes
        self.under = []   # symbol indices that read unstaged bytes
        self.over = []    # symbols after which a commit overwrote unread bytes
        self.i = 0        # symbols decoded so far
        self.min_slack = 1 << 30  # fewest staged-but-unread bytes left after a symbol's reads
        for _ in range(DEC_RING // (4 * DEC_PF)):
            if not self.pend_ok:
                self._issue()
            self._commit()
        while self.fillb - self.bpos < 8 * need_head:
            if not self.pend_ok:
                self._issue()
            self._commit()
        if not self.pend_ok:
            self._issue()
        self._check(need_head)
        if self.head == 0:
            self._check(need_span)

    def clone(self):
        return copy.deepcopy(self)

    def unread(self):
        """Staged bytes not yet consumed."""
        return (self.fillb - self.bpos) // 8

    def span_offset(self):
        """The next symbol's offset in its ring-check span (None in the head and tail, where
        every symbol is followed by a check)."""
        j = self.i - self.head
        if j < 0 or j >= 16 * self.nph:
            return None
        return j % DEC_CHECK_SPAN

    def _issue(self):
        self.pend_ok = DEC_LD // DEC_PF

    def _commit(self):
        if self.fillb - self.bpos > 32 * DEC_RING - 128 * DEC_PF:
            self.over.append(self.i - 1)
        self.fillb += 128 * DEC_PF
        self.pend_ok -= 1

    def _sync(self, need):
        while self.fillb - self.bpos < 8 * need:
            if not self.pend_ok:
                self._issue()
            self._commit()

    def _check(self, need):
        if self.fillb - self.bpos < 8 * need:
            self._sync(need)

    def _phase(self):
        if self.pend_ok and self.fillb - self.bpos <= 32 * DEC_RING - 128 * DEC_PF:
            self._commit()
        if not self.pend_ok:
            self._issue()

    def step(self, k, m):
        """One symbol that settles k no-carry bytes and m range-reduction bytes, then the
        checks the kernel runs after it."""
        i = self.i
        if self.bpos + 8 * k > self.fillb:
            self.under.append(i)
        self.bpos += 8 * k
        if m:
            self._sync(m + self.need_rare)
            for _ in range(m):
                if self.bpos + 8 > self.fillb:
                    self.under.append(i)
                self.bpos += 8
        self.min_slack = min(self.min_slack, (self.fillb - self.bpos) // 8)
        self.i = i + 1
        j = self.i - self.head     # symbols of the body decoded so far
        if i < self.head:
            self._check(self.need_head)
            if self.i == self.head:
                self._check(self.need_span)
        elif j <= 16 * self.nph:
            if self.rolled:  # rc_indexed.hip:336-355: a check after every 4, the span need last
                if j % 4 == 0:
                    self._check(self.need_head)
                if j % 16 == 0:
                    self._check(self.need_span)
                    self._phase()
                    self._check(self.need_span)
            elif j % 16 == 0:
                self._phase()
                self._check(self.need_span)
            elif j % DEC_CHECK_SPAN == 0:
                self._check(self.need_span)
        else:
            self._check(self.need_head)


def replay(km, align=0, head=0, need_rare=NEED_SPAN, need_span=NEED_SPAN, schedule="static",
           need_head=NEED_HEAD):
    """Replay the decoder's ring schedule over one chunk.  km: [(k, m)] per symbol; align: the
    code stream's address mod 64; head: symbols decoded singly before the output is 64-B
    aligned; schedule: which decoder's (SCHEDULES).  Returns (under-run symbol indices,
    over-write symbol indices)."""
    g = Replay(len(km), align, head, need_rare, need_span, schedule, need_head)
    for k, m in km:
        g.step(k, m)
    return g.under, g.over


# `which` of tightness(): the need that is lowered, as replay()'s argument and its shipped value
NEEDS = {"span": ("need_span", NEED_SPAN), "rare": ("need_rare", NEED_SPAN),
         "head": ("need_head", NEED_HEAD)}


def tightness(km, align, head, schedule="static", which="span"):
    """How sharply a stream tests one ring need: the largest value below the shipped one of the
    need `which` ("span": DEC_NEED_SPAN; "rare": DEC_NEED_SM; "head": the need of 12 of the
    per-symbol head and tail checks and of the rolled path's checks) at which the replay
    under-runs, the other needs at their shipped values; 0 if no value under-runs.  A decoder
    whose need were cut to that value or below would read stale ring bytes on this stream; one
    cut less far would still pass it."""
    arg, shipped = NEEDS[which]
    for v in range(shipped - 1, -1, -1):
        if replay(km, align, head, schedule=schedule, **{arg: v})[0]:
            return v
    return 0


M64 = (1 << 64) - 1


def settle(c, cum, total, syms):
    """[(k, m)] per symbol of an encoder run: the bytes no_carry_expansion (range_coder.rs:110-116)
    and range_reduction_expansion (:126-135) settle in param_update (:53-92), from a u64
    restatement of the coder (the decoder's state follows the encoder's exactly)."""
    low, rng = 0, M64
    out = []
    for s in syms:
        r = rng // total
        rng = r * int(c[s])
        low = low + r * int(cum[s])
        k = 0
        while (low ^ (low + rng)) < 1 << 56:
            low, rng, k = (low << 8) & M64, (rng << 8) & M64, k + 1
        m = 0
        while rng < 1 << 48:
            rng = (~low & M64) & ((1 << 48) - 1)
            low, rng, m = (low << 8) & M64, (rng << 8) & M64, m + 1
        out.append((k, m))
    return out
