"""The tight ring streams on the host (tests/golden/ring_tight.json, made by
tests/golden/make_ring_tight.py): each is steered for one (schedule, align, head) of
tests/ring_sim.py so that a decoder with a lowered ring need would read unstaged bytes on it.
Checked here, all recomputed from the symbols: the streams are the oracle's; the conditions the
generator works to (tightness, heads, alignments, rare events at every span offset, a sound
shipped schedule wherever the GPU tests place a stream); the recorded tightness; that the family
references (a set of K identical rows under any index stream or context map, the table as a wide
model) give the static bytes, which is what lets one fixture serve all four decoders; and, for
the record, how blunt the older ring fixtures are by the same measure."""
import json
import os

import numpy as np
import pytest

from oracle import cpu
import indexed_ref
import order1_ref
import periodic_ref
import ring_sim
import wide_ref

HERE = os.path.dirname(os.path.abspath(__file__))
UNROLLED = {"indexed_rolled": "indexed"}


@pytest.fixture(scope="module")
def tight_fx():
    with open(os.path.join(HERE, "golden", "ring_tight.json")) as f:
        fx = json.load(f)
    for ch in fx["chunks"]:
        md = fx["models"][ch["model"]]
        ch["km"] = ring_sim.settle(md["c"], md["cum"], md["total"], ch["symbols"])
    return fx


def test_tight_streams_match_oracle(tight_fx):
    assert sorted(tight_fx["models"]) == ["magic", "pow2"]
    for name, total in (("pow2", 65536), ("magic", 65535)):
        md = tight_fx["models"][name]
        assert md["total"] == total and md["c"] == [total - 255] + [1] * 255
        assert md["cum"] == [0] + list(np.cumsum(md["c"])[:-1])
    for k, ch in enumerate(tight_fx["chunks"]):
        md = tight_fx["models"][ch["model"]]
        c, cum, total = md["c"], md["cum"], md["total"]
        assert len(ch["symbols"]) == tight_fx["n"] == 256
        f, code, _ = cpu.encode(c, cum, total, ch["symbols"])
        assert f == 0 and code.hex() == ch["encoded_hex"], k
        f, d = cpu.decode(c, cum, total, code, len(ch["symbols"]))
        assert f == 0 and list(d) == ch["symbols"], k
        assert 8 + sum(a + b for a, b in ch["km"]) == len(code)
        assert [i for i, (_, m) in enumerate(ch["km"]) if m] == ch["rare_at"]


def test_tight_streams_are_tight(tight_fx):
    """Every stream under-runs with the span need at 16 (of 24): an 8-symbol span settles at
    most 17 no-carry bytes before a range_reduction_expansion stages its own, so a check that
    finds 16 staged is the tightest that can fail, and 17 is out of reach.  The rolled path
    checks 12 bytes after every 4 symbols, which settle at most 9: there the span need cannot
    bind at all (tightness 0), so its streams are span-tight under the same kernel's unrolled
    schedule, which they also run through, and bind the need of 12 instead (at most 8)."""
    for k, ch in enumerate(tight_fx["chunks"]):
        sch = ch["schedule"]
        span = ring_sim.tightness(ch["km"], ch["align"], ch["head"], UNROLLED.get(sch, sch))
        assert 16 <= span <= 17, (k, span)
        if sch in UNROLLED:
            assert ring_sim.tightness(ch["km"], ch["align"], ch["head"], sch) == 0
    rolled = [ch for ch in tight_fx["chunks"] if ch["schedule"] == "indexed_rolled"]
    assert max(ch["tight_head"] for ch in rolled) == 8


def test_tight_streams_cover_heads_aligns_and_span_offsets(tight_fx):
    chunks = tight_fx["chunks"]
    assert {ch["schedule"] for ch in chunks} == set(ring_sim.SCHEDULES)
    assert {ch["align"] for ch in chunks} >= {0, 1, 31, 33, 63}
    for sch, (_, top) in ring_sim.SCHEDULES.items():
        mine = [ch for ch in chunks if ch["schedule"] == sch]
        heads = {ch["head"] for ch in mine}
        assert {0, top} <= heads and any(h % 2 and h < 8 for h in heads), (sch, heads)
        assert {ch["model"] for ch in mine} == {"pow2", "magic"}
        offs = {(i - ch["head"]) % ring_sim.DEC_CHECK_SPAN for ch in mine for i in ch["rare_at"]
                if i >= ch["head"]}
        assert offs == set(range(ring_sim.DEC_CHECK_SPAN)), (sch, offs)


def test_shipped_schedule_is_sound_wherever_the_gpu_tests_place_a_stream(tight_fx):
    """No under-run and no over-write under the shipped needs: every stream, in every decoder's
    schedule, at its fixture alignment and at every head the GPU tests give it (the heads the
    streams were steered for, and 16 and 48)."""
    heads = sorted({ch["head"] for ch in tight_fx["chunks"]} | {16, 48})
    for k, ch in enumerate(tight_fx["chunks"]):
        for sch, (_, top) in ring_sim.SCHEDULES.items():
            for head in heads:
                if head <= top:
                    under, over = ring_sim.replay(ch["km"], ch["align"], head, schedule=sch)
                    assert not under and not over, (k, sch, head, under, over)


def test_recorded_tightness_is_reproduced(tight_fx):
    reached = {}
    for k, ch in enumerate(tight_fx["chunks"]):
        sch = ch["schedule"]
        for which in ring_sim.NEEDS:
            t = ring_sim.tightness(ch["km"], ch["align"], ch["head"], sch, which)
            assert t == ch["tight_" + which], (k, which, t)
            r = reached.setdefault(sch, dict(span=0, rare=0, head=0))
            r[which] = max(r[which], t)
            if t:  # the definition: under-runs at t, and at no need between t and the shipped one
                arg, shipped = ring_sim.NEEDS[which]
                for v in range(t, shipped + 1):
                    under, _ = ring_sim.replay(ch["km"], ch["align"], ch["head"], schedule=sch,
                                               **{arg: v})
                    assert bool(under) == (v == t), (k, which, v)
        if sch in UNROLLED:
            assert ch["tight_span_unrolled"] == ring_sim.tightness(
                ch["km"], ch["align"], ch["head"], UNROLLED[sch])
    assert reached == tight_fx["reached"]


def test_schedule_aliases_and_arguments():
    """The family schedules that are position for position the static one are aliases of it,
    not copies; a wide head is counted in 2-byte symbols, so at most 31."""
    static = ring_sim.SCHEDULES["static"][0]
    assert all(ring_sim.SCHEDULES[s][0] == static for s in ("indexed", "order1", "wide"))
    assert ring_sim.SCHEDULES["indexed_rolled"][0] != static
    km = [(2, 0)] * 64
    with pytest.raises(ValueError):
        ring_sim.replay(km, 0, 32, schedule="wide")
    with pytest.raises(ValueError):
        ring_sim.replay(km, 0, 0, schedule="adaptive")
    assert ring_sim.replay(km, 0, 31, schedule="wide") == ring_sim.replay(km, 0, 31)


def test_family_references_give_the_static_bytes(tight_fx):
    rng = np.random.default_rng(5)
    for k, ch in enumerate(tight_fx["chunks"]):
        md = tight_fx["models"][ch["model"]]
        total = md["total"]
        syms = np.array(ch["symbols"], np.uint8)
        code = bytes.fromhex(ch["encoded_hex"])
        K = (1, 8, 64)[k % 3]
        c, cum = indexed_ref.tables([md["c"]] * K)
        idx = rng.integers(0, K, len(syms))
        assert indexed_ref.encode_ref(c, cum, total, syms, idx) == (0, code), k
        f, d = indexed_ref.decode_ref(c, cum, total, code, idx)
        assert f == 0 and (d == syms).all(), k
        cm = rng.integers(0, K, 256)
        first = int(rng.integers(0, K))
        assert order1_ref.encode_ref(c, cum, total, cm, first, syms) == (0, code), k
        f, d = order1_ref.decode_ref(c, cum, total, cm, first, code, len(syms))
        assert f == 0 and (d == syms).all(), k
        P = (2, 8)[k % 2]
        cmp_ = rng.integers(0, K, (P, 256))
        assert periodic_ref.encode_ref(c, cum, total, cmp_, first, syms) == (0, code), k
        f, d = periodic_ref.decode_ref(c, cum, total, cmp_, first, code, len(syms))
        assert f == 0 and (d == syms).all(), k
        wc, wcum, wtotal = wide_ref.table(md["c"])
        assert wtotal == total
        assert wide_ref.encode_ref(wc, wcum, total, syms) == (0, code), k
        f, d = wide_ref.decode_ref(wc, wcum, total, code, len(syms))
        assert f == 0 and (d == syms).all(), k


def test_older_ring_fixtures_are_blunt():
    """For the record: by the same measure the directed fixtures of make_ring_fixtures.py have
    tightness 0 for the span need and for the rare path's need at the head they were steered
    for (0): no lowered ring need makes any of them under-run there.  At the other two heads
    test_gpu_ring.py gives them (59 and 16: outputs 5 and 48 bytes past a 64-B boundary) the
    check between head and body happens to find some of them lower: span tightness 15 and 12
    at the most, so a span need of 16 still passes all of them; the rare path's need never
    binds.  They show that a range_reduction_expansion at any span offset decodes right, not
    that the ring needs are large enough.  A re-steered set would show here."""
    with open(os.path.join(HERE, "golden", "ring_fixtures.json")) as f:
        fx = json.load(f)
    worst = {0: 0, 59: 0, 16: 0}
    for k, ch in enumerate(fx["chunks"]):
        km = ring_sim.settle(fx["c"], fx["cum"], fx["total"], ch["symbols"])
        for head in worst:
            worst[head] = max(worst[head],
                              ring_sim.tightness(km, ch["align"], head, "static", "span"))
            assert ring_sim.tightness(km, ch["align"], head, "static", "rare") == 0, (k, head)
    assert worst == {0: 0, 59: 15, 16: 12}
