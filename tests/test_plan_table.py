"""The LDS plans of the set, order-1 and wide coders against tests/golden/plans.json: the 8 words of
rc_model_set_plan_ and rc_model_order1_plan_ for every K in 1 .. 64 and of rc_model_wide_plan_ at
the alphabet sizes around its table thresholds, at totals on both sides of every bit length.  The
fixture was recorded from the library as it was BEFORE the three plans came to share one decoder
rule (tests/golden/make_plan_fixture.py), so this pins that rule against the code it replaced, not
against itself.  Host only."""
import ctypes
import json
import os

import pytest

from range_coder_rust_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans.json")
with open(GOLDEN) as _f:
    PLANS = json.load(_f)


def test_fixture_covers_what_it_should():
    assert PLANS["totals"] == [256, 257, 511, 512, 513, 2048, 2049, 4096, 4097, 32768, 32769,
                               40000, 65535, 65536]
    for hook in ("rc_model_set_plan_", "rc_model_order1_plan_"):
        assert sorted(map(int, PLANS[hook])) == list(range(1, 65))
    assert sorted(map(int, PLANS["rc_model_wide_plan_"])) == [1, 2, 255, 256, 257, 1023, 1024,
                                                              2047, 2048, 4095, 4096]
    for hook in ("rc_model_set_plan_", "rc_model_order1_plan_", "rc_model_wide_plan_"):
        for rows in PLANS[hook].values():
            assert len(rows) == len(PLANS["totals"]) and all(len(r) == 8 for r in rows)


@pytest.mark.parametrize("hook", ["rc_model_set_plan_", "rc_model_order1_plan_",
                                  "rc_model_wide_plan_"])
def test_plans_are_the_recorded_ones(hook):
    fn = getattr(N.load(), hook)
    out = (ctypes.c_uint32 * 8)()
    for size, rows in PLANS[hook].items():
        for total, want in zip(PLANS["totals"], rows):
            assert fn(int(size), total, out) == N.RC_OK, (hook, size, total)
            assert list(out) == want, (hook, size, total, dict(zip(PLANS["words"], out)))
