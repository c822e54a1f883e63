"""Generates tests/golden/plans.json (committed): the LDS plans of the set, order-1 and wide coders
as a GIVEN build of the library reports them, for tests/test_plan_table.py to hold later builds
to.  Run once, from the repo root, against the library the plans are to be pinned to (the parent
of the commit that reworks the plan code, built by tools/build_rev.sh):

    RC_LIB_PATH=variants/librc_amd_parent.so python tests/golden/make_plan_fixture.py

Host only (the plan hooks need no device).  The test never runs this script.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from range_coder_rust_amd import _native as N  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

# the plans depend on the total only through the bit length of total - 1: both sides of every
# power of two from 2^8 to 2^16, and a total that is not near one
TOTALS = [256, 257, 511, 512, 513, 2048, 2049, 4096, 4097, 32768, 32769, 40000, 65535, 65536]
SET_SIZES = list(range(1, 65))
WIDE_SIZES = [1, 2, 255, 256, 257, 1023, 1024, 2047, 2048, 4095, 4096]


def plan(hook, size, total):
    out = (ctypes.c_uint32 * 8)()
    assert getattr(N.load(), hook)(size, total, out) == N.RC_OK, (hook, size, total)
    return list(out)


def table(hook, sizes):
    return {str(size): [plan(hook, size, t) for t in TOTALS] for size in sizes}


def main():
    assert os.environ.get("RC_LIB_PATH"), "set RC_LIB_PATH to the library the plans are pinned to"
    doc = dict(words=["enc_lanes", "enc_lds", "enc_layout", "enc_tab", "dec_lanes", "dec_lds",
                      "dec_bits", "dec_shift"],
               totals=TOTALS,
               rc_model_set_plan_=table("rc_model_set_plan_", SET_SIZES),
               rc_model_order1_plan_=table("rc_model_order1_plan_", SET_SIZES),
               rc_model_wide_plan_=table("rc_model_wide_plan_", WIDE_SIZES))
    with open(os.path.join(HERE, "plans.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote plans.json from", N.LIB_PATH)


if __name__ == "__main__":
    main()
