"""The static decoder's code ring on the GPU: the directed ring fixtures
(tests/golden/ring_fixtures.json, made by tests/golden/make_ring_fixtures.py) put a
range_reduction_expansion at every offset of the 8-symbol ring-check span, each followed by the
symbols that settle the most bytes, with the code streams at the alignments the fixtures were
steered for (the decoder's 64-B load bursts start on 64-B boundaries).  Every decoder variant of
the model (pair buckets at both workgroup sizes, and the bucket decoder) must return the
fixture's symbols with no flag, also with the output misaligned (a head of single symbols).

The older fixtures leave the ring far from its limit when their heavy spans come (DESIGN.md
§5.2), so the tight streams (tests/golden/ring_tight.json, made by
tests/golden/make_ring_tight.py) run through the same variants too: each is steered so that a
ring check finds just 16 bytes staged before 8 symbols that settle 17, and a decoder whose span
check staged 16 bytes instead of 24 would decode it wrong.

Run against a scratch `-DRC_RING_GUARD` library (RC_LIB_PATH, tools/ring_guard.py), the same
assertions show that no symbol read a code byte its ring had not staged: the guard flag would
make the chunk's flags non-zero."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import ring_check_exact, ring_decode_at  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


@pytest.fixture(scope="module")
def ring_fx():
    with open(os.path.join(HERE, "golden", "ring_fixtures.json")) as f:
        return json.load(f)


def _decode_at(m, chunks, head, reps=1):
    """Code stream k at its fixture alignment mod 64 inside 64-B slots; decoded output at
    `head` bytes past a 64-B boundary (plus 64-B aligned chunk strides)."""
    return ring_decode_at(lambda *a: rc.decode_batch(m, *a), list(chunks) * reps, head)


@pytest.mark.parametrize("pair", ["512", "1024", "0"])
@pytest.mark.parametrize("head", [0, 5, 48])
def test_ring_fixtures_decode(ctx, ring_fx, knob_ctx, pair, head):
    c = np.array(ring_fx["c"], np.uint32)
    cum = np.array(ring_fx["cum"], np.uint32)
    chunks = ring_fx["chunks"]
    m = rc.StaticModel(c, cum, ring_fx["total"], ctx=knob_ctx(RC_DEC_PAIR=pair))
    s, sym_off, flags = _decode_at(m, chunks, head)
    assert (flags == 0).all(), flags
    assert (s[:head] == 0xEE).all() and (s[sym_off[-1]:] == 0xEE).all()
    for k, ch in enumerate(chunks):
        got = s[sym_off[k]:sym_off[k + 1]]
        assert (got == np.array(ch["symbols"], np.uint8)).all(), (pair, head, k)


def test_ring_fixtures_full_waves(ctx, ring_fx, knob_ctx):
    """Every fixture in many lanes at once (whole workgroups of the bucket decoder, LUT 4: the
    fixtures' model, total 2^16, has 2^12 buckets and so runs 512-lane workgroups, the variant
    2^20-chunk launches of this model take), against the oracle's decode."""
    c = np.array(ring_fx["c"], np.uint32)
    cum = np.array(ring_fx["cum"], np.uint32)
    total = ring_fx["total"]
    chunks = ring_fx["chunks"]
    m = rc.StaticModel(c, cum, total, ctx=knob_ctx(RC_DEC_PAIR="0"))
    s, sym_off, flags = _decode_at(m, chunks, 0, reps=64)
    assert (flags == 0).all()
    for k in range(len(flags)):
        ch = chunks[k % len(chunks)]
        f, d = cpu.decode(c, cum, total, bytes.fromhex(ch["encoded_hex"]), len(ch["symbols"]))
        assert f == 0
        assert (s[sym_off[k]:sym_off[k + 1]] == d).all(), k


@pytest.fixture(scope="module")
def tight_fx():
    with open(os.path.join(HERE, "golden", "ring_tight.json")) as f:
        return json.load(f)


def _tight_model(tight_fx, name, ctx):
    md = tight_fx["models"][name]
    m = rc.StaticModel(np.array(md["c"], np.uint32), np.array(md["cum"], np.uint32), md["total"],
                       ctx=ctx)
    return m, [ch for ch in tight_fx["chunks"] if ch["model"] == name]


# pair buckets at both workgroup sizes, the default dispatch, the direct q-to-symbol table and
# the buckets (test_gpu_direct_table.py's variants)
TIGHT_VARIANTS = ["512", "1024", "0", "6", "4"]


@pytest.mark.parametrize("pair", TIGHT_VARIANTS)
@pytest.mark.parametrize("name", ["pow2", "magic"])
def test_tight_streams_decode(ctx, tight_fx, knob_ctx, name, pair):
    """Every tight stream of the model at every head some stream of it was steered for (a wide
    stream's head of h 2-byte symbols is the same schedule as a head of h bytes here), so each
    at its own head, and at two more (16, 48)."""
    m, chunks = _tight_model(tight_fx, name, knob_ctx(RC_DEC_PAIR=pair))
    for head in sorted({ch["head"] for ch in chunks} | {16, 48}):
        s, sym_off, flags = ring_decode_at(lambda *a: rc.decode_batch(m, *a), chunks,
                                           (64 - head) % 64)
        ring_check_exact(s, sym_off, flags, chunks)


@pytest.mark.parametrize("pair", ["0", "6"])
@pytest.mark.parametrize("name", ["pow2", "magic"])
def test_tight_streams_full_launch(ctx, tight_fx, knob_ctx, name, pair):
    """The tight streams interleaved and repeated to 1,280 chunks in one launch: more than one
    workgroup at either size (512 lanes for the buckets, 1,024 for the q-to-symbol table), the
    last one partly dead, and every wave mixing streams at different points of their schedules."""
    m, chunks = _tight_model(tight_fx, name, knob_ctx(RC_DEC_PAIR=pair))
    many = (chunks * (1280 // len(chunks) + 1))[:1280]
    for head in (0, 5):
        s, sym_off, flags = ring_decode_at(lambda *a: rc.decode_batch(m, *a), many,
                                           (64 - head) % 64)
        ring_check_exact(s, sym_off, flags, many)
