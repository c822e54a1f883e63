"""The code rings of the family decoders on the GPU: k_decode_indexed, k_decode_order1 (period 1
and periodic) and k_decode_wide stage their code like k_decode_static, each with its own head,
phase, burst and tail loops (tests/ring_sim.py SCHEDULES reads them off the kernels).  The tight
streams (tests/golden/ring_tight.json, made by tests/golden/make_ring_tight.py) are coded with one
table, so a set of K identical rows, whatever the index stream or the context maps, and the table
as a wide model all decode the static bytes (tests/test_ring_tight.py shows it on the references):
one fixture serves all four decoders.  Every stream must come back byte-exact with no flag and
the sentinels around the outputs intact, at the head it was steered for and at the others.

The indexed decoder has a second schedule: when a lane of the wave holds an index >= K among the
16 of a phase, every lane takes set_phase16's rolled path for that phase (a check of 12 bytes
after every 4 symbols).  A chunk whose indexes are all >= K puts its whole wave on that path for
every phase (the outputs share one head, so the lanes' phases coincide), which is the schedule
the "indexed_rolled" streams are steered for; one whose first index alone is >= K does so for
one phase.  The sound chunks beside it must stay exact.

Run against a scratch -DRC_RING_GUARD library (tools/ring_guard.py probe_tight), these decodes
show where a lowered ring need makes a symbol read bytes its ring has not staged."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
import indexed_ref  # noqa: E402
from gpu_helpers import dev, ring_check_exact, ring_decode_at  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ["pow2", "magic"]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


@pytest.fixture(scope="module")
def tight_fx():
    with open(os.path.join(HERE, "golden", "ring_tight.json")) as f:
        return json.load(f)


def table(tight_fx, name):
    md = tight_fx["models"][name]
    chunks = [ch for ch in tight_fx["chunks"] if ch["model"] == name]
    return np.array(md["c"], np.uint32), np.array(md["cum"], np.uint32), md["total"], chunks


def heads_of(chunks, top=63):
    """Every head some stream was steered for, and two more."""
    return sorted({ch["head"] for ch in chunks if ch["head"] <= top} | {16, top - 15})


def full_launch(chunks):
    """The streams interleaved and repeated to 1,280 chunks: more than one 1,024-lane workgroup,
    the last one partly dead, every wave mixing streams at different points of their schedules."""
    return (chunks * (1280 // len(chunks) + 1))[:1280]


# ---- indexed ---------------------------------------------------------------------------------
def indexed_call(mset, idx):
    return lambda code, coff, clen, syms, sym_off: rc.decode_batch_indexed(
        mset, code, coff, clen, dev(idx), syms, sym_off)


def run_indexed(mset, K, chunks, head, rng, poison=None):
    """Random indexes < K; poison: None, or "all" / "first": in every 64 lanes one chunk whose
    indexes (all of them, or the first alone) are K.  Returns the poisoned chunks."""
    n = len(chunks[0]["symbols"])
    off = (64 - head) % 64
    idx = rng.integers(0, K, off + n * len(chunks) + 64).astype(np.uint8)
    bad = list(range(7, len(chunks), 64)) if poison else []
    for k in bad:
        at = off + n * k
        idx[at:at + (n if poison == "all" else 1)] = K
    s, sym_off, flags = ring_decode_at(indexed_call(mset, idx), chunks, off)
    ring_check_exact(s, sym_off, flags, chunks, skip=bad)
    return bad, flags, idx, sym_off


@pytest.mark.parametrize("K", [1, 64])
@pytest.mark.parametrize("name", MODELS)
def test_indexed_tight_streams(ctx, tight_fx, name, K):
    c, cum, total, chunks = table(tight_fx, name)
    mset = rc.StaticModelSet(np.tile(c, (K, 1)), np.tile(cum, (K, 1)), total)
    rng = np.random.default_rng(K)
    for head in heads_of(chunks):
        run_indexed(mset, K, chunks, head, rng)


@pytest.mark.parametrize("poison", ["all", "first"])
@pytest.mark.parametrize("K", [1, 64])
@pytest.mark.parametrize("name", MODELS)
def test_indexed_rolled_path_beside_a_flagged_chunk(ctx, tight_fx, name, K, poison):
    """The same batch with one chunk of bad indexes: its neighbours take the rolled path (for
    every phase, or for the phase of the bad index) and stay exact; its own flag and output
    are indexed_ref's (BAD_MODEL at its first symbol, so nothing of its output is specified)."""
    c, cum, total, chunks = table(tight_fx, name)
    cs, cums = np.tile(c, (K, 1)), np.tile(cum, (K, 1))
    mset = rc.StaticModelSet(cs, cums, total)
    rng = np.random.default_rng(100 + K)
    for head in heads_of(chunks):
        bad, flags, idx, sym_off = run_indexed(mset, K, chunks, head, rng, poison)
        assert bad
        for k in bad:
            f, out = indexed_ref.decode_ref(cs, cums, total,
                                            bytes.fromhex(chunks[k]["encoded_hex"]),
                                            idx[sym_off[k]:sym_off[k + 1]])
            assert f == indexed_ref.F_BAD_MODEL and len(out) == 0
            assert flags[k] == f, (head, k, flags[k])


@pytest.mark.parametrize("poison", [None, "all"])
@pytest.mark.parametrize("name", MODELS)
def test_indexed_full_launch(ctx, tight_fx, name, poison):
    c, cum, total, chunks = table(tight_fx, name)
    mset = rc.StaticModelSet(np.tile(c, (8, 1)), np.tile(cum, (8, 1)), total)
    rng = np.random.default_rng(8)
    many = full_launch(chunks)
    for head in (0, 5):
        bad, flags, _, _ = run_indexed(mset, 8, many, head, rng, poison)
        assert (flags[bad] == indexed_ref.F_BAD_MODEL).all()


# ---- order-1 ---------------------------------------------------------------------------------
def order1_set(c, cum, total, K, P, rng):
    """K identical rows, one random context map per phase, a random first row."""
    cm = rng.integers(0, K, (P, 256))
    return rc.Order1ModelSet(np.tile(c, (K, 1)), np.tile(cum, (K, 1)), total,
                             ctx_map=cm if P > 1 else cm[0], first_row=int(rng.integers(0, K)),
                             period=P)


# (K rows, period): period 1 at 1, 8 and 64 rows; periodic sets with one map per phase.  The
# heads steered for (5, 63, and the wide streams' 1, 29, 31) are odd, so mp.align(head) sees a
# head that is no multiple of the period.
O1_SHAPES = [(1, 1), (8, 1), (64, 1), (8, 2), (8, 8)]


@pytest.mark.parametrize("K,P", O1_SHAPES)
@pytest.mark.parametrize("name", MODELS)
def test_order1_tight_streams(ctx, tight_fx, name, K, P):
    c, cum, total, chunks = table(tight_fx, name)
    o1 = order1_set(c, cum, total, K, P, np.random.default_rng(10 * K + P))
    heads = heads_of(chunks)
    assert any(h % P for h in heads) or P == 1
    for head in heads:
        s, sym_off, flags = ring_decode_at(lambda *a: rc.decode_batch_order1(o1, *a), chunks,
                                           (64 - head) % 64)
        ring_check_exact(s, sym_off, flags, chunks)


@pytest.mark.parametrize("K,P", [(8, 1), (8, 8)])
@pytest.mark.parametrize("name", MODELS)
def test_order1_full_launch(ctx, tight_fx, name, K, P):
    c, cum, total, chunks = table(tight_fx, name)
    o1 = order1_set(c, cum, total, K, P, np.random.default_rng(K + P))
    many = full_launch(chunks)
    for head in (0, 5):
        s, sym_off, flags = ring_decode_at(lambda *a: rc.decode_batch_order1(o1, *a), many,
                                           (64 - head) % 64)
        ring_check_exact(s, sym_off, flags, many)


# ---- wide ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_wide_tight_streams(ctx, tight_fx, name):
    """The table as a wide model of n = 256.  Output offsets in 2-byte symbols: 0, 3 and 31
    (heads 0, 29 and 1), the largest head (31: offset 1) and the rest."""
    c, cum, total, chunks = table(tight_fx, name)
    w = rc.WideStaticModel(c, cum, total)
    offs = sorted({(32 - h) % 32 for h in heads_of(chunks, top=31)} | {0, 1, 3, 31})
    for off in offs:
        s, sym_off, flags = ring_decode_at(lambda *a: rc.decode_batch_wide(w, *a), chunks, off,
                                           wide=True)
        ring_check_exact(s, sym_off, flags, chunks)


@pytest.mark.parametrize("name", MODELS)
def test_wide_full_launch(ctx, tight_fx, name):
    c, cum, total, chunks = table(tight_fx, name)
    w = rc.WideStaticModel(c, cum, total)
    many = full_launch(chunks)
    for off in (0, 3):
        s, sym_off, flags = ring_decode_at(lambda *a: rc.decode_batch_wide(w, *a), many, off,
                                           wide=True)
        ring_check_exact(s, sym_off, flags, many)
