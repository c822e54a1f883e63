"""The direct-table decoder (k_decode_static LUT 6: a byte per q in LDS, 1,024-lane workgroups)
beside the bucket decoder it stands in for (LUT 4), each forced through RC_DEC_PAIR in a fresh
context (6: the direct table, 4: the buckets) and each compared with the C oracle byte for byte:
the encoder's bytes, lengths and flags, the decoded symbols and the decoder's flags.  Models of
the whole class (2048 < total <= 2^16; tests/direct_table_models.py), partial and multiple
1,024-lane workgroups, ragged chunk lengths around the 16-symbol phase and the 64-symbol burst,
code and output offsets at arbitrary alignments, garbage and truncated streams (hints past the
total, the masked index, the exact fix-up reaching c == 0), and the directed ring fixtures
(the ring code is shared; the workgroup shape and the rings' LDS base are new)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from oracle import cpu  # noqa: E402
from gpu_helpers import dev, run_decode, run_encode  # noqa: E402
from direct_table_models import models  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = models()
VARIANTS = ["6", "4"]
LENS = [0, 1, 15, 16, 17, 63, 64, 65, 130, 300, 700]
# every model at 1025 chunks (a full workgroup and one lane of the next); the headline's model
# and the smallest total (the magic-division kernels) at every shape
CASES = [(name, 1025) for name in sorted(MODELS)] + [
    (name, n) for name in ("zipf65536", "zipf2049") for n in (1, 1023, 2049)]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


_REF = {}


def _chunks(name, n_chunks):
    """Ragged chunks of the model's symbols and the oracle's code for each, made once."""
    key = (name, n_chunks)
    if key not in _REF:
        c, cum, total = MODELS[name]
        rng = np.random.default_rng(len(name) * 1000 + n_chunks)
        lens = [300] if n_chunks == 1 else [LENS[k % len(LENS)] for k in range(n_chunks)]
        if name == "rare_heavy":  # the c = 1 symbols, a few runs of the large one between them
            pool = rng.integers(2, 256, sum(lens))
            pool[rng.random(len(pool)) < 0.05] = 0
        else:
            pool = rng.choice(len(c), sum(lens), p=c / c.sum())
        pool = pool.astype(np.uint8)
        ends = np.cumsum(lens)
        chunks = [pool[e - L:e] for e, L in zip(ends, lens)]
        enc = [cpu.encode(c, cum, total, ch) for ch in chunks]
        _REF[key] = (lens, chunks, enc)
    return _REF[key]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,n_chunks", CASES)
def test_round_trip_vs_oracle(ctx, knob_ctx, name, n_chunks, variant):
    c, cum, total = MODELS[name]
    lens, chunks, enc = _chunks(name, n_chunks)
    m = rc.StaticModel(c, cum, total, ctx=knob_ctx(RC_DEC_PAIR=variant))
    caps = [rc.slot_capacity(L, m.max_bits_per_symbol() + 1) for L in lens]
    out, out_off, ol, fl = run_encode(m, chunks, caps, misalign=True, seed=n_chunks)
    for k, (f, b, L) in enumerate(enc):
        assert (fl[k], ol[k]) == (f, L) and f == 0, k
        assert bytes(out[out_off[k]:out_off[k] + L]) == b, k
    dec, fd = run_decode(m, [b for _, b, _ in enc], lens, misalign=True, seed=n_chunks + 1)
    assert (fd == 0).all(), np.nonzero(fd)[0][:8]
    for k, ch in enumerate(chunks):
        assert (dec[k] == ch).all(), k


def _corrupt(name):
    """Garbage streams, streams shorter than the 8 primed bytes, and valid streams cut inside a
    symbol, with the oracle's flags and symbols for each, made once."""
    key = (name, "corrupt")
    if key not in _REF:
        c, cum, total = MODELS[name]
        rng = np.random.default_rng(len(name) + 77)
        codes = [rng.integers(0, 256, int(rng.integers(8, 400))).astype(np.uint8).tobytes()
                 for _ in range(1100)]
        counts = [int(rng.integers(0, 300)) for _ in codes]
        codes += [rng.integers(0, 256, L).astype(np.uint8).tobytes() for L in range(8)]
        counts += [3] * 8
        _, chunks, enc = _chunks(name, 1025)
        for k in range(8, 1025, 97):  # cut mid-stream, and two bytes before the end
            b = enc[k][1]
            for cut in (len(b) // 2, len(b) - 2):
                codes.append(b[:max(cut, 0)])
                counts.append(len(chunks[k]))
        want = [cpu.decode(c, cum, total, code, n) for code, n in zip(codes, counts)]
        _REF[key] = (codes, counts, want)
    return _REF[key]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_corrupt_streams_decode_like_oracle(ctx, knob_ctx, name, variant):
    """Flags equal the oracle's for every stream; symbols equal the oracle's for every stream it
    decodes without a flag (what a flagged chunk's output holds is not specified)."""
    c, cum, total = MODELS[name]
    codes, counts, want = _corrupt(name)
    m = rc.StaticModel(c, cum, total, ctx=knob_ctx(RC_DEC_PAIR=variant))
    dec, fd = run_decode(m, codes, counts, misalign=True, seed=5)
    flagged = 0
    for k, (f, d) in enumerate(want):
        assert fd[k] == f, (k, fd[k], f)
        if f == 0:
            assert (dec[k] == d).all(), k
        else:
            flagged += 1
    assert flagged >= 8  # (the streams under 8 bytes at the least)


@pytest.fixture(scope="module")
def ring_fx():
    with open(os.path.join(HERE, "golden", "ring_fixtures.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("head", [0, 5, 48])
def test_ring_fixtures_direct_table(ctx, ring_fx, knob_ctx, head):
    """Every directed ring fixture in whole 1,024-lane workgroups of the direct-table decoder:
    code stream k at its fixture alignment mod 64 inside 64-B slots, the output `head` bytes past
    a 64-B boundary (a head of single symbols)."""
    c = np.array(ring_fx["c"], np.uint32)
    cum = np.array(ring_fx["cum"], np.uint32)
    fx = ring_fx["chunks"]
    reps = -(-1100 // len(fx))
    codes = [bytes.fromhex(ch["encoded_hex"]) for ch in fx] * reps
    aligns = [ch["align"] for ch in fx] * reps
    syms = [np.array(ch["symbols"], np.uint8) for ch in fx] * reps
    count = len(syms[0])
    assert all(len(s) == count for s in syms) and count % 64 == 0
    slot = 64 * ((max(len(b) for b in codes) + 64 + 63) // 64)
    blob = np.zeros(slot * len(codes) + 64, np.uint8)
    coff = np.zeros(len(codes), np.int64)
    for k, (b, a) in enumerate(zip(codes, aligns)):
        coff[k] = slot * k + a
        blob[coff[k]:coff[k] + len(b)] = np.frombuffer(b, np.uint8)
    clen = np.array([len(b) for b in codes], np.int64)
    sym_off = np.arange(len(codes) + 1, dtype=np.int64) * count + head
    m = rc.StaticModel(c, cum, ring_fx["total"], ctx=knob_ctx(RC_DEC_PAIR="6"))
    out = torch.full((int(sym_off[-1]) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    flags = rc.decode_batch(m, dev(blob), dev(coff), dev(clen), out, dev(sym_off))
    torch.cuda.synchronize()
    s = out.cpu().numpy()
    assert (flags.cpu().numpy() == 0).all()
    assert (s[:head] == 0xEE).all() and (s[sym_off[-1]:] == 0xEE).all()
    got = s[head:sym_off[-1]].reshape(len(codes), count)
    assert (got == np.stack(syms)).all()


def test_default_dispatch_matches_both(ctx, knob_ctx):
    """The unset switch picks per launch; whichever it picks decodes the same bytes."""
    c, cum, total = MODELS["zipf65536"]
    lens, chunks, enc = _chunks("zipf65536", 2049)
    m = rc.StaticModel(c, cum, total, ctx=knob_ctx(RC_DEC_PAIR="0"))
    dec, fd = run_decode(m, [b for _, b, _ in enc], lens, misalign=True, seed=9)
    assert (fd == 0).all()
    for k, ch in enumerate(chunks):
        assert (dec[k] == ch).all(), k
