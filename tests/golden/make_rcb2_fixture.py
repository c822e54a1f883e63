"""Generates tests/golden/rcb2_order1.json (committed).  Run from the repo root:

    python tests/golden/make_rcb2_fixture.py

One small RCB2 container of kind 2 (an order-1 set) with the checksum section, built entirely on
the CPU: a seeded K = 4 set over 16 symbols, three chunks of its chain (the last one ragged),
streams from tests/order1_ref.py, framing and checksums from tests/container2_ref.py.  The GPU
must decode the blob to the recorded symbols and write the same bytes from the same model
(tests/test_gpu_container2.py), which pins the format across commits."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import container2_ref as R  # noqa: E402
import order1_ref as O1  # noqa: E402

SEED, K, N_SYMBOLS, TOTAL, CHUNK, N = 20260, 4, 16, 4096, 1000, 2333


def main():
    rng = np.random.default_rng(SEED)
    rows = O1.markov_rows(rng, K, N_SYMBOLS, TOTAL)
    ctx_map = rng.integers(0, K, N_SYMBOLS).astype(np.uint8)
    first_row = 2
    c, cum = O1.tables(rows)
    syms = O1.draw_markov(rng, rows, ctx_map, first_row, N)
    chunks = [syms[i:i + CHUNK] for i in range(0, N, CHUNK)]
    codes = []
    for ch in chunks:
        f, b = O1.encode_ref(c, cum, TOTAL, ctx_map, first_row, ch)
        assert f == 0
        f, back = O1.decode_ref(c, cum, TOTAL, ctx_map, first_row, b, len(ch))
        assert f == 0 and np.array_equal(back, ch)
        codes.append(b)
    blob = R.build(R.KIND_ORDER1, N_SYMBOLS, chunks, codes, c=c, total=TOTAL, ctx_map=ctx_map,
                   first_row=first_row, checksums=True)
    p = R.parse(blob)
    assert p["container_bytes"] == len(blob) and p["sums"] == [R.checksum(x) for x in chunks]
    out = {"seed": SEED, "n_models": K, "n_symbols": N_SYMBOLS, "total_freq": TOTAL,
           "chunk_size": CHUNK, "n_chunks": len(chunks), "container_hex": blob.hex(),
           "symbols_hex": syms.tobytes().hex()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rcb2_order1.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{path}: container {len(blob)} bytes, {N} symbols")


if __name__ == "__main__":
    main()
