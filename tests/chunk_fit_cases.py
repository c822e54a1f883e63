"""The seeded mixtures that the chunk-set fit is tested on (tests/test_chunk_fit_ref.py on the
host, tests/test_gpu_chunk_set.py on the device)."""
import numpy as np


def zipf_p(n=256, a=1.2):
    w = 1.0 / np.arange(1, n + 1) ** a
    return w / w.sum()


def two_source(n_chunks=96, length=1024, seed=7):
    """-> (chunks uint8[n, length], labels): 40 % of the chunks from Zipf(1.2) over 256 symbols,
    the rest from its mirror image 255 - s"""
    rng = np.random.default_rng(seed)
    labels = (rng.random(n_chunks) >= 0.4).astype(np.uint8)  # 1: the mirror
    p = zipf_p()
    chunks = rng.choice(256, (n_chunks, length), p=p).astype(np.uint8)
    chunks[labels == 1] = 255 - chunks[labels == 1]
    return chunks, labels


def four_source(n_chunks=120, length=512, seed=11):
    """-> (chunks, labels): Zipf(1.2), its mirror, Zipf rotated by 128 symbols, and uniform bytes"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 4, n_chunks).astype(np.uint8)
    base = rng.choice(256, (n_chunks, length), p=zipf_p()).astype(np.uint8)
    chunks = base.copy()
    chunks[labels == 1] = 255 - base[labels == 1]
    chunks[labels == 2] = base[labels == 2] + np.uint8(128)
    uni = rng.integers(0, 256, (n_chunks, length)).astype(np.uint8)
    chunks[labels == 3] = uni[labels == 3]
    return chunks, labels


def histograms(chunks):
    return np.stack([np.bincount(ch, minlength=256) for ch in chunks]).astype(np.uint64)
