"""The models of the direct-table decoder's tests (test_direct_table.py on the host,
test_gpu_direct_table.py on the GPU): static models of the small bucket class, 2048 < total <=
2^16, which k_decode_static decodes through the buckets (LUT 4) or through the q-to-symbol table
(LUT 6)."""
import numpy as np

from range_coder_rust_amd import synth


def cum_of(c):
    c = np.asarray(c, dtype=np.uint64)
    return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.uint32)


def _zipf(total, n=256):
    w = 1.0 / np.arange(1, n + 1) ** 1.2
    c = np.maximum(1, np.floor(w / w.sum() * total)).astype(np.int64)
    c[int(np.argmax(c))] += total - c.sum()
    assert c.min() >= 1 and c.sum() == total
    return c.astype(np.uint32)


def _sparse():
    """Fewer than 256 symbols, three of them with c == 0 (they own no table entry)."""
    rng = np.random.default_rng(11)
    c = rng.integers(1, 400, 200).astype(np.uint32)
    c[[5, 77, 150]] = 0
    return c


def _rare_heavy(total=65536, c_big=65536 - 255):
    """test_gpu_parity.py::test_rare_heavy_models' table: 254 symbols of c = 1 beside a large
    one, so coding the rare ones settles 2-3 bytes a symbol and range_reduction_expansion runs
    often."""
    c = np.ones(256, np.int64)
    c[0] = c_big
    c[1] = total - c_big - 254
    return c.astype(np.uint32)


def models():
    """name -> (c, cum, total)"""
    out = {}
    c, cum, total = synth.zipf_table()  # the headline's model: Zipf(1.2), total 2^16
    out["zipf65536"] = (np.asarray(c, np.uint32), np.asarray(cum, np.uint32), int(total))
    for total in (2049, 4096, 65535):  # the smallest of the class (magic division); pow2; 2^16 - 1
        c = _zipf(total)
        out[f"zipf{total}"] = (c, cum_of(c), total)
    c = _sparse()
    out["sparse"] = (c, cum_of(c), int(c.sum()))
    c = _rare_heavy()
    out["rare_heavy"] = (c, cum_of(c), 65536)
    for name, (c, cum, total) in out.items():
        assert 2048 < total <= 65536 and int(c.astype(np.uint64).sum()) == total, name
    return out
