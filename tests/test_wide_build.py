"""CPU checks of wide model construction: the library exports rc_histogram_wide and
rc_ideal_bits_wide and refuses a null context without a device, the reference the GPU tests use
(wide_build_ref.py) is pinned to the oracle on 256-bin data, and the wide quantiser equals the
oracle's on a 4096-bin count vector."""
import numpy as np

from range_coder_rust_amd import _native as N
from range_coder_rust_amd import model_build as MB
from oracle import model_build as O
from wide_build_ref import hist_ref, ideal_bits_ref, zipf_counts


def test_library_exports_wide_build_calls():
    lib = N.load()
    for name in ("rc_histogram_wide", "rc_ideal_bits_wide"):
        assert name in N.EXPORTS
        assert hasattr(lib, name), name


def test_null_context_rejected():
    lib = N.load()
    assert lib.rc_histogram_wide(None, None, None, 0, 256, None, None, None) == N.RC_E_ARG
    assert lib.rc_histogram_wide(None, None, None, 1, 256, None, None, None) == N.RC_E_ARG
    assert lib.rc_ideal_bits_wide(None, None, None, None, 0, None) == N.RC_E_ARG
    assert lib.rc_ideal_bits_wide(None, None, None, None, 1, None) == N.RC_E_ARG


def test_histogram_copies_follow_the_alphabet():
    """Many copies of every bin for small alphabets, one at 4096 bins; the counters of all
    copies fit the workgroup's 4096 counter words."""
    lib = N.load()
    assert lib.rc_histogram_wide_copies_(0) == 0 and lib.rc_histogram_wide_copies_(4097) == 0
    for n, want in ((1, 32), (128, 32), (129, 16), (256, 16), (257, 8), (1000, 4), (1024, 4),
                    (2048, 2), (2049, 1), (4096, 1)):
        assert lib.rc_histogram_wide_copies_(n) == want, n
        assert n * want <= 4096


def test_ideal_bits_ref_equals_oracle_on_256_bins():
    rng = np.random.default_rng(1)
    c, _, total = zipf_counts(256)
    c[[7, 200]] = 0  # symbols without a code length
    chunks = [rng.integers(0, 256, int(k)).astype(np.uint16) for k in (0, 1, 50, 3000)]
    chunks.append(np.array([1, 2, 7], np.uint16))
    chunks.append(np.array([], np.uint16))
    rows = np.stack([hist_ref(ch, 256)[0] for ch in chunks])
    got = ideal_bits_ref(chunks, c, total)
    want = O.ideal_bits(rows, [int(x) for x in c], total)
    assert got.tolist() == want.tolist()  # the same sums in the same order: bit-equal
    assert np.isinf(got[4]) and got[5] == 0.0
    # a symbol past a shorter alphabet has no code length either
    short = ideal_bits_ref([np.array([3, 299, 300], np.uint16), np.array([299], np.uint16)],
                           np.ones(300, np.uint32), 300)
    assert np.isinf(short[0]) and np.isfinite(short[1])


def test_quantize_counts_wide_equals_oracle_at_4096_bins():
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 1000, 4096).astype(np.uint64)
    counts[rng.random(4096) < 0.3] = 0
    counts[17] = 10 ** 7
    for T, all_symbols in ((1 << 16, True), (1 << 16, False), (4096, True), (0, False)):
        want = O.quantize_counts(counts, T, O.Q_ALL_SYMBOLS if all_symbols else 0)
        c, cum, total = MB.quantize_counts_wide(counts, T, all_symbols)
        assert (list(c), list(cum), total) == (want[0], want[1], want[2]), (T, all_symbols)
