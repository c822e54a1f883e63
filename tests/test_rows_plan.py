"""The rule that picks rc_stream_decode_rows's kernel (rc_rows.hip, rows_decode_plan; DESIGN.md
§9.18), through its host-only hooks: no device is needed.  0 is the wave-per-stream kernel, 1 the
lane-per-stream kernel."""
import ctypes

import numpy as np
import pytest

from range_coder_rust_amd import _native as N
import rows_ref as RR

CUS = (1, 256)


@pytest.fixture(scope="module")
def lib():
    return N.load()


def plan_curve(lib, n_symbols, n_cus, upto):
    """the plan at every stream count 1..upto (every one: nothing is sampled)"""
    return np.fromiter((lib.rc_rows_decode_plan_(n, n_symbols, n_cus) for n in range(1, upto + 1)),
                       np.int8, upto)


@pytest.mark.parametrize("n_cus", CUS)
@pytest.mark.parametrize("n_symbols", RR.SIZES)
def test_64_streams_or_fewer_take_the_wave_kernel(lib, n_symbols, n_cus):
    assert [lib.rc_rows_decode_plan_(n, n_symbols, n_cus) for n in range(0, 65)] == [0] * 65


@pytest.mark.parametrize("n_cus", CUS)
@pytest.mark.parametrize("n_symbols", RR.SIZES)
def test_monotone_in_the_stream_count(lib, n_symbols, n_cus):
    """Over 1..2^20 streams the plan is 0, then 1, and only 0 or 1."""
    p = plan_curve(lib, n_symbols, n_cus, 1 << 20)
    assert set(np.unique(p).tolist()) <= {0, 1}
    assert (np.diff(p) >= 0).all()
    assert p[:64].max() == 0


def test_many_streams_take_the_lane_kernel(lib):
    assert lib.rc_rows_decode_plan_(65536, 256, 256) == 1
    assert lib.rc_rows_decode_plan_(65536, 64, 256) == 1
    # the stream count does not wrap on its way to the rule
    assert lib.rc_rows_decode_plan_(0xFFFFFFFF, 256, 0xFFFFFFFF) in (0, 1)
    assert lib.rc_rows_decode_plan_(0xFFFFFFFF, 256, 256) == 1


def test_the_choice_hook_rejects_bad_arguments(lib):
    """A null context, and a choice beyond 2 (refused before the context is read: a block of
    zeroed host memory stands in for one, since no context exists without a device)."""
    for which in (0, 1, 2, 3):
        assert lib.rc_rows_decoder_(None, which) == N.RC_E_ARG
    fake = ctypes.create_string_buffer(4096)
    for which in (3, 4, 0xFFFFFFFF):
        assert lib.rc_rows_decoder_(ctypes.cast(fake, ctypes.c_void_p), which) == N.RC_E_ARG
    assert fake.raw == bytes(4096)
