"""bench.py's command line: a plain run measures the headline only, --full adds the extras,
--dump-outputs writes what the last timed step returned (checked here against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from oracle import cpu
from range_coder_rust_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L = 512, 16384  # the bench runs below: 512 chunks of 16 KiB (the adaptive legs' chunk size)


def _args(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _args(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    a = _args(["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full is True and a.dump_outputs == "d"


def test_dump_sample_is_fixed_and_fits():
    a, b = bench.sample_chunks(1 << 20, 58), bench.sample_chunks(1 << 20, 58)
    assert np.array_equal(a, b) and a.dtype == np.int64
    assert len(np.unique(a)) == 58 and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < 1 << 20
    assert np.array_equal(bench.sample_chunks(5, 9), np.arange(5))
    # the default size: every chunk's length and flags, and whole chunks up to the budget
    cap = api.slot_capacity(65536, 8.0, slack=1.02)
    per, full = bench.dump_plan(1 << 20, 65536, cap)
    assert len(per) == 1 << 20 and len(full) >= 32
    assert 16 * len(per) + 4 * (cap + 65536) * len(full) <= bench.DUMP_BYTES <= 64 * 10**6
    # more chunks than the per-chunk files hold: a sample of those too
    per, _ = bench.dump_plan(1 << 22, 1024, api.slot_capacity(1024, 8.0, slack=1.02))
    assert len(per) == bench.DUMP_PER_CHUNK


def _bench(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--global-chunks", str(N), "--chunks", str(N), "--chunk-bytes", str(L)]
                       + argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    d = tmp_path / "dump"
    line = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["bit_exact_round_trip"] is True
    assert line["ms_per_step"] > 0 and line["unit"] == "Gsymbols/s" and line["dtype"] == "u64"
    # value and ms_per_step are one measurement, each rounded to 3 decimals
    assert abs(line["value"] - N * L / line["ms_per_step"] / 1e6) <= \
        line["value"] * 0.0006 / line["ms_per_step"] + 2e-3
    assert line["extras"] == {} and line["cpu_baseline"] is None
    cap = api.slot_capacity(L, 8.0, slack=1.02)
    per, full = bench.dump_plan(N, L, cap)
    assert len(per) == N and 8 <= len(full) < N  # every length; the bytes of a sample
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert {k: (v.dtype, v.shape) for k, v in got.items()} == {
        "code_len": (np.float64, (N,)), "encode_flags": (np.float32, (N,)),
        "decode_flags": (np.float32, (N,)), "code_sample": (np.float32, (len(full), cap)),
        "decoded_sample": (np.float32, (len(full), L))}
    assert sum(v.nbytes for v in got.values()) <= 64 * 10**6
    assert not got["encode_flags"].any() and not got["decode_flags"].any()
    assert line["bytes_per_symbol"] == round(got["code_len"].sum() / (N * L), 5)
    c, cum, total = synth.zipf_table()
    inv = synth.inverse_cdf(c)
    for row in (0, 1, len(full) // 2, len(full) - 1):
        k = int(full[row])
        ch = synth.host_chunk(bench.SEED, inv, k, L)
        f, b, lb = cpu.encode(c, cum, total, ch)
        assert f == 0 and got["code_len"][k] == lb
        assert np.array_equal(got["code_sample"][row, :lb], np.frombuffer(b, np.uint8))
        assert not got["code_sample"][row, lb:].any()
        assert np.array_equal(got["decoded_sample"][row], ch)


@pytest.mark.gpu
def test_full_run_keeps_the_extras():
    line = _bench(["--full", "--steps", "2", "--warmup", "1", "--no-host-stream",
                   "--cpu-seconds", "0.05", "--cpu-threads", "2"])
    assert set(line["extras"]) == {"model_build", "uniform_weak", "container", "adaptive_c4",
                                   "adaptive_c4_128"}
    assert line["bit_exact_round_trip"] is True and line["cpu_baseline"]["value"] > 0
    assert line["extras"]["uniform_weak"]["bit_exact_round_trip"] is True
    assert line["extras"]["container"]["decode_from_container_ok"] is True
