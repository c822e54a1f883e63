"""The host builder of a wide16 fine model's device tables (csrc/rc_wide16_fine_tables.h) in a
stand-alone program built for the host with the address and undefined-behaviour sanitizers: bucket,
rank search and occupied symbol against a brute-force find_index, the ranks per bucket, the padding
and the sentinel, and the encoder's entries, on dense, sparse, two-symbol, one-symbol and
non-power-of-two tables at both bucket counts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide16_fine_tables_match_brute_force_under_sanitizers(tmp_path):
    exe = tmp_path / "wide16_fine_tables_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "wide16_fine_tables_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("8 tables ok"), out.stdout
