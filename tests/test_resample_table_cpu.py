"""The coefficient tables of K21 (activezero_amd/csrc/az_resample_table.h: Pillow's triangle-filter tables for 8-bit data)
compiled for the CPU with AddressSanitizer + UBSan and swept over every size pair up to 96 inside the ratio cap -- the same
functions libazhip.so exports as az_resample_bilinear_ksize / az_resample_bilinear_table."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_tables_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the image is expected to have it")
    exe = tmp_path / "resample_table_test"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-Werror", os.path.join(REPO, "tests", "host", "resample_table_test.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "size pairs swept, 0 failures" in run.stdout
