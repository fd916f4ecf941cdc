"""Launch shaping of the add+dom column-pair rounds (band_plan.cpp shape_colpair: round sizing with pair items, the
rest of the band as a single-block tail) under ASan + UBSan, in the stand-alone program
tests/native/colpair_plan_check.cpp.  No GPU."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nldsc_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_colpair_shape_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "sanitize-colpair"], check=True, capture_output=True, timeout=600)
    exe = os.path.join(CSRC, "build", "colpair_plan_check_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "colpair_plan_check OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
