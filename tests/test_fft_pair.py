"""The pair form's lane program (n_fft = 1024: two real frames per 1024-point wave transform, csrc/pair_kernels.h) on the CPU."""
import os
import shutil
import subprocess

import pytest


def test_pair_lane_program_on_host(tmp_path):
    """tests/fft_pair_test.cpp against a double DFT; second line: the pair whose second frame is all zeros (the last pair of an odd frame count)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc) and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "fft_pair_test")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fft_pair_test.cpp")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", src, "-o", exe])
    for line in subprocess.check_output([exe]).decode().split("\n")[:2]:
        spec_a, spec_b, rt_a, rt_b, herm = (float(x) for x in line.split())
        # inputs uniform in [-1, 1): spectra ~ sqrt(1024) * 0.6, 1e-4 absolute is ~5e-6 relative (test_host's bound for the same transform); the round
        # trips are normalised by 1 / 1024 and at most 2 in magnitude: the same relative bound is 1e-5.  The split is bitwise conjugate-symmetric.
        assert spec_a < 1e-4 and spec_b < 1e-4 and rt_a < 1e-5 and rt_b < 1e-5 and herm == 0.0, line
