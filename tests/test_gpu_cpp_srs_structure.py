"""-m gpu: builds and runs tests/cpp/test_srs_structure.cpp (Setup::check_powers, from_lagrange_points, contribute and
verify_contribution of host/baby_plonk.hpp) against libbp_msm_ntt.so"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_setup_structure(tmp_path):
    exe = str(tmp_path / "test_srs_structure")
    libdir = os.path.join(ROOT, "baby_plonk_rust_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "test_srs_structure.cpp"), "-o", exe,
                           "-L" + libdir, "-lbp_msm_ntt", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "srs structure ok" in out.stdout
