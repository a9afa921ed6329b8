"""The pass kernels' store after the recursion against the rule it is built on (csrc/rmpc_inst.hpp): the host program
tests/host/after_recursion_check.cpp runs store_after_recursion and inst_load -> inst_after_recursion -> inst_store on
two copies of a one-instance workspace, for every outcome of the recursion, scaled-curvature weights around kCsMin,
back-off lengths up to kCurvBackMax and every kernel variant, and compares every word."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_store_after_recursion_matches_the_rule(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "after_recursion_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Irobot_mpcs_amd/csrc", "-Iinclude",
                           "tests/host/after_recursion_check.cpp", "-o", exe], cwd=ROOT)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "OK" and len(lines) == 12, run.stdout   # 11 variants of 64 cases each
    assert all(" 64 cases, 0 mismatches" in ln for ln in lines[:-1]), run.stdout
