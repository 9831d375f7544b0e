"""What the MSMs started ahead learn (zk-mpc_amd/csrc/msm_spec.hpp: which table follows which with the same scalars, which table takes a
transform's output, two wrong guesses give a table up, confirmations earn it back, forget, off) is host logic over table keys and
integers.  tests/msm_spec_policy_main.cpp drives that header alone, with fake keys, through every rule; it checks itself.  The
device side of the same feature: tests/test_gpu_trait_path.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_learning_rule_of_the_msms_started_ahead(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "msm_spec_policy")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"),
                        os.path.join(ROOT, "tests", "msm_spec_policy_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
