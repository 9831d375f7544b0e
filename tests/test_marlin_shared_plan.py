"""CPU: zk-mpc_amd/csrc/marlin_shared_plan.hpp, by which the parties of zk_marlin_prove_shared[_spdz]_batch agree on their chunks and
lay out the items of a chunk's small opens.  tests/marlin_shared_plan_main.cpp drives the header alone: the minimum over 1, 2 and 8
parties, one zero among the bounds meaning no for all, the chunks of count in {1, 2, 5, 64, 65} under caps {1, 2, 64} covering every
proof once with a short last chunk where it should be, and for lanes 1 and 2 a distinct slot for every (proof, item, lane), ordered by
proof within each kind -- built with g++ under the address and undefined-behaviour sanitizers where they link."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plan_header_alone(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "marlin_shared_plan")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"),
            os.path.join(ROOT, "tests", "marlin_shared_plan_main.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                   # no sanitizer runtime on this machine: the plain build (the program's own checks remain)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr

