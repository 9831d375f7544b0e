"""How the host orders streams (zk-mpc_amd/csrc/stream_order.hpp: the owned event ZkEvent, the fence zk_streams_follow, the stage mark
ZkStageMark) is host logic over four runtime calls.  tests/stream_order_main.cpp drives that header alone, with stand-ins of the
four calls that count live events, log every call and fail on request: no event leaks or dies twice on any path, a fence stops at
its first failing call, a mark makes no call where stream order already holds.  It checks itself.  The device side of the types:
tests/test_gpu_msm.py (the jobs' marks and timers), tests/test_gpu_groth16_flight.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_include():
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "/opt/rocm/include"):
        if os.path.exists(os.path.join(d, "hip", "hip_runtime_api.h")):
            return d
    return None


def test_events_fences_and_stage_marks_on_counting_stand_ins(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    inc = _rocm_include()
    if not inc:
        pytest.skip("no hip/hip_runtime_api.h")
    exe = str(tmp_path / "stream_order")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", inc,
                        "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"), os.path.join(ROOT, "tests", "stream_order_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
