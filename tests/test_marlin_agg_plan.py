"""CPU: zk-mpc_amd/csrc/marlin_agg_plan.hpp, from which the device form of the aggregated Marlin check takes every launch and buffer
size.  tests/marlin_agg_plan_main.cpp drives the header alone and replays, for count in {1, 3, 4, 5, 32, 33, 313, 314, 315, 2^18}, every
lane of every launch against buffers of exactly the plan's sizes and every pass of the two sum-downs (room for m and m / 64 + 1 points,
at most 64 left) -- built with g++ under the address and undefined-behaviour sanitizers, so a lane outside its buffer is a report."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plan_header_alone_keeps_every_lane_inside_its_buffer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "marlin_agg_plan")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"),
            os.path.join(ROOT, "tests", "marlin_agg_plan_main.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                   # no sanitizer runtime on this machine: the plain build (the program's own checks remain)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_the_entry_point_and_the_hook_size_their_buffers_from_the_plan():
    """No scratch size of the device form is written out beside the plan: every zk_scratch of aggregate_dev and of the hook names a
    field of it."""
    import re
    src = open(os.path.join(ROOT, "zk-mpc_amd", "csrc", "marlin_verify.hip")).read()
    body = src[src.index("int aggregate_dev("):src.index('extern "C" int zk_marlin_verify_aggregate_host')]
    sizes = re.findall(r'zk_scratch\(ctx, "[a-z_]+", ([^,]+),', body)
    assert len(sizes) == 9 and all(s.startswith("pl.") for s in sizes), sizes
    hook = open(os.path.join(ROOT, "zk-mpc_amd", "csrc", "g1_term_fold.hip")).read()
    parts = re.findall(r'zk_scratch\(ctx, "term_part_[ab]", ([^,]+),', hook)
    assert parts == ["sp.part_a * AGG_XYZZ_BYTES", "sp.part_b * AGG_XYZZ_BYTES"]
