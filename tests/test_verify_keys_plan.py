"""CPU: zk-mpc_amd/csrc/verify_keys_plan.hpp, from which Groth16 verification over several keys (csrc/groth16_verify_keys.hip) takes
the grouping of a batch by key and every index of the keyed sum -- the single-key entry points included, which plan one slot.  tests/verify_keys_plan_main.cpp drives the header alone: the
stable permutation, segment and input offsets, unused keys, the identity plan of one key, every refusal, and a replay of every lane of every level -- the kernel's
own lane function, its tree step for step with integers for points, against buffers of exactly the plan's sizes.  Built with g++,
plain and once under the address and undefined-behaviour sanitizers, so a lane outside its buffer is a report."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"),
           os.path.join(ROOT, "tests", "verify_keys_plan_main.cpp"), "-o", exe] + flags
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return r, None
    return r, subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_the_plan_header_alone(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    built, ran = build_and_run(tmp_path, "verify_keys_plan", [])
    assert built.returncode == 0, built.stderr
    assert ran.returncode == 0 and ran.stdout.strip().endswith("ok"), ran.stdout + ran.stderr


def test_the_plan_header_under_the_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    built, ran = build_and_run(tmp_path, "verify_keys_plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0 and any(w in built.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("no sanitizer runtime on this machine")      # (the plain build above has run the program's own checks)
    assert built.returncode == 0, built.stderr
    assert ran.returncode == 0 and ran.stdout.strip().endswith("ok"), ran.stdout + ran.stderr


def test_the_forms_size_their_buffers_from_the_plan():
    """No size of the keyed sum is written out beside the plan: its scratch buffers and its launches name the plan's fields."""
    import re
    src = open(os.path.join(ROOT, "zk-mpc_amd", "csrc", "groth16_verify_keys.hip")).read()
    body = src[src.index("int aggregate_keys_dev("):src.index("// ---- proof by proof")]
    sizes = dict(re.findall(r'zk_scratch\(ctx, "(vk_[a-z_]+)", ([^,]+),', body))
    assert sizes == {"vk_perm": "count * 4", "vk_meta": "pl.meta_words * 4", "vk_part_a": "pl.part_a * XW * 4", "vk_part_b": "(pl.part_b + 1) * XW * 4",
                     "vk_tag_a": "pl.part_a * 4", "vk_tag_b": "(pl.part_b + 1) * 4"}, sizes
    assert "zkvk::keyed_lane(seg_off, mis, n_seg, g)" in src and "atomic" not in src.lower().replace("no atomics", "")
