"""examples/host_marlin.cpp -- a compiled host that goes from the mul-chain's matrices and toxic waste to a Marlin proof and its
verdict through include/zkmpc_hip.h alone (zk_marlin_index_build, zk_marlin_pad_assignment_dev, zk_marlin_prove,
zk_marlin_vk_from_index, zk_marlin_verify_host).  CPU: it builds with g++ and fails loudly without a GPU.  GPU: its proof bytes are
those of prove_native under the same seeds."""
import subprocess

import pytest

import zkref as O
import pyseq.marlin_seq as DM
from zk_mpc_amd.api import Rng
from helpers import mont1
import marlin_index_cases as IC
from test_host_example import build


def test_compiled_marlin_host_builds_and_fails_loudly_without_a_gpu(tmp_path):
    import torch
    exe = build(tmp_path, "host_marlin")
    if torch.cuda.is_available():
        pytest.skip("GPU present: the gpu test runs it")
    r = subprocess.run([exe, "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "proof" not in r.stdout and "zk_ctx_create" in r.stderr


@pytest.mark.gpu
def test_compiled_marlin_host_prints_the_proof_of_prove_native(ctx, tmp_path):
    n = 37
    exe = build(tmp_path, "host_marlin")
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert out["verdict"] == "1" and out["verdict_wrong_input"] == "0"
    # the same toxic waste, assignment seeds and prover seed as the program's
    r1cs, _ = O.mul_chain_r1cs(n, 3, 5)
    info = DM.shape_info(*IC.host_arrays(r1cs))
    srs = DM.UniversalSrs(ctx, info["max_degree_needed"] + 3, 0x5eed1234, 1, 7)
    nix = DM.NativeIndex(ctx, IC.host_arrays(r1cs), srs)
    try:
        z = ctx.mul_chain_assignment_dev(n, mont1(3), mont1(5))
        want = DM.prove_native(nix, nix.pad_assignment(z), Rng.from_seed(bytes((3 * i + 1) & 0xff for i in range(32)), 20))
        assert bytes.fromhex(out["proof"]) == want
    finally:
        nix.free()
