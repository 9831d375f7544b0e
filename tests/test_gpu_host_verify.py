"""A compiled VERIFIER above the C ABI (examples/host_verify.cpp, written against include/zkmpc_hip.h alone): two verifying keys from
the bytes VerifyingKey::serialize writes, a batch whose proofs belong to either key, one seeded verdict over both keys
(zk_groth16_vkeys_verify_aggregate) and the verdict of every proof.  CPU: it builds with g++ and fails loudly without a GPU.  GPU: what
it prints is what the Python API answers on the same bytes, for a valid batch and for one with a changed input."""
import struct
import subprocess

import pytest

import zkref as O
import groth16_verify_cases as G
import groth16_keys_cases as K
from test_host_example import build

SEED = bytes(range(40, 72))


def batch_bytes(key_of, xs, data):
    """the example's BATCH file: u64 count, then per proof u32 key, u32 n, n inputs as Fr::serialize writes them, the proof"""
    out = [struct.pack("<Q", len(key_of))]
    for k, x, proof in zip(key_of, xs, data):
        out.append(struct.pack("<II", k, len(x)) + b"".join(int(v).to_bytes(32, "little") for v in x) + bytes(proof))
    return b"".join(out)


def test_the_verifier_host_builds_and_fails_loudly_without_a_gpu(tmp_path):
    import torch
    exe = build(tmp_path, "host_verify")
    if torch.cuda.is_available():
        pytest.skip("GPU present: the gpu test runs it")
    keys = K.four_keys()
    for i, k in enumerate((keys[1], keys[2])):
        (tmp_path / ("key%d" % i)).write_bytes(O.vk_serialize(k.opk, True))
    (tmp_path / "batch").write_bytes(batch_bytes([0], [[5]], [bytes(192)]))
    r = subprocess.run([exe, str(tmp_path / "key0"), str(tmp_path / "key1"), str(tmp_path / "batch")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ok_all" not in r.stdout and "zk_ctx_create" in r.stderr


@pytest.mark.gpu
def test_the_verifier_host_prints_the_verdicts_of_the_python_api(ctx, tmp_path):
    from test_gpu_groth16_verify_keys import device_batch
    keys = K.four_keys()
    two = [keys[1], keys[2]]                                  # one and three public inputs
    exe = build(tmp_path, "host_verify")
    for i, k in enumerate(two):
        (tmp_path / ("key%d" % i)).write_bytes(O.vk_serialize(k.opk, True))
    vkeys = [ctx.vkey_deserialize(O.vk_serialize(k.opk, True), check_subgroup=True) for k in two]
    key_of = [1, 0, 0, 1, 1, 0, 1]
    rng = O.Prng(0x4057)
    xs, abcs = K.forge_batch(two, key_of, rng)
    data = device_batch(ctx, two, key_of, abcs)
    for given, want in ((xs, [1] * 7), (xs[:4] + [G.spoil(xs[4], 2)] + xs[5:], [1, 1, 1, 1, 0, 1, 1])):
        (tmp_path / "batch").write_bytes(batch_bytes(key_of, given, data))
        r = subprocess.run([exe, str(tmp_path / "key0"), str(tmp_path / "key1"), str(tmp_path / "batch"), SEED.hex()], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
        ok, each = ctx.verify_keys_aggregate(vkeys, key_of, K.flat_inputs(given), data.tobytes(), seed=SEED, each=True)
        assert lines["keys"] == "1 3 inputs"
        assert int(lines["ok_all"]) == int(ok) == int(all(want))
        assert [int(v) for v in lines["ok_each"].split()] == each.tolist() == want
    for v in vkeys:
        v.free()
