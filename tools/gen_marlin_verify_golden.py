#!/usr/bin/env python3
"""Writes tests/golden/marlin_verify.json: Marlin proofs of two small systems from the project's own CPU oracle
(oracle/marlin_full_ref.py), each with tampered variants and the oracle verifier's verdict on every one.

    python tools/gen_marlin_verify_golden.py          (about half a minute, no GPU)

Per system: how it was made (the seeds, so the device prover can reproduce the good proof), the verifier key as the fields of
zk_marlin_vk_host (points as canonical integers), the public input, and the variants: {name, inputs, proof (hex), verdict}.  A
variant the oracle cannot even deserialise has verdict 0.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import fsrng_ref as FR          # noqa: E402
import marlin_full_ref as MF    # noqa: E402
import marlin_ref as M          # noqa: E402
import zkref as O               # noqa: E402
from helpers import marlin_test_system   # noqa: E402

SYSTEMS = [(3, 0x4d56_0003), ("tiny7", 0x4d56_0007)]
# byte offsets inside the 951-byte proof (8 | 8 + 4 x 49 | 8 + 49 + 97 + 49 | 8 + 97 + 49 | 8 + 7 x 32 | 8 + 3 | 8 + 49 + 32 + 49 | 1)
OFF_W_FLAG, OFF_Z_B, OFF_H_1, OFF_EVALS = 64, 114, 366, 577


def verdict(keys, inputs, data):
    try:
        return int(bool(MF.verify(keys, inputs, MF.proof_deserialize(data))))
    except Exception:
        return 0


def off_curve_x(start):
    x = start
    while O.fq_sqrt((x * x % O.Q_MOD * x + 1) % O.Q_MOD) is not None:
        x += 1
    return x


def outside_subgroup_point(start):
    """x upward from `start` until x^3 + 1 is a square and r P != O: a curve point in the cofactor's part."""
    x = start
    while True:
        y = O.fq_sqrt((x * x % O.Q_MOD * x + 1) % O.Q_MOD)
        if y is not None and O.ec_mul_raw((x, y), O.R_MOD, O.FqOps) is not None:       # (g1_mul reduces its scalar mod r)
            return (x, y)
        x += 1


def variants(keys, inputs, good):
    P = O.R_MOD
    out = []

    def add(name, data, inp=None):
        inp = list(inputs) if inp is None else inp
        out.append({"name": name, "inputs": [hex(v) for v in inp], "proof": bytes(data).hex(), "verdict": verdict(keys, inp, bytes(data))})

    def edited(fn):
        pr = MF.proof_deserialize(good)
        fn(pr)
        return pr.serialize()

    add("good", good)
    add("wrong_input", good, [(inputs[0] + 1) % P] + list(inputs[1:]))

    def ev(i):
        def f(pr):
            pr.evaluations[i] = (pr.evaluations[i] + 1) % P
        return f
    add("eval_a_denom_plus_1", edited(ev(0)))
    add("eval_z_b_plus_1", edited(ev(6)))

    def swap(pr):
        pr.commitments[0][0], pr.commitments[0][1] = pr.commitments[0][1], pr.commitments[0][0]
    add("w_z_a_swapped", edited(swap))

    def wit(pr):
        pr.pc_proof[1] = (O.g1_mul(O.G1_GEN, 0x1234567), pr.pc_proof[1][1])
    add("wit_gamma_other_point", edited(wit))

    def rv(pr):
        assert pr.pc_proof[0][1] is not None
        pr.pc_proof[0] = (pr.pc_proof[0][0], (pr.pc_proof[0][1] + 1) % P)
    add("random_v_plus_1", edited(rv))

    def drop(pr):
        pr.commitments[1][1] = (pr.commitments[1][1][0], None, False)
    add("g_1_shifted_dropped", edited(drop))

    def extra(pr):
        pr.commitments[1][0] = (pr.commitments[1][0][0], pr.commitments[1][1][1], True)
    add("t_shifted_added", edited(extra))

    b = bytearray(good)
    b[OFF_EVALS + 3 * 32:OFF_EVALS + 4 * 32] = P.to_bytes(32, "little")
    add("eval_is_r", b)

    b = bytearray(good)
    x = int.from_bytes(bytes(b[OFF_H_1:OFF_H_1 + 47]) + bytes([b[OFF_H_1 + 47] & 0x3f]), "little")
    b[OFF_H_1:OFF_H_1 + 48] = off_curve_x(x).to_bytes(48, "little")
    add("h_1_off_curve", b)

    b = bytearray(good)
    pt = outside_subgroup_point(0x5eed)
    b[OFF_Z_B:OFF_Z_B + 48] = O.g1_serialize(pt)
    # The oracle's g1_deserialize multiplies by r through g1_mul, which reduces the scalar mod r first: its subgroup test lets every
    # curve point through.  The verdict recorded here is therefore the one its pairing equations give (the commitment is absorbed
    # into the transcript, so they fail); the library rejects the proof earlier, at r P != O.
    add("z_b_outside_subgroup", b)
    assert out[-1]["verdict"] == 0

    add("last_byte_cut", good[:-1])
    add("one_byte_appended", good + b"\x00")
    b = bytearray(good)
    assert b[OFF_W_FLAG] == 0
    b[OFF_W_FLAG] = 2
    add("option_flag_2", b)
    return out


def system(n, seed):
    rng = O.Prng(seed)
    r1cs, z = marlin_test_system(n, rng)
    sq, zz = M.pad_and_square(r1cs, z)
    oix = M.Index(sq)
    beta, g_k, gg_k, h_k = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    pp = O.KzgParams(MF.max_degree_for(oix) + 3, beta, g_k=g_k, gg_k=gg_k, h_k=h_k)
    keys = MF.Keys(oix, pp)
    prover_seed = bytes((11 * i + seed) & 0xff for i in range(32))
    good = MF.prove(keys, zz, FR.ChaChaRng(prover_seed, 20)).serialize()
    assert len(good) == 951
    inputs = list(zz[1:oix.num_instance])
    vs = variants(keys, inputs, good)
    assert vs[0]["verdict"] == 1 and any(v["verdict"] == 1 for v in vs), "the oracle rejects its own proof"
    g1 = lambda p: [hex(p[0]), hex(p[1])]
    g2 = lambda p: [[hex(p[0][0]), hex(p[0][1])], [hex(p[1][0]), hex(p[1][1])]]
    key = {"ivk_bytes": keys.ivk_bytes().hex(), "g": g1(pp.g), "gamma_g": g1(pp.gamma_g), "h": g2(pp.h), "beta_h": g2(pp.beta_h),
           "shift_h": g1(keys.shift_power(keys.bounds["g_1"])), "shift_k": g1(keys.shift_power(keys.bounds["g_2"]))}
    return {"system": n, "prng_seed": seed, "prover_seed": prover_seed.hex(), "max_degree": keys.max_degree,
            "srs": {"beta": hex(beta), "g_k": hex(g_k), "gamma_g_k": hex(gg_k), "h_k": hex(h_k)},
            "dom_h": oix.dom_h.size, "dom_k": oix.dom_k.size, "num_instance": oix.num_instance,
            "key": key, "inputs": [hex(v) for v in inputs], "variants": vs}


def main():
    doc = {"generator": "tools/gen_marlin_verify_golden.py", "systems": [system(n, s) for n, s in SYSTEMS]}
    path = os.path.join(ROOT, "tests", "golden", "marlin_verify.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for s in doc["systems"]:
        print(s["system"], "|H|", s["dom_h"], "|K|", s["dom_k"], {v["name"]: v["verdict"] for v in s["variants"]})


if __name__ == "__main__":
    main()
