#!/usr/bin/env python3
"""Writes tests/golden/marlin_aggregate.json: four ACCEPTED Marlin proofs of one key from the project's own CPU oracle
(oracle/marlin_full_ref.py), for the aggregated verifier's tests -- a folded check needs several good proofs of one key, and
tests/golden/marlin_verify.json holds one per system.

    python tools/gen_marlin_aggregate_golden.py          (about a quarter of a minute, no GPU)

The key is the one of marlin_verify.json's system 3 (the mul-chain of three constraints), rebuilt from that fixture's seeds and held
to its recorded bytes; the proofs are of two assignments O.mul_chain_r1cs(3, a, b), two prover seeds each.  Per proof: the assignment's
(a, b), the prover seed, the public input, the proof (hex) and the oracle verifier's verdict on it.
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

SYSTEM = 3
ASSIGNMENT_SEED = 0xA66_0003


def main():
    with open(os.path.join(ROOT, "tests", "golden", "marlin_verify.json")) as f:
        system = next(s for s in json.load(f)["systems"] if s["system"] == SYSTEM)
    # tools/gen_marlin_verify_golden.py::system: the assignment's two values first, then the SRS's four
    rng = O.Prng(system["prng_seed"])
    r1cs, z = O.mul_chain_r1cs(SYSTEM, rng.fr(), rng.fr())
    sq, _ = M.pad_and_square(r1cs, z)
    oix = M.Index(sq)
    beta, g_k, gg_k, h_k = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    assert [hex(v) for v in (beta, g_k, gg_k, h_k)] == [system["srs"][n] for n in ("beta", "g_k", "gamma_g_k", "h_k")]
    keys = MF.Keys(oix, O.KzgParams(MF.max_degree_for(oix) + 3, beta, g_k=g_k, gg_k=gg_k, h_k=h_k))
    assert keys.ivk_bytes().hex() == system["key"]["ivk_bytes"], "not the fixture's key"

    arng = O.Prng(ASSIGNMENT_SEED)
    proofs = []
    for a_i in range(2):
        a, b = arng.fr(), arng.fr()
        r1, zz = O.mul_chain_r1cs(SYSTEM, a, b)
        _, zz = M.pad_and_square(r1, zz)
        inputs = list(zz[1:oix.num_instance])
        for s_i in range(2):
            prover_seed = bytes((29 * i + 7 * a_i + 3 * s_i + 1) & 0xff for i in range(32))
            data = MF.prove(keys, zz, FR.ChaChaRng(prover_seed, 20)).serialize()
            assert len(data) == 951
            verdict = int(bool(MF.verify(keys, inputs, MF.proof_deserialize(data))))
            assert verdict == 1, "the oracle rejects its own proof"
            proofs.append({"a": hex(a), "b": hex(b), "prover_seed": prover_seed.hex(), "inputs": [hex(v) for v in inputs],
                           "proof": data.hex(), "verdict": verdict})
    doc = {"generator": "tools/gen_marlin_aggregate_golden.py", "system": SYSTEM, "key_of": "tests/golden/marlin_verify.json",
           "assignment_seed": ASSIGNMENT_SEED, "proofs": proofs}
    path = os.path.join(ROOT, "tests", "golden", "marlin_aggregate.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(len(proofs), "proofs,", os.path.getsize(path), "bytes;", [p["inputs"] for p in proofs])


if __name__ == "__main__":
    main()
