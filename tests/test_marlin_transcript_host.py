"""CPU: Marlin's Fiat-Shamir transcript (zk-mpc_amd/csrc/marlin_transcript.hpp: what the provers and the verifier share) against
oracle/marlin_full_ref.py::transcript_challenges.  This test writes the cases -- the commitments as affine coordinates -- and what the
oracle derives from them; tests/marlin_transcript_main.cpp, which includes the header alone, reads them and prints alpha, eta_a, eta_b,
eta_c, beta, gamma and the opening challenge xi, compared exactly -- under the address and undefined-behaviour sanitizers where they link."""
import os
import shutil
import subprocess

import pytest

import zkref as O
import marlin_full_ref as MF
import marlin_verify_cases as MC

ROOT = MC.ROOT


def _cases():
    """(name, |H|, ivk, public input, commitments, evaluations) -- the `good` proof of each fixture system; the same with one
    commitment of each round replaced by the identity (the (0, 1, infinity) encoding, which an empty polynomial's commitment produces
    and no fixture proof contains), as the commitment itself and as a shifted one; a seed with no public input beside the constant 1."""
    out = []
    for system in MC.fixture()["systems"]:
        keys = MC.oracle_keys(system)
        good = system["variants"][0]
        assert good["name"] == "good"
        inputs = [int(x, 16) for x in good["inputs"]]
        inputs += [0] * (max(len(inputs), O.Domain(len(inputs) + 1).size - 1) - len(inputs))      # as Marlin::verify formats them
        proof = MF.proof_deserialize(bytes.fromhex(good["proof"]))
        base = (system["dom_h"], keys, inputs)
        name = "system %s " % system["system"]
        out.append((name + "good",) + base + (proof.commitments, proof.evaluations))

        def with_identity(at):
            cs = [list(rnd) for rnd in proof.commitments]
            for rnd, i, shifted in at:
                comm, s, has = cs[rnd][i]
                assert has or not shifted
                cs[rnd][i] = (comm, None, has) if shifted else (None, s, has)
            return cs
        out.append((name + "identity: w, t, g_2",) + base + (with_identity([(0, 0, False), (1, 0, False), (2, 0, False)]), proof.evaluations))
        out.append((name + "identity: mask_poly, g_1 shifted, h_2",) + base + (with_identity([(0, 3, False), (1, 1, True), (2, 1, False)]), proof.evaluations))
        if len(out) == 3:
            out.append((name + "no public input", system["dom_h"], keys, [], proof.commitments, proof.evaluations))
    return out


def _line(dom_h, keys, inputs, commitments, evaluations):
    pt = lambda p: "inf" if p is None else "%x:%x" % p
    t = ["%x" % dom_h, keys.ivk_bytes().hex(), "%x" % len(inputs)] + ["%x" % x for x in inputs]
    assert [len(r) for r in commitments] == [4, 3, 2]
    for rnd in commitments:
        for comm, shifted, has in rnd:
            t += [pt(comm), pt(shifted) if has else "-"]
    assert len(evaluations) == 7
    return " ".join(t + ["%x" % e for e in evaluations])


def _oracle(dom_h, keys, inputs, commitments, evaluations):
    assert keys.index.dom_h.size == dom_h
    ch, fs = MF.transcript_challenges(keys.ivk_bytes(), keys.index, inputs, commitments)
    fs.absorb(b"".join(MF.fr_bytes(e) for e in evaluations))
    xi = fs.next_u128() % O.R_MOD
    return " ".join("%x" % v for v in (ch["alpha"], ch["eta_a"], ch["eta_b"], ch["eta_c"], ch["beta"], ch["gamma"], xi))


def test_transcript_header_derives_the_oracles_challenges(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if not hipcc:
        pytest.skip("no hipcc")
    cases = _cases()
    assert len(cases) == 7 and any(not c[3] for c in cases)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(_line(*c[1:]) for c in cases) + "\n")
    exe = str(tmp_path / "marlin_transcript")
    base = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"),
            os.path.join(ROOT, "tests", "marlin_transcript_main.cpp"), "-o", exe]
    r = subprocess.run(base + ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                   # no sanitizer runtime on this machine: the plain build
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.strip().split("\n")
    want = [_oracle(*c[1:]) for c in cases]
    assert len(got) == len(want)
    wrong = [(c[0], g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, wrong
    assert len(set(want)) == len(want)      # every case moves the transcript
