"""CPU: Fr on the host (zk-mpc_amd/csrc/hostfr.hpp: the conversions, the 64-bit power, the domain roots, Montgomery's trick) against
oracle/zkref.py.  This test writes the cases and what the oracle says of them; tests/host_fr_main.cpp, which includes the header
alone, reads them back and compares -- under the address and undefined-behaviour sanitizers where they link."""
import os
import shutil
import subprocess

import pytest

import zkref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R_MOD


def _cases():
    rng = O.Prng(0x46720A)
    rand = [rng.fr() for _ in range(3)]
    lines = []
    add = lambda *t: lines.append(" ".join(x if isinstance(x, str) else "%x" % x for x in t))
    for x in (0, 1, 2**29 - 1, 2**29, 2**58 - 1, 2**58, 2**64 - 1):
        add("u64", x, x % R)
    for b in [0, 1, R - 1] + rand:
        for e in (0, 1, 2, 3, 2**32 - 1, 2**32, 2**63, 2**64 - 1):
            add("pow", b, e, pow(b, e, R))
    for log in range(48):
        add("root", log, O.Domain(1 << log).group_gen if log <= 28 else "-")
    for n in (0, 1, 2, 33):
        patterns = {"none": [], "all": range(n), "first": [0], "last": [n - 1], "adjacent": [n // 2 - 1, n // 2]}
        for zeros in patterns.values():
            v = [rng.fr() or 1 for _ in range(n)]
            for i in zeros:
                if 0 <= i < n:
                    v[i] = 0
            add("binv", n, *v, *O.batch_inversion(v))
    for x in [0, 1, R - 1] + rand:
        internal = x * pow(2, 261, R) % R                   # nine limbs of 29 bits, Montgomery radix 2^261
        add("limbs", x, *[(internal >> (29 * i)) & (2**29 - 1) for i in range(9)])
        add("abi", x, x * pow(2, 256, R) % R)               # the reference's form: four 64-bit words, radix 2^256
    return lines


def test_host_fr_equals_the_oracle(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if not hipcc:
        pytest.skip("no hipcc")
    lines = _cases()
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "host_fr")
    base = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"),
            os.path.join(ROOT, "tests", "host_fr_main.cpp"), "-o", exe]
    r = subprocess.run(base + ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                   # no sanitizer runtime on this machine: the plain build
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok %d" % len(lines), r.stdout + r.stderr
