"""CPU: the integer half of Marlin::index as the library does it (zk-mpc_amd/csrc/marlin_shape.hpp through zk_diag_marlin_shape_host:
padding of the instance, squaring, balance_matrices, rows sorted by column, the transposes over H, the sizes) against
oracle/marlin_ref.py, entry for entry, on systems given as the circuit gives them; what the call refuses; and
tests/marlin_shape_main.cpp, which drives the header alone and checks its invariants itself."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import zk_mpc_amd.convert as cv
import zk_mpc_amd.marlin as DM
from zk_mpc_amd import _lib
import marlin_index_cases as IC
from helpers import circuit_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(m: "DM.Csr"):
    co = cv.fr_from_mont(m.coeff) if m.nnz else []
    return [[(co[e], int(m.col[e])) for e in range(int(m.row_ptr[r]), int(m.row_ptr[r + 1]))] for r in range(len(m.row_ptr) - 1)]


def _compare(r1cs, z):
    want_info, want, swapped, _ = IC.oracle_shape(r1cs, z)
    info, mats = DM.shape_host(*IC.host_arrays(r1cs))
    assert info == want_info
    for which, (got, w) in enumerate(zip(mats, want)):
        assert _rows(got) == w, which
    return want_info, swapped


@pytest.mark.parametrize("name", IC.GPU_MARLIN_SYSTEMS + IC.HAND_BUILT)
def test_shape_equals_the_oracle(name):
    r1cs, z = IC.system(name)
    info, swapped = _compare(r1cs, z)
    assert info["num_instance"] & (info["num_instance"] - 1) == 0 and info["num_instance"] + info["num_witness"] == info["num_constraints"]
    if name == "more_constraints":          # both branches of squaring: witnesses added here, rows added for the mul-chain
        assert r1cs.num_constraints > r1cs.num_instance + r1cs.num_witness and info["num_witness"] > r1cs.num_witness
    if name == 13:
        assert r1cs.num_constraints < r1cs.num_instance + r1cs.num_witness and info["num_constraints"] > r1cs.num_constraints
    if name == "three_instance":
        assert r1cs.num_instance == 3 and info["num_instance"] == 4
    if name == "swap_some":
        assert any(swapped) and not all(swapped)
    if name == "swap_none":
        assert not any(swapped)
    if name == "empty_c":
        assert not any(r1cs.c)
    if name == "repeated_column":
        assert any(len({i for _, i in row}) < len(row) for row in r1cs.a)


def test_an_instance_count_that_is_no_power_of_two_from_the_generator():
    r1cs, z = circuit_system((9, 2, 2), 4242)
    assert r1cs.num_instance == 3
    info, _ = _compare(r1cs, z)
    assert info["num_instance"] == 4 and info["num_witness_in"] == r1cs.num_witness


def _raw(h, which=0, cap=64, info=True):
    rp, col, co = np.zeros(256, np.uint32), np.zeros(cap, np.uint32), np.zeros((cap, 4), np.uint64)
    out = _lib.MarlinIxInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return _lib.load().zk_diag_marlin_shape_host(None if h is None else C.byref(h), which, p(rp), p(col), p(co), cap, C.byref(out) if info else None)


def test_what_the_shape_call_refuses():
    r1cs, _ = IC.system("swap_some")
    ni, nw, a, b, c = IC.host_arrays(r1cs)
    good, _k = DM._r1cs_host(ni, nw, a, b, c)
    assert _raw(good) == 0 and _raw(good, info=False) == 0
    assert _raw(None) == -2 and _raw(good, which=6) == -2 and _raw(good, which=-1) == -2
    assert _raw(good, cap=3) == -2                                          # A has four entries after balancing
    h, _k1 = DM._r1cs_host(0, nw + ni, a, b, c)
    assert _raw(h) == -2                                                    # num_instance = 0
    rp = a[0].copy(); rp[0] = 1
    h, _k2 = DM._r1cs_host(ni, nw, (rp, a[1], a[2]), b, c)
    assert _raw(h) == -2                                                    # a row_ptr that does not start at 0
    rp = a[0].copy(); rp[2] = rp[1] - 1
    h, _k3 = DM._r1cs_host(ni, nw, (rp, a[1], a[2]), b, c)
    assert _raw(h) == -2                                                    # ... that decreases
    col = b[1].copy(); col[-1] = ni + nw
    h, _k4 = DM._r1cs_host(ni, nw, a, (b[0], col, b[2]), c)
    assert _raw(h) == -2                                                    # a column that is no variable
    h, _k5 = DM._r1cs_host(ni, nw, a, b, c)
    h.c_row_ptr = None
    assert _raw(h) == -2                                                    # a null pointer inside
    assert _raw(good) == 0


def test_the_shape_header_alone_checks_its_invariants(tmp_path):
    """tests/marlin_shape_main.cpp: square, instance a power of two, entries conserved, rows sorted, each transpose agrees with its
    matrix, the greedy rule replayed on the row lengths -- over generated systems, under the address and undefined-behaviour
    sanitizers where they link."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "marlin_shape")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zk-mpc_amd", "csrc"),
            os.path.join(ROOT, "tests", "marlin_shape_main.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                   # no sanitizer runtime on this machine: the plain build
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
