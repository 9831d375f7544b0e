"""zk_marlin_prove_batch at the C boundary, without a GPU: the symbol is exported, its ctypes signature and the generated Rust
declaration agree with the header argument for argument, and NULL arguments are refused before any device is touched."""
import ctypes as C
import os
import re

import zk_mpc_amd
from zk_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zk_marlin_prove_batch"
ZK_ERR_ARG = -2


def _header_args():
    text = open(os.path.join(ROOT, "include", "zkmpc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "include/zkmpc_hip.h does not declare " + NAME
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_symbol_is_exported():
    lib = zk_mpc_amd.load()
    assert hasattr(lib, NAME)
    assert NAME in _lib.PROTOTYPES


def test_ctypes_and_rust_agree_with_the_header():
    args = _header_args()
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "index", "powers_g", "powers_gamma_g", "count", "z_dev", "z_stride", "rngs",
                                                          "mask_on_device", "proofs_out", "slot", "proof_lens"]
    restype, argtypes = _lib.PROTOTYPES[NAME]
    assert restype is C.c_int and len(argtypes) == len(args)
    rust = open(os.path.join(ROOT, "bindings", "hip_ffi.rs")).read()
    m = re.search(r"pub fn %s\((.*)\) -> i32;" % NAME, rust)
    assert m, "bindings/hip_ffi.rs does not declare " + NAME
    rust_args = [a.split(":", 1)[1].strip() for a in m.group(1).split(", ")]
    assert len(rust_args) == len(args)
    for c_arg, ct, ra in zip(args, argtypes, rust_args):
        is_ptr = "*" in c_arg
        assert (ct is C.c_void_p) == is_ptr, (c_arg, ct)
        assert ra.startswith("*") == is_ptr, (c_arg, ra)
        if not is_ptr:
            want = {"size_t": (C.c_size_t, "usize"), "int": (C.c_int, "i32")}[c_arg.split()[0]]
            assert (ct, ra) == want, (c_arg, ct, ra)
    assert rust_args[7] == "*const *mut ZkRng"          # count generators, one per proof


def test_null_arguments_are_refused_without_a_device():
    lib = zk_mpc_amd.load()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    slot = lib.zk_marlin_proof_max_size()
    assert getattr(lib, NAME)(None, p, p, p, 2, p, 8, p, 0, p, slot, p) == ZK_ERR_ARG
    assert getattr(lib, NAME)(None, None, None, None, 0, None, 0, None, 0, None, 0, None) == ZK_ERR_ARG
