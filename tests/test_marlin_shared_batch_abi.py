"""zk_marlin_prove_shared_batch / zk_marlin_prove_shared_spdz_batch at the C boundary, without a GPU: the symbols are exported, their
ctypes signatures and the generated Rust declarations agree with the header argument for argument, and NULL arguments are refused
before any device is touched."""
import ctypes as C
import os
import re

import pytest

import zk_mpc_amd
from zk_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_ERR_ARG = -2
TAIL = ["net", "proofs_out", "slot", "proof_lens", "bytes_sent"]
HEAD = ["ctx", "index", "powers_g", "powers_gamma_g", "count"]
NAMES = {
    "zk_marlin_prove_shared_batch": HEAD + ["z_share_dev", "z_stride", "rngs", "mask_on_device", "tx", "ty", "tz"] + TAIL,
    "zk_marlin_prove_shared_spdz_batch": HEAD + ["z_lanes_dev[2]", "z_stride", "rngs", "mask_on_device", "tx_lanes[2]", "ty_lanes[2]", "tz_lanes[2]"] + TAIL,
}


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "zkmpc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "include/zkmpc_hip.h does not declare " + name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_the_symbol_is_exported(name):
    lib = zk_mpc_amd.load()
    assert hasattr(lib, name)
    assert name in _lib.PROTOTYPES


@pytest.mark.parametrize("name", sorted(NAMES))
def test_ctypes_and_rust_agree_with_the_header(name):
    args = _header_args(name)
    assert [a.split()[-1].lstrip("*") for a in args] == NAMES[name]
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is C.c_int and len(argtypes) == len(args)
    rust = open(os.path.join(ROOT, "bindings", "hip_ffi.rs")).read()
    m = re.search(r"pub fn %s\((.*)\) -> i32;" % name, rust)
    assert m, "bindings/hip_ffi.rs does not declare " + name
    rust_args = [a.split(":", 1)[1].strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(", ")]
    assert len(rust_args) == len(args)
    for c_arg, ct, ra in zip(args, argtypes, rust_args):
        is_ptr = "*" in c_arg or "[" in c_arg
        assert (ct is C.c_void_p) == is_ptr, (c_arg, ct)
        assert ra.startswith("*") == is_ptr, (c_arg, ra)
        if not is_ptr:
            want = {"size_t": (C.c_size_t, "usize"), "int": (C.c_int, "i32")}[c_arg.split()[0]]
            assert (ct, ra) == want, (c_arg, ct, ra)
    assert rust_args[7] == "*const *mut ZkRng"          # count generators, one per proof
    assert rust_args[-1] == "*mut u64" and rust_args[-2] == "*mut usize"
    if name.endswith("spdz_batch"):
        assert rust_args[5] == "*const *const c_void"   # {share, MAC share}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_null_arguments_are_refused_without_a_device(name):
    lib = zk_mpc_amd.load()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    slot = lib.zk_marlin_proof_max_size()
    fn = getattr(lib, name)
    assert fn(None, p, p, p, 2, p, 8, p, 0, None, None, None, None, p, slot, p, None) == ZK_ERR_ARG
    assert fn(None, None, None, None, 0, None, 0, None, 0, None, None, None, None, None, 0, None, None) == ZK_ERR_ARG
