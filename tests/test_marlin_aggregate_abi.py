"""CPU: the device form of the aggregated Marlin check is part of the C ABI -- zk_marlin_verify_aggregate_coeffs,
zk_marlin_verify_aggregate and the hook zk_diag_g1_term_sum_dev are exported by the built library, declared in include/zkmpc_hip.h,
bound in zk-mpc_amd/_lib.py with the header's argument counts and present in the regenerated Rust bindings; without a device the calls
refuse a null context rather than compute anything on the host."""
import ctypes as C
import os
import re

import zk_mpc_amd as Z
import zk_mpc_amd.marlin as DM
from zk_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"zk_marlin_verify_aggregate_coeffs": 10, "zk_marlin_verify_aggregate": 10, "zk_diag_g1_term_sum_dev": 7}


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "zkmpc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name + " is not declared in include/zkmpc_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_the_three_symbols_are_exported_declared_and_bound():
    lib = Z.load()
    rust = open(os.path.join(ROOT, "bindings", "hip_ffi.rs")).read()
    for name, arity in NEW.items():
        assert hasattr(lib, name), "libzkmpc_hip.so does not export " + name
        assert _header_arity(name) == arity
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == arity, name
        m = re.search(r"pub fn %s\((.*)\) -> i32;" % name, rust)
        assert m, name + " is not in bindings/hip_ffi.rs"
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(", ")) == arity, name
    # the host form keeps the contract the device form is held to: same arguments but the context
    assert _header_arity("zk_marlin_verify_aggregate_host") == NEW["zk_marlin_verify_aggregate_coeffs"] - 1
    assert _header_arity("zk_diag_g1_glv_sum_host") == NEW["zk_diag_g1_term_sum_dev"] - 2


def test_python_forms_exist():
    for name in ("verify_aggregate", "verify_aggregate_coeffs", "diag_g1_term_sum"):
        assert callable(getattr(DM, name)), name
    assert (DM.TERM_FULL, DM.TERM_GLV) == (0, 1)


def test_a_null_context_is_refused_before_anything_is_read():
    lib = Z.load()
    ok = C.c_int(7)
    assert lib.zk_marlin_verify_aggregate_coeffs(None, None, 1, None, 0, None, None, None, C.byref(ok), None) == -2
    assert lib.zk_marlin_verify_aggregate(None, None, 1, None, 0, None, None, None, C.byref(ok), None) == -2
    assert lib.zk_diag_g1_term_sum_dev(None, None, None, 1, 0, None, None) == -2
    assert ok.value == 7
