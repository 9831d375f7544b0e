"""The batch entry points (zk_msm_g*_multi_dev, zk_groth16_prove_batch*) refuse a null context with ZK_ERR_ARG, without a GPU."""
import ctypes as C

import zk_mpc_amd

ZK_ERR_ARG = -2


def test_batch_entry_points_reject_a_null_context():
    lib = zk_mpc_amd.load()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    assert lib.zk_msm_g1_multi_dev(None, p, 0, p, 1, 1, 1, p) == ZK_ERR_ARG
    assert lib.zk_msm_g2_multi_dev(None, p, 0, p, 1, 1, 1, p) == ZK_ERR_ARG
    assert lib.zk_groth16_prove_batch_dev(None, p, p, 1, p, p, p, p) == ZK_ERR_ARG
    assert lib.zk_groth16_prove_batch(None, p, p, 1, p, p, p, p) == ZK_ERR_ARG
