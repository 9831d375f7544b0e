"""zk_pk_derive_eval_h measured: what deriving the tables of H over coset values costs a key that was loaded, and what its proofs
gain.  Mul-chain keys filling their domain.  For every size a SEQUENCE of fresh processes, one per configuration, in rotating order:

    setup     the key from zk_groth16_setup (tables from the trapdoor)
    loaded    that key serialised, freed and read back with zk_pk_deserialize: the old witness map
    derived   the same, then zk_pk_derive_eval_h: wall time, its phases (the context's "derive.*" timers), device memory
              before / peak / after (hipMemGetInfo sampled from a thread while the call runs)

each timing `--reps` passes over four assignments (create_proof_dev, every call announcing the next assignment) after two warm-up
passes, and hashing the proofs: the three configurations must give the same bytes.  Every child runs under its own `timeout`; the
first child that fails or runs out of time ends the run.  One JSON line per child and one summary line per size (median per-proof
times, gain, break-even number of proofs), on stdout and appended to --out.

    python tools/bench_derive_eval_h.py [--sizes 16,18,20] [--rounds 2] [--reps 6] [--out profiles/derive_eval_h.jsonl]

The butterfly kernel's time per level comes from one run of its own, no counters in it:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_derive_eval_h.py --child derived --log 20 --reps 0
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("setup", "loaded", "derived")


class MemWatch:
    """used device memory (MB) sampled while a call runs: hipMemGetInfo from a thread (ctypes releases the GIL during the call)"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.peak = 0.0
        self._stop = threading.Event()

    def used(self):
        free, total = C.c_size_t(), C.c_size_t()
        return (total.value - free.value) / 1e6 if self.hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 else 0.0

    def __enter__(self):
        def run():
            while not self._stop.is_set():
                self.peak = max(self.peak, self.used())
                time.sleep(0.005)
        self.t = threading.Thread(target=run, daemon=True)
        self.t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self.t.join()


def child(mode, log_n, reps):
    import numpy as np
    import zk_mpc_amd as Z
    import zk_mpc_amd.convert as cv
    import zk_mpc_amd.serialize as S
    rs = np.random.RandomState(2025)
    mont = lambda: cv.fr_to_mont([int.from_bytes(rs.bytes(31), "little")])[0]
    ctx = Z.Context(0)
    n = (1 << log_n) - 2
    rec = {"mode": mode, "log_n": log_n, "constraints": n}
    dr = ctx.r1cs_mul_chain(n)
    td = [mont() for _ in range(7)]
    zs = [ctx.mul_chain_assignment_dev(n, mont(), mont()) for _ in range(4)]
    rl, sl = [mont() for _ in range(4)], [mont() for _ in range(4)]
    t0 = time.perf_counter()
    pk = ctx.groth16_setup(dr, *td)
    rec["setup_s"] = round(time.perf_counter() - t0, 3)
    mem = MemWatch()
    if mode != "setup":
        data = S.proving_key_bytes(ctx, pk, False)
        pk.free()
        rec["key_bytes"] = len(data)
        t0 = time.perf_counter()
        pk, _, _ = S.proving_key_from_bytes(ctx, data, compressed=False)
        rec["deserialize_s"] = round(time.perf_counter() - t0, 3)
        del data
        assert not pk.eval_h(dr)
    if mode == "derived":
        ctx.set_profiling(True)
        rec["mem_before_mb"] = round(mem.used())
        with mem:
            t0 = time.perf_counter()
            pk.derive_eval_h(dr)
            rec["derive_s"] = round(time.perf_counter() - t0, 3)
        rec["mem_peak_mb"], rec["mem_after_mb"] = round(mem.peak), round(mem.used())
        rec["derive_phases_ms"] = {k[7:]: round(v[0], 1) for k, v in ctx.timers().items() if k.startswith("derive.")}
        ctx.set_profiling(False)
    rec["eval_h"] = bool(pk.eval_h(dr))
    rec["mem_key_mb"] = round(mem.used())
    assert rec["eval_h"] == (mode != "loaded")

    def one_pass():
        out = []
        for k in range(4):
            ctx.groth16_hint_next_dev(zs[(k + 1) & 3].ptr if k < 3 else None)
            out.append(ctx.create_proof_dev(pk, dr, zs[k].ptr, rl[k], sl[k]))
        return out

    if reps:
        want = one_pass()
        assert one_pass() == want
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = one_pass()
            ts.append((time.perf_counter() - t0) * 1e3 / 4)
            assert got == want
        rec["proof_ms"] = [round(t, 4) for t in ts]
        rec["proof_ms_median"] = round(float(np.median(ts)), 4)
        rec["proofs_sha"] = hashlib.sha256(b"".join(want)).hexdigest()[:16]
    pk.free(); dr.free()
    ctx.close()
    print("DERIVE_BENCH " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,18,20")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--child", choices=MODES)
    ap.add_argument("--log", type=int, default=16)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derive_eval_h.jsonl"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.log, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")

    for log_n in [int(x) for x in a.sizes.split(",")]:
        recs = {m: [] for m in MODES}
        for rnd in range(a.rounds):
            for i in range(3):
                mode = MODES[(i + rnd) % 3]
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--log", str(log_n),
                       "--reps", str(a.reps)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in r.stdout.splitlines() if l.startswith("DERIVE_BENCH ")]
                if r.returncode != 0 or not line:
                    emit({"log_n": log_n, "mode": mode, "round": rnd, "failed": r.returncode, "stderr": r.stderr[-1500:]})
                    sys.exit("the %s child at 2^%d ended with status %d: stopping" % (mode, log_n, r.returncode))
                rec = json.loads(line[-1][len("DERIVE_BENCH "):])
                rec["round"] = rnd
                emit(rec)
                recs[mode].append(rec)
        import numpy as np
        med = {m: float(np.median([t for r in recs[m] for t in r["proof_ms"]])) for m in MODES}
        spread = {m: [r["proof_ms_median"] for r in recs[m]] for m in MODES}
        assert len({r["proofs_sha"] for m in MODES for r in recs[m]}) == 1, "the configurations disagree on the proof bytes"
        d = recs["derived"]
        gain = med["loaded"] - med["derived"]
        derive_s = float(np.median([r["derive_s"] for r in d]))
        emit({"summary": True, "log_n": log_n, "proof_ms_median": {m: round(med[m], 4) for m in MODES}, "proof_ms_by_child": spread,
              "gain_ms": round(gain, 4), "derive_s": derive_s, "deserialize_s": float(np.median([r["deserialize_s"] for r in d + recs["loaded"]])),
              "break_even_proofs": round(derive_s * 1e3 / gain) if gain > 0 else None, "derive_phases_ms": d[-1]["derive_phases_ms"],
              "mem_before_mb": d[-1]["mem_before_mb"], "mem_peak_mb": d[-1]["mem_peak_mb"], "mem_after_mb": d[-1]["mem_after_mb"],
              "mem_setup_key_mb": recs["setup"][-1]["mem_key_mb"], "proofs_equal": True})


if __name__ == "__main__":
    main()
