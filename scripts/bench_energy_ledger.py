"""usage (GPU box): python3 scripts/bench_energy_ledger.py [--R N] [--steps K] [--warmup W] [--modes off,on]
Cost of the energy ledger (measure_shadow_work / measure_heat) on the flagship workload: NCMC switch steps of the S23k
System (23,400 atoms, 275 mobile, `systems.s23k()`, "H V R O R V H" at 4 fs, mixed precision) through NativeBatch, with the ledger off
and on, on the same build.  Prints ONE JSON line: microseconds per step and kernel launches per step (blues_get_stats [2] of member 0,
the batch's leader) for each mode, and the on / off ratio.  Run it under `rocprofv3 --kernel-trace --stats -- python3 ...` with
`--modes on` for the kernel table."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from blues_amd import build, integrators, systems, tuning  # noqa: E402

DT = 0.004


def run(measure, R, steps, warmup):
    from blues_amd.engine import NativeBatch, NativeEngine
    s, v = systems.s23k()
    rng = np.random.RandomState(7)
    engs = []
    for r in range(R):
        d = integrators.generateNCMCIntegrator(nstepsNC=steps + warmup, dt=DT, temperature=300.0, seed=100 + r,
                                               measure_shadow_work=measure).to_data(precision=0, replica=r)
        e = NativeEngine(s, d)
        e.set_velocities(v * (1.0 + 0.02 * rng.standard_normal(v.shape)))
        engs.append(e)
    b = NativeBatch(engs)
    b.step(warmup)
    engs[0].get_positions()   # (synchronises)
    l0 = engs[0].stats()["kernel_launches"]
    t0 = time.perf_counter()
    b.step(steps)
    engs[0].get_positions()
    sec = time.perf_counter() - t0
    st = b.stats()
    out = {"ledger": bool(measure), "R": R, "steps": steps, "us_per_step": 1e6 * sec / steps, "ns_per_day": R * steps * DT * 1e-3 / sec * 86400.0,
           "launches_per_step": (engs[0].stats()["kernel_launches"] - l0) / steps, "lockstep_steps": st["lockstep_steps"], "fallback_steps": st["fallback_steps"],
           "shadow_work_member0": engs[0].get_global("shadow_work"), "heat_member0": engs[0].get_global("heat"),
           "protocol_work_member0": engs[0].get_global("protocol_work")}
    b.close()
    for e in engs:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--modes", default="off,on")
    a = ap.parse_args()
    build.build_engine()
    tuning.set(assume_batch=a.R)
    res = [run(m == "on", a.R, a.steps, a.warmup) for m in a.modes.split(",")]
    out = {"metric": "S23k NCMC switch through NativeBatch, energy ledger off / on (mixed precision)", "unit": "us/step", "dt_ps": DT, "results": res}
    by = {r["ledger"]: r for r in res}
    if True in by and False in by:
        out["on_over_off"] = by[True]["us_per_step"] / by[False]["us_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
