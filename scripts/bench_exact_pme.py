"""usage (GPU box): python3 scripts/bench_exact_pme.py [--mode cost|bits] [--R N] [--steps K] [--warmup W] [--repeats N] [--treatments a,b] [--label NAME]
The 'exact' alchemical PME treatment (SystemData.alchemical_pme_treatment; kernels_pme.h: k_pme_exact_fast_b in mixed precision) against 'direct-space'.

--mode cost (default): R chains (1024) of the S23k frozen System with reciprocal space (mesh 18 x 27 x 36), mixed precision, stepped
through NativeBatch; each treatment in --treatments is timed --repeats times after one warm-up, all in this process, and ONE JSON line
reports every repeat's us_per_step, the medians and the ratio exact / direct-space.  For the mesh kernels' own durations run this
script under `rocprofv3 --kernel-trace --stats` (a run of its own) and read k_pme_exact_fast_b / k_pme_fast_b.

--mode bits: the fixed 45-step switch of the default periodic toluene box DESIGN.md records (generateNCMCIntegrator(nstepsNC=45,
dt=0.002, temperature=300, seed=7), the fixture's velocities; 3 steps, then 42 with the launches counted), both precisions: the bits of
protocol_work and the launches per 42 steps.  BLUES_LIB_PATH points the loader at another build (the parent's) for the comparison."""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from blues_amd import build, integrators, systems  # noqa: E402

DT = 0.002
LABEL = "this commit"   # --label: what the record calls the library under test (never the loader's path)


def bits():
    from blues_amd.engine import NativeEngine
    s, v = systems.toluene_box()
    out = {"mode": "bits", "library": LABEL}
    for name, precision in (("mixed", 0), ("double", 1)):
        e = NativeEngine(s, integrators.generateNCMCIntegrator(nstepsNC=45, dt=DT, temperature=300.0, seed=7).to_data(precision=precision))
        e.set_velocities(v)
        e.step(3)
        l0 = e.stats()["kernel_launches"]
        e.step(42)
        out[name] = {"protocol_work_bits": struct.pack(">d", e.get_global("protocol_work")).hex(), "launches_per_42_steps": int(e.stats()["kernel_launches"] - l0)}
        e.close()
    return out


def cost(R, steps, warmup, repeats, treatments):
    from blues_amd.engine import NativeBatch, NativeEngine
    base, v = systems.s23k(mobile_atoms=275, frozen=True)
    base = systems.with_reciprocal_space(base)
    out = {"mode": "cost", "library": LABEL, "R": R, "steps": steps, "repeats": repeats, "atoms": base.n_atoms,
           "pme_grid": list(base.pme_grid), "treatments": {}}
    for tr in treatments:
        s = systems.with_alchemical_pme_treatment(base, tr)
        nsteps_nc = warmup + repeats * steps   # (one switch covers the measurement: no switch end in the timed steps)
        engs = []
        for r in range(R):
            d = integrators.generateNCMCIntegrator(nstepsNC=nsteps_nc, dt=DT, temperature=300.0, seed=100 + r).to_data(precision=0, replica=r)
            e = NativeEngine(s, d)
            e.set_velocities(v * (1.0 + 0.0001 * r))
            engs.append(e)
        b = NativeBatch(engs)
        b.step(warmup)
        engs[0].get_positions()   # (synchronises)
        l0 = engs[0].stats()["kernel_launches"]
        us = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            b.step(steps)
            engs[0].get_positions()
            us.append(1e6 * (time.perf_counter() - t0) / steps)
        st = b.stats()
        out["treatments"][tr] = {"us_per_step": us, "us_per_step_median": float(np.median(us)), "us_per_step_min": min(us), "us_per_step_max": max(us),
                                 "launches_per_step_leader": (engs[0].stats()["kernel_launches"] - l0) / float(repeats * steps),
                                 "lockstep_steps": st["lockstep_steps"], "fallback_steps": st["fallback_steps"],
                                 "protocol_work_chain0": engs[0].get_global("protocol_work"),
                                 "exact_pme_fast_launches": engs[0].stats()["exact_pme_fast_launches"], "exact_pme_general_launches": engs[0].stats()["exact_pme_general_launches"]}
        b.close()
        for e in engs:
            e.close()
    t = out["treatments"]
    if "exact" in t and "direct-space" in t:
        out["ratio_exact_over_direct_space"] = t["exact"]["us_per_step_median"] / t["direct-space"]["us_per_step_median"]
    return out


def main():
    global LABEL
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="cost", choices=("cost", "bits"))
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--treatments", default="direct-space,exact")
    ap.add_argument("--label", default=LABEL, help="name of the build in the record, e.g. 'parent build (<commit>)' with BLUES_LIB_PATH set")
    a = ap.parse_args()
    LABEL = a.label
    build.build_engine()
    print(json.dumps(bits() if a.mode == "bits" else cost(a.R, a.steps, a.warmup, a.repeats, a.treatments.split(","))))


if __name__ == "__main__":
    main()
