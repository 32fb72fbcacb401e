"""usage (GPU box): python3 scripts/bench_implicit_solvent.py [--steps K] [--warmup W] [--repeats N] [--only NAME:R,...] [--model OBC2|OBC1|none]
NoCutoff NCMC stepping with GB-OBC implicit solvent (kernels_gb.h) through NativeBatch, modelled on scripts/bench_nocutoff.py: the
975-atom TOL-parm cluster (alchemical atoms 0-14, HBonds, dt 2 fs, mixed precision) as a lone chain and at R = 1024.  --model none
steps the same Systems without implicit solvent (what scripts/bench_nocutoff.py measures) in the same process, for the ratio
GB step / plain step.  Each configuration is timed --repeats times after one warm-up; prints ONE JSON line with every repeat's
us_per_step, their median and spread, and the pairs each GB kernel evaluates per step (every atom with every other atom, from both
ends: R n (n - 1); divide by the kernel's time from a `rocprofv3 --kernel-trace --stats` run of this script for the pair rate)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from blues_amd import amber, build, integrators  # noqa: E402

SYSTEMS = {"TOL-parm": list(range(15)), "vacDivaline": list(range(22, 32))}
DEFAULT = [("TOL-parm", 1), ("TOL-parm", 1024)]
DT = 0.002


def gb_system(name, model):
    g = os.path.join(ROOT, "tests", "golden")
    prm = amber.read_prmtop(os.path.join(g, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(g, name + ".inpcrd"))
    return amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=SYSTEMS[name], nonbonded_method="NoCutoff",
                                   implicit_solvent=None if model == "none" else model)


def run(name, R, model, steps, warmup, repeats):
    from blues_amd.engine import NativeBatch, NativeEngine
    s = gb_system(name, model)
    nsteps_nc = warmup + repeats * steps   # (one switch covers the measurement: no switch end in the timed steps)
    rng = np.random.RandomState(7)
    engs = []
    for r in range(R):
        d = integrators.generateNCMCIntegrator(nstepsNC=nsteps_nc, dt=DT, temperature=300.0, seed=100 + r).to_data(precision=0, replica=r)
        e = NativeEngine(s, d)
        e.set_velocities(0.3 * rng.standard_normal((s.n_atoms, 3)) * (s.mass[:, None] > 0))
        engs.append(e)
    b = NativeBatch(engs)
    b.step(warmup)
    engs[0].get_positions()   # (synchronises)
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        b.step(steps)
        engs[0].get_positions()
        us.append(1e6 * (time.perf_counter() - t0) / steps)
    st = b.stats()
    out = {"system": name, "R": R, "model": model, "atoms": s.n_atoms, "steps": steps, "repeats": repeats, "us_per_step": us,
           "us_per_step_median": float(np.median(us)), "us_per_step_min": min(us), "us_per_step_max": max(us),
           "ns_per_day_median": R * DT * 1e-3 / (float(np.median(us)) * 1e-6) * 86400.0,
           "gb_pairs_per_kernel_per_step": 0 if model == "none" else R * s.n_atoms * (s.n_atoms - 1),
           "lockstep_steps": st["lockstep_steps"], "fallback_steps": st["fallback_steps"]}
    b.close()
    for e in engs:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated NAME:R configurations instead of TOL-parm:1,TOL-parm:1024")
    ap.add_argument("--model", default="OBC2,none", help="comma-separated: OBC2, OBC1, none (the plain NoCutoff System)")
    a = ap.parse_args()
    build.build_engine()
    cfgs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.only.split(",")] if a.only else DEFAULT
    res = [run(n, R, m, a.steps, a.warmup, a.repeats) for n, R in cfgs for m in a.model.split(",")]
    ratios = {}
    for n, R in cfgs:
        by = {r["model"]: r["us_per_step_median"] for r in res if r["system"] == n and r["R"] == R}
        if "none" in by:
            ratios["%s:%d" % (n, R)] = {m: by[m] / by["none"] for m in by if m != "none"}
    print(json.dumps({"metric": "NoCutoff NCMC step with GB-OBC implicit solvent through NativeBatch (mixed precision)", "unit": "us/step", "dt_ps": DT,
                      "results": res, "gb_over_plain": ratios}))


if __name__ == "__main__":
    main()
