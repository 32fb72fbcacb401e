"""usage (GPU box): python3 scripts/bench_lj_switch.py [--replicas R] [--reps N] [--steps K] [--switch 0.8]
What the Lennard-Jones switching function costs on the S23k batch (mixed precision, mostly frozen: the per-atom-list
kernel and the fp32 dense alchemical kernel, bench.py's path), with and without a switch on the same System:
  blues_batch_time_nonbonded   the batch's nonbonded launch (pruned lists current / re-derived, weighted by the batch's own history)
  blues_time_nonbonded         the same kernel of ONE chain laid out as a member of such a batch (BluesTuning.assume_batch)
  us / step                    NCMC steps through NativeBatch, median of --repeats timed blocks
and the pairs inside the cutoff / inside the shell of one chain's i-atoms, from which the per-pair figure is formed.
Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from blues_amd import build, integrators, systems, tuning  # noqa: E402


def measure(s, v, R, reps, steps, repeats):
    from blues_amd.engine import NativeBatch, NativeEngine
    nsteps_nc = 20 + repeats * steps
    engs = []
    for r in range(R):
        d = integrators.generateNCMCIntegrator(nstepsNC=nsteps_nc, dt=0.004, temperature=300.0, seed=100 + r).to_data(precision=0, replica=r)
        e = NativeEngine(s, d); e.set_velocities(v); engs.append(e)
    b = NativeBatch(engs)
    b.step(20)
    engs[0].get_positions()
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        b.step(steps)
        engs[0].get_positions()
        us.append(1e6 * (time.perf_counter() - t0) / steps)
    modes = [b.time_nonbonded_modes(reps) for _ in range(3)]
    batch_nb = [b.time_nonbonded(reps) for _ in range(3)]
    st = engs[0].stats()
    out = {"us_per_step": us, "us_per_step_median": float(np.median(us)), "batch_time_nonbonded_us": batch_nb,
           "batch_pruned_current_us": [m[0] for m in modes], "batch_pruning_pass_us": [m[1] for m in modes], "prune_fraction": modes[-1][2],
           "nonbonded_kernel": st["nonbonded_kernel"], "alchemical_kernel": st["alchemical_kernel"], "lj_switch": list(engs[0].lj_switch()),
           "fallback_steps": b.stats()["fallback_steps"]}
    b.close()
    for e in engs:
        e.close()
    saved = tuning.current()
    tuning.set(assume_batch=max(R, 1024))
    try:
        e = NativeEngine(s, integrators.generateNCMCIntegrator(nstepsNC=20, dt=0.004, temperature=300.0, seed=1).to_data(precision=0))
        out["lone_time_nonbonded_us"] = [e.time_nonbonded(reps) for _ in range(3)]
        e.close()
    finally:
        tuning._apply(saved)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--switch", type=float, default=0.8)
    a = ap.parse_args()
    build.build_engine()
    s, v = systems.s23k(275, frozen=True)
    # pairs one chain's nonbonded kernel evaluates inside the cutoff, and those of them in the shell (mobile non-alchemical i-atoms)
    x = np.asarray(s.positions); box = np.asarray(s.box, dtype=np.float64)
    alch = np.zeros(s.n_atoms, bool); alch[np.asarray(s.alchemical_atoms)] = True
    n_in = n_shell = 0
    for i in np.nonzero((s.mass > 0) & ~alch)[0]:
        d = x[~alch] - x[i]; d -= box * np.rint(d / box); r2 = (d * d).sum(1)
        n_in += int(((r2 < s.cutoff ** 2) & (r2 > 0)).sum()); n_shell += int(((r2 < s.cutoff ** 2) & (r2 > a.switch ** 2)).sum())
    res = {"metric": "cost of the Lennard-Jones switching function on the S23k batch (mixed precision)", "replicas": a.replicas, "reps": a.reps,
           "switch_distance": a.switch, "cutoff": float(s.cutoff), "pairs_in_cutoff_per_chain": n_in, "pairs_in_shell_per_chain": n_shell,
           "without": measure(s, v, a.replicas, a.reps, a.steps, a.repeats),
           "with": measure(systems.with_switch_distance(s, a.switch), v, a.replicas, a.reps, a.steps, a.repeats)}
    w, wo = res["with"], res["without"]
    res["batch_time_nonbonded_ratio"] = float(np.median(w["batch_time_nonbonded_us"]) / np.median(wo["batch_time_nonbonded_us"]))
    res["lone_time_nonbonded_ratio"] = float(np.median(w["lone_time_nonbonded_us"]) / np.median(wo["lone_time_nonbonded_us"]))
    res["us_per_step_ratio"] = w["us_per_step_median"] / wo["us_per_step_median"]
    res["extra_ns_per_pair_in_cutoff"] = 1e3 * (np.median(w["batch_time_nonbonded_us"]) - np.median(wo["batch_time_nonbonded_us"])) / (a.replicas * n_in) if n_in else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
