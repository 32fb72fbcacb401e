"""usage (GPU box): python3 scripts/bench_nocutoff.py [--steps K] [--only NAME:R,...]
NoCutoff (vacuum) stepping through NativeBatch: NCMC switch steps of the reference's RandomLigandRotationMove test System
(blues/tests/test_randomrotation.py: TOL-parm, NoCutoff, HBonds, dt 2 fs, alchemical atoms 0-14) at R = 1, 64, 256, 1024 and of
vacDivaline (alchemical atoms 22-31, the side chain SideChainMove(struct, [1]) selects) at R = 1024.  Prints ONE JSON line: ns/day
per configuration (R chains x simulated time per wall-clock time) and the environment pairs the all-pairs kernel evaluates per step
(pairs_per_step: each pair of a mobile environment atom with every atom, from both ends; divide by the kernel's time from a
`rocprofv3 --kernel-trace --stats` run of this script for the achieved pair rate).
--only ethylene:R runs the reference's known-answer System (tests/ethylene.py: 8 atoms, custom pair form + centroid bond, dt 1 fs,
200 K) instead: its environment atoms are frozen and the all-pairs kernel is not launched (pairs_per_step 0)."""
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
DEFAULT = [("TOL-parm", 1), ("TOL-parm", 64), ("TOL-parm", 256), ("TOL-parm", 1024), ("vacDivaline", 1024)]
DT = 0.002


def nocutoff_system(name):
    g = os.path.join(ROOT, "tests", "golden")
    prm = amber.read_prmtop(os.path.join(g, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(g, name + ".inpcrd"))
    return amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=SYSTEMS[name], nonbonded_method="NoCutoff")


def run(name, R, steps, warmup, nsteps_nc):
    from blues_amd.engine import NativeBatch, NativeEngine
    custom = name == "ethylene"
    if custom:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import ethylene
        s, proto = ethylene.load()
    else:
        s = nocutoff_system(name)
    dt, temperature = (proto["dt"], proto["temperature"]) if custom else (DT, 300.0)
    rng = np.random.RandomState(7)
    engs = []
    for r in range(R):
        d = integrators.generateNCMCIntegrator(nstepsNC=nsteps_nc, dt=dt, temperature=temperature, seed=100 + r).to_data(precision=0, replica=r)
        e = NativeEngine(s, d)
        e.set_velocities(0.3 * rng.standard_normal((s.n_atoms, 3)) * (s.mass[:, None] > 0))
        engs.append(e)
    b = NativeBatch(engs)
    b.step(warmup)
    engs[0].get_positions()   # (synchronises)
    t0 = time.perf_counter()
    b.step(steps)
    engs[0].get_positions()
    sec = time.perf_counter() - t0
    st = b.stats()
    mobile_env = int(((s.mass > 0) & ~np.isin(np.arange(s.n_atoms), s.alchemical_atoms)).sum())
    out = {"system": name, "R": R, "atoms": s.n_atoms, "steps": steps, "us_per_step": 1e6 * sec / steps,
           "ns_per_day": R * steps * dt * 1e-3 / sec * 86400.0, "pairs_per_step": 0 if custom else R * mobile_env * s.n_atoms, "dt_ps": dt,   # (each result carries its own timestep)
           "lockstep_steps": st["lockstep_steps"], "fallback_steps": st["fallback_steps"], "nonbonded_kernel": engs[0].stats()["nonbonded_kernel"]}
    b.close()
    for e in engs:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="", help="comma-separated NAME:R configurations instead of the default five")
    a = ap.parse_args()
    build.build_engine()
    cfgs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.only.split(",")] if a.only else DEFAULT
    nsteps_nc = a.steps + a.warmup   # (one switch covers the measurement: no switch end in the timed steps)
    res = [run(n, R, a.steps, a.warmup, nsteps_nc) for n, R in cfgs]
    out = {"metric": "NoCutoff NCMC ns/day through NativeBatch (mixed precision)", "unit": "ns/day", "results": res}
    if all(r["dt_ps"] == DT for r in res):   # (the ethylene workload steps at its own 1 fs: every result carries its dt_ps)
        out = {"metric": out["metric"], "unit": "ns/day", "dt_ps": DT, "results": res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
