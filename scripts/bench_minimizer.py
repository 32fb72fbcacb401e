"""usage (GPU box): python3 scripts/bench_minimizer.py [--sizes 64,1024] [--iterations K] [--precision mixed|double]
The device-resident minimiser (kernels_minimize.h) on the 975-atom toluene box with the ligand and its 60 nearest
atoms mobile, mobile atoms jittered by 0.01 nm (case 3 of tests/test_gpu_minimizer.py):
  lone    wall time per iteration and iterations to tolerance 10 kJ/mol/nm of Simulation.minimizeEnergy(method="host") against
          method="device"; kernel launches per device iteration (NativeEngine.stats) beside those of one get_forces();
  batch   NativeBatch.minimize_all at every R of --sizes: K iterations (tolerance out of reach), wall time per iteration.
Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from blues_amd import build, integrators, systems  # noqa: E402

LIG = np.arange(15)
FUNCS = {"lambda_sterics": "1 - 0.3*sin(3.141592653589793*lambda)", "lambda_electrostatics": "1 - 0.5*sin(3.141592653589793*lambda)"}


def integ(seed=7):
    return integrators.AlchemicalExternalLangevinIntegrator(FUNCS, splitting="H V R O R V H", temperature=300.0, timestep=0.002,
                                                            constraint_tolerance=1e-10, nsteps_neq=20, seed=seed)


def case3():
    s, v = systems.toluene_box()
    near = systems.nearest_molecules(s, LIG, 60, exclude_idx=LIG)
    return systems.freeze_except(s, np.concatenate([LIG, near])), v


def jittered(s, seed):
    mob = np.asarray(s.mass) > 0
    x = np.array(s.positions, dtype=np.float64)
    x[mob] += 0.01 * np.random.RandomState(seed).uniform(-1.0, 1.0, (int(mob.sum()), 3))
    return x


def lone(precision):
    from blues_amd.context import Simulation
    s, _ = case3()
    out = {}
    for method in ("host", "device"):
        sim = Simulation(None, s, integ(), precision=precision)
        e = sim.context._engine
        e.set_positions(jittered(s, 1))
        e.get_forces()
        l0 = e.stats()["kernel_launches"]; e.get_forces(); per_pass = e.stats()["kernel_launches"] - l0
        e.set_positions(jittered(s, 1)); e.potential_energy()
        st0 = e.stats()
        t0 = time.perf_counter()
        r = sim.minimizeEnergy(10.0, 3000 if method == "device" else 0, method=method)
        e.get_positions()
        sec = time.perf_counter() - t0
        st1 = e.stats()
        passes = st1["force_passes"] - st0["force_passes"]
        f = e.get_forces()
        row = {"seconds": sec, "kernel_launches": st1["kernel_launches"] - st0["kernel_launches"], "e_final": e.potential_energy(),
               "raw_fmax_mobile": float(np.abs(f[np.asarray(s.mass) > 0]).max()), "launches_per_get_forces": per_pass}
        if method == "device":
            row.update(result=r, iterations=r["iterations"], us_per_iteration=1e6 * sec / max(1, r["iterations"] + 1),
                       launches_per_iteration=(st1["kernel_launches"] - st0["kernel_launches"]) / float(r["iterations"] + 1))
        else:   # (the host loop: every iteration is set_positions + an energy evaluation, accepted ones add a get_forces)
            evals = st1["own_energy_evaluations"] - st0["own_energy_evaluations"]
            row.update(energy_evaluations=evals, us_per_iteration=1e6 * sec / max(1, evals))
        out[method] = row
        e.close()
    return out


def batch(R, iterations, precision):
    from blues_amd.engine import NativeBatch, NativeEngine
    s, _ = case3()
    prec = 1 if precision == "double" else 0
    engs = []
    for r in range(R):
        e = NativeEngine(s, integ(seed=100 + r).to_data(precision=prec, replica=r))
        e.set_positions(jittered(s, 10 + r))
        engs.append(e)
    b = NativeBatch(engs)
    b.minimize_all(1e-9, 16)          # warm-up: layouts, lists, buffers
    engs[0].get_positions()
    l0 = engs[0].stats()["kernel_launches"]
    t0 = time.perf_counter()
    _, res = b.minimize_all(1e-9, iterations)
    engs[0].get_positions()
    sec = time.perf_counter() - t0
    st = b.stats()
    out = {"R": R, "iterations": iterations, "seconds": sec, "us_per_iteration": 1e6 * sec / (iterations + 1),
           "launches_per_iteration_leader": (engs[0].stats()["kernel_launches"] - l0) / float(iterations + 1),
           "lockstep_steps": st["lockstep_steps"], "fallback_steps": st["fallback_steps"], "fmax_member0": res[0]["fmax"]}
    b.close()
    for e in engs:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--precision", default="mixed", choices=("mixed", "double"))
    a = ap.parse_args()
    build.build_engine()
    out = {"bench": "minimizer", "source_sha": build.source_sha(), "precision": a.precision, "lone": lone(a.precision),
           "batch": [batch(int(R), a.iterations, a.precision) for R in a.sizes.split(",") if R]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
