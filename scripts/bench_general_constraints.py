"""Cost of general constraint clusters (profiles/general_constraints): the mostly-frozen toluene box as a batch of R chains,
mixed precision.  python scripts/bench_general_constraints.py {hb|hb_interp|ab|ha} [--R 1024] [--steps 100] [--warmup 20] prints one JSON line:
us per step, kernel launches per step and, with a library built with -DBLUES_GEN_SWEEPS (BLUES_LIB_PATH), the sweeps per SHAKE."""
import argparse, copy, ctypes, json, os, sys, time
ap = argparse.ArgumentParser(); ap.add_argument("variant"); ap.add_argument("--R", type=int, default=1024); ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--root", default=os.getcwd()); a = ap.parse_args()
sys.path.insert(0, a.root)
import numpy as np
from blues_amd import integrators, systems, tuning
from blues_amd.engine import NativeEngine, NativeBatch
LIG = np.arange(15)
def general_ligand(s, hangles):
    s = copy.copy(s); ba, bp = np.asarray(s.bond_atoms), np.asarray(s.bond_params)
    m = np.isin(ba[:, 0], LIG) & np.isin(ba[:, 1], LIG)
    ca = [tuple(int(q) for q in p) for p in np.asarray(s.constraint_atoms)]; cd = [float(d) for d in np.asarray(s.constraint_dist)]
    for (i, j), (r0, _) in zip(ba[m], bp[m]): ca.append((int(i), int(j))); cd.append(float(r0))
    s.bond_atoms, s.bond_params = ba[~m], bp[~m]
    if hangles:
        dist = {frozenset(p): d for p, d in zip(ca, cd)}; aa, ap_ = np.asarray(s.angle_atoms), np.asarray(s.angle_params); keep = np.ones(len(aa), bool)
        for q, ((i, j, k), (th0, _)) in enumerate(zip(aa, ap_)):
            if i in LIG and k in LIG and s.mass[i] < 4 and s.mass[k] < 4:
                d1, d2 = dist[frozenset((int(i), int(j)))], dist[frozenset((int(k), int(j)))]
                ca.append((int(i), int(k))); cd.append(float(np.sqrt(d1 * d1 + d2 * d2 - 2 * d1 * d2 * np.cos(th0)))); keep[q] = False
        s.angle_atoms, s.angle_params = aa[keep], ap_[keep]
    s.constraint_atoms = np.array(ca, dtype=np.int32).reshape(-1, 2); s.constraint_dist = np.array(cd); return s
s0, v0 = systems.toluene_box()
s = {"hb": s0, "hb_interp": s0, "ab": None, "ha": None}[a.variant]
if s is None: s = general_ligand(s0, a.variant == "ha")
near = systems.nearest_molecules(s, LIG, 60, exclude_idx=LIG); s = systems.freeze_except(s, np.concatenate([LIG, near]))
tuning.set(assume_batch=a.R, **({"fast_step": 0} if a.variant == "hb_interp" else {}))
n = a.steps + a.warmup
engs = []
for r in range(a.R):
    it = integrators.generateNCMCIntegrator(nstepsNC=n + 50, dt=0.002, temperature=300.0, seed=40 + r)
    e = NativeEngine(s, it.to_data(precision=0, replica=r)); e.set_velocities(v0 * (1.0 + 1e-4 * r)); engs.append(e)
B = NativeBatch(engs)
B.step(a.warmup); engs[0].get_global("protocol_work")
k0 = engs[0].stats()["kernel_launches"]
t0 = time.perf_counter(); B.step(a.steps); w = engs[0].get_global("protocol_work"); t1 = time.perf_counter()
out = {"variant": a.variant, "R": a.R, "steps": a.steps, "us_per_step": 1e6 * (t1 - t0) / a.steps, "launches_per_step": (engs[0].stats()["kernel_launches"] - k0) / a.steps,
       "protocol_work_member0": w, "step_threads": engs[0].stats()["step_threads"], "batch": {k: int(v) for k, v in B.stats().items() if "steps" in k}}
from blues_amd import _lib
lib = _lib.load()
if hasattr(lib, "blues_debug_gen_sweeps"):
    c = (ctypes.c_ulonglong * 3)(); lib.blues_debug_gen_sweeps(c)
    out["shake_calls"], out["sweeps_total"], out["sweeps_max"] = int(c[0]), int(c[1]), int(c[2]); out["sweeps_mean"] = c[1] / max(1, c[0])
print(json.dumps(out), flush=True)
B.close(); [e.close() for e in engs]
