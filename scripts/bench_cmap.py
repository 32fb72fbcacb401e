"""usage (GPU box): python3 scripts/bench_cmap.py [--steps K] [--warmup W] [--repeats N] [--only NAME:R,...] [--maps with,without]
NCMC stepping with and without CMAP torsion correction maps (kernels_bonded.h: T_CMAP) through NativeBatch, in the manner of
scripts/bench_implicit_solvent.py, mixed precision, dt 2 fs:
  s23k_solute at R = 64    the freeze_radius workload (285 mobile solute atoms, water frozen, full PME off: the direct-space box of
                           bench.py --workload rotmove-solute) with a SYNTHETIC assignment -- the box has no protein: every one of
                           its 19 toluenes gets one CMAP torsion over five bonded ring carbons and a 24 x 24 map of its own;
  vacDivaline at R = 1024  the 35-atom NoCutoff dipeptide with one 24 x 24 map on its backbone C-N-CA-C-OXT.
Each configuration is timed --repeats times after one warm-up; prints ONE JSON line with every repeat's us_per_step, their median,
the counts of torsions and bonded entries, and the ratio with / without.  The bonded kernel's own duration comes from a
`rocprofv3 --kernel-trace --stats` run of this script (k_bonded_entries_b<true, true> against k_bonded_entries_b<false, false>).

--mode bits: the two fixed 45-step switches DESIGN.md 4i records, of Systems WITHOUT maps (generateNCMCIntegrator(nstepsNC=45, dt=0.002,
temperature=300, seed=7); 3 steps, then 42 with the launches counted; both precisions): the plain NoCutoff TOL-parm System from
velocities 0.3 N(0, 1) of RandomState(7) and the default periodic toluene box from the fixture's velocities -- the bits of
protocol_work and the launches per 42 steps.  BLUES_LIB_PATH points the loader at another build (the parent's) for the comparison."""
import argparse
import dataclasses
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from blues_amd import amber, build, integrators, systems  # noqa: E402

DEFAULT = [("s23k_solute", 64), ("vacDivaline", 1024)]
DT = 0.002
TWO_PI = 2.0 * np.pi


def smooth_map(n, k):
    g = np.arange(n) * TWO_PI / n
    p, s = g[:, None], g[None, :]
    return (1.0 + 0.1 * k) * (4.0 * np.cos(p) + 2.0 * np.sin(2.0 * s) + 3.0 * np.cos(p - s + 0.4))


def bonded_path(s, atoms, length=5):
    """`length` of `atoms` joined in a row by harmonic bonds (heavy atoms: the bonds to hydrogen are constraints)"""
    atoms = set(int(a) for a in atoms)
    nb = {}
    for a, b in np.asarray(s.bond_atoms):
        if int(a) in atoms and int(b) in atoms:
            nb.setdefault(int(a), []).append(int(b)); nb.setdefault(int(b), []).append(int(a))

    def walk(path):
        if len(path) == length:
            return path
        for q in nb.get(path[-1], []):
            if q not in path:
                out = walk(path + [q])
                if out:
                    return out
        return None
    for first in sorted(nb):
        p = walk([first])
        if p:
            return p
    return None


def system(name, with_maps):
    if name == "s23k_solute":
        s, v = systems.s23k_solute(frozen=True)
        if with_maps:      # synthetic: one torsion and one map per toluene (residues 0..18 of the box are its solute molecules)
            res = np.asarray(s.residue_of_atom)
            tors = []
            for r in np.unique(res[np.asarray(s.mass) > 0]):
                p = bonded_path(s, np.nonzero(res == r)[0])
                if p:
                    tors.append([len(tors), p[0], p[1], p[2], p[3], p[1], p[2], p[3], p[4]])
            s = dataclasses.replace(s, cmap_maps=tuple(smooth_map(24, k) for k in range(len(tors))), cmap_torsions=np.array(tors, np.int32))
        return s, v
    g = os.path.join(ROOT, "tests", "golden")
    prm = amber.read_prmtop(os.path.join(g, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(g, name + ".inpcrd"))
    s = amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=list(range(22, 32)), nonbonded_method="NoCutoff")
    if with_maps:
        names = list(s.names)
        c0 = names.index("C"); n1 = names.index("N", c0); ca = names.index("CA", n1); c1 = names.index("C", ca); last = names.index("OXT", c1)
        s = dataclasses.replace(s, cmap_maps=(smooth_map(24, 0),), cmap_torsions=np.array([[0, c0, n1, ca, c1, n1, ca, c1, last]], np.int32))
    return s, None


def bits(label):
    from blues_amd.engine import NativeEngine
    g = os.path.join(ROOT, "tests", "golden")
    prm = amber.read_prmtop(os.path.join(g, "TOL-parm.prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(g, "TOL-parm.inpcrd"))
    nocut = amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=list(range(15)), nonbonded_method="NoCutoff")
    periodic, v = systems.toluene_box()
    out = {"mode": "bits", "library": label}
    for sname, s, vel in (("NoCutoff TOL-parm", nocut, 0.3 * np.random.RandomState(7).standard_normal((nocut.n_atoms, 3)) * (nocut.mass[:, None] > 0)),
                          ("periodic toluene box", periodic, v)):
        for pname, precision in (("mixed", 0), ("double", 1)):
            e = NativeEngine(s, integrators.generateNCMCIntegrator(nstepsNC=45, dt=DT, temperature=300.0, seed=7).to_data(precision=precision))
            e.set_velocities(vel)
            e.step(3)
            l0 = e.stats()["kernel_launches"]
            e.step(42)
            out["%s, %s" % (sname, pname)] = {"protocol_work_bits": struct.pack(">d", e.get_global("protocol_work")).hex(),
                                              "launches_per_42_steps": int(e.stats()["kernel_launches"] - l0)}
            e.close()
    return out


def run(name, R, with_maps, steps, warmup, repeats):
    from blues_amd.engine import NativeBatch, NativeEngine
    s, v = system(name, with_maps)
    nsteps_nc = warmup + repeats * steps   # (one switch covers the measurement: no switch end in the timed steps)
    rng = np.random.RandomState(7)
    engs = []
    for r in range(R):
        d = integrators.generateNCMCIntegrator(nstepsNC=nsteps_nc, dt=DT, temperature=300.0, seed=100 + r).to_data(precision=0, replica=r)
        e = NativeEngine(s, d)
        e.set_velocities(v if v is not None else 0.3 * rng.standard_normal((s.n_atoms, 3)) * (s.mass[:, None] > 0))
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
    tors = np.asarray(s.cmap_torsions).reshape(-1, 9)
    mobile = np.asarray(s.mass) > 0
    out = {"system": name, "R": R, "maps": "with" if with_maps else "without", "atoms": s.n_atoms, "mobile_atoms": int(mobile.sum()), "steps": steps, "repeats": repeats,
           "us_per_step": us, "us_per_step_median": float(np.median(us)), "us_per_step_min": min(us), "us_per_step_max": max(us),
           "cmap_maps": len(s.cmap_maps), "cmap_torsions": len(tors), "cmap_entries": int(sum(len(set(int(a) for a in row[1:] if mobile[a])) for row in tors)),
           "plain_torsions": len(s.torsion_atoms), "lockstep_steps": st["lockstep_steps"], "fallback_steps": st["fallback_steps"]}
    b.close()
    for e in engs:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated NAME:R configurations instead of s23k_solute:64,vacDivaline:1024")
    ap.add_argument("--maps", default="with,without")
    ap.add_argument("--mode", default="cost", choices=("cost", "bits"))
    ap.add_argument("--label", default="this commit", help="what the record calls the library under test")
    a = ap.parse_args()
    if a.mode == "bits":
        print(json.dumps(bits(a.label)))
        return
    build.build_engine()
    cfgs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.only.split(",")] if a.only else DEFAULT
    res = [run(n, R, m == "with", a.steps, a.warmup, a.repeats) for n, R in cfgs for m in a.maps.split(",")]
    ratios = {}
    for n, R in cfgs:
        by = {r["maps"]: r["us_per_step_median"] for r in res if r["system"] == n and r["R"] == R}
        if "with" in by and "without" in by:
            ratios["%s:%d" % (n, R)] = by["with"] / by["without"]
    print(json.dumps({"metric": "NCMC step with and without CMAP torsions through NativeBatch (mixed precision)", "unit": "us/step", "dt_ps": DT,
                      "results": res, "with_over_without": ratios}))


if __name__ == "__main__":
    main()
