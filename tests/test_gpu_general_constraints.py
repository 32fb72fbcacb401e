"""GPU suite: general constraint clusters (AllBonds, HAngles; kernels_constraints.h) against the CPU oracle, whose
Gauss-Seidel SHAKE / RATTLE (oracle/blues_oracle.c) solves the same clusters.

Fixtures: the toluene box with the ligand's 7 harmonic bonds turned into constraints at their r0 (one 15-atom / 15-constraint
cluster, "AllBonds"), the same plus the three methyl H-H distances (18 constraints, "HAngles"), and a 100-atom chain in vacuum
(two atoms per lane, six waves' worth of constraints in two colours).

Tolerances.  With constraint_tolerance = 1e-12 both solvers are converged far below the project's double-precision bars whatever
their sweep order: protocol work 1e-9 max(1, |W|) (tests/test_gpu_switching.py), positions 1e-9 nm, velocities 1e-9 nm/ps.  At
the default 1e-8 two correct solvers may differ by O(tol) per step: the oracle alone moves by 5e-8 / 2e-7 kJ/mol between the two
tolerances over these 20 steps, so double precision is held to 1e-5 max(1, |W|) and mixed precision to its usual 2e-4 max(1, |W|)."""
import copy

import numpy as np
import pytest

from blues_amd import integrators, moves, systems
from blues_amd._abi import NB_NOCUTOFF, SystemData

pytestmark = pytest.mark.gpu

LIG = np.arange(15)
FUNCS = {"lambda_sterics": "1 - 0.3*sin(3.141592653589793*lambda)", "lambda_electrostatics": "1 - 0.5*sin(3.141592653589793*lambda)"}
NSTEPS = 20


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def general_ligand(s, hangles=False, lig=LIG):
    """The ligand's harmonic bonds -> constraints at r0; hangles: also its H-X-H angles -> H-H distances (hydrogens by mass < 4: the
    fixture is mass-repartitioned)."""
    s = copy.copy(s)
    ba, bp = np.asarray(s.bond_atoms), np.asarray(s.bond_params)
    m = np.isin(ba[:, 0], lig) & np.isin(ba[:, 1], lig)
    ca = [tuple(int(q) for q in p) for p in np.asarray(s.constraint_atoms)]
    cd = [float(d) for d in np.asarray(s.constraint_dist)]
    for (i, j), (r0, _) in zip(ba[m], bp[m]):
        ca.append((int(i), int(j))); cd.append(float(r0))
    s.bond_atoms, s.bond_params = ba[~m], bp[~m]
    if hangles:
        dist = {frozenset(p): d for p, d in zip(ca, cd)}
        aa, ap = np.asarray(s.angle_atoms), np.asarray(s.angle_params)
        keep = np.ones(len(aa), bool)
        for q, ((i, j, k), (th0, _)) in enumerate(zip(aa, ap)):
            if i in lig and k in lig and s.mass[i] < 4 and s.mass[k] < 4:
                d1, d2 = dist[frozenset((int(i), int(j)))], dist[frozenset((int(k), int(j)))]
                ca.append((int(i), int(k))); cd.append(float(np.sqrt(d1 * d1 + d2 * d2 - 2 * d1 * d2 * np.cos(th0))))
                keep[q] = False
        s.angle_atoms, s.angle_params = aa[keep], ap[keep]
    s.constraint_atoms = np.array(ca, dtype=np.int32).reshape(-1, 2)
    s.constraint_dist = np.array(cd, dtype=np.float64)
    return s


def chain_system(n=100, d=0.15):
    """Zigzag chain in vacuum: n atoms of mass 12, n - 1 constraints of length d, sigma 0.2, epsilon 0.3, 1-2 and 1-3 excluded,
    the first 3 atoms alchemical."""
    i = np.arange(n)
    x = np.stack([i * d * np.cos(np.pi / 6), (i % 2) * d * np.sin(np.pi / 6), np.zeros(n)], axis=1)
    excl = [(a, a + 1) for a in range(n - 1)] + [(a, a + 2) for a in range(n - 2)]
    return SystemData(box=np.zeros(3), mass=np.full(n, 12.0), charge=np.zeros(n), sigma=np.full(n, 0.2), epsilon=np.full(n, 0.3),
                      exclusions=np.array(sorted(excl), dtype=np.int32),
                      constraint_atoms=np.array([(a, a + 1) for a in range(n - 1)], dtype=np.int32), constraint_dist=np.full(n - 1, d),
                      alchemical_atoms=np.arange(3, dtype=np.int32), nonbonded_method=NB_NOCUTOFF, cutoff=1.0, ewald_alpha=0.0,
                      dispersion_correction=False, remove_cm_motion=True, positions=x)


def nocutoff(s):
    s = copy.copy(s)
    s.nonbonded_method, s.pme_grid, s.ewald_alpha, s.dispersion_correction = NB_NOCUTOFF, (0, 0, 0), 0.0, False
    return s


def mostly_frozen(s):
    near = systems.nearest_molecules(s, LIG, 60, exclude_idx=LIG)
    return systems.freeze_except(s, np.concatenate([LIG, near]))


def integ(tol, splitting="H V R O R V H", nprop=1, seed=7):
    return integrators.AlchemicalExternalLangevinIntegrator(FUNCS, splitting=splitting, temperature=300.0, timestep=0.002, constraint_tolerance=tol,
                                                            nsteps_neq=NSTEPS, nprop=nprop, seed=seed)


def constraint_errors(s, x, v):
    ca = np.asarray(s.constraint_atoms); m = (s.mass[ca[:, 0]] > 0) | (s.mass[ca[:, 1]] > 0)
    ca, cd = ca[m], np.asarray(s.constraint_dist)[m]
    r = x[ca[:, 0]] - x[ca[:, 1]]
    if s.nonbonded_method != NB_NOCUTOFF:
        r = systems.min_image(r, s.box)
    d2 = (r * r).sum(1)
    return (np.abs(d2 - cd * cd) / (cd * cd)).max(), np.abs(((v[ca[:, 0]] - v[ca[:, 1]]) * r).sum(1)).max()


_oracle_runs = {}


def oracle_run(oracle_mod, key, s, v, it):
    """(work after every step, final x, final v) of the oracle in double precision; computed once per key."""
    if key not in _oracle_runs:
        o = oracle_mod.Oracle(s, it.to_data(precision=1))
        o.set_velocities(v)
        w = []
        for _ in range(NSTEPS):
            o.step(1); w.append(o.get_global("protocol_work"))
        _oracle_runs[key] = (np.array(w), o.get_positions(), o.get_velocities())
    return _oracle_runs[key]


def gpu_run(Engine, s, v, it, precision):
    g = Engine(s, it.to_data(precision=precision))
    try:
        g.set_velocities(v)
        w = []
        for _ in range(NSTEPS):
            g.step(1); w.append(g.get_global("protocol_work"))
        return np.array(w), g.get_positions(), g.get_velocities(), g.stats()
    finally:
        g.close()


def check_tight(s, got, ref, tol):
    (wg, xg, vg, _), (wo, xo, vo) = got, ref
    print("work", wg[-1], wo[-1], "dW", np.abs(wg - wo).max(), "dx", np.abs(xg - xo).max(), "dv", np.abs(vg - vo).max(), "cons", constraint_errors(s, xg, vg))
    assert np.all(np.abs(wg - wo) <= 1e-9 * np.maximum(1.0, np.abs(wo))), (wg, wo)
    assert np.abs(xg - xo).max() <= 1e-9 and np.abs(vg - vo).max() <= 1e-9
    ex, ev = constraint_errors(s, xg, vg)
    # |d^2 - r^2| <= 2 tol d^2 is the solver's own acceptance; (v_i - v_j).r: RATTLE accepts |delta| <= tol with
    # delta = -(dv.r) / (r.r (w_i + w_j)), so |dv.r| <= tol r.r (w_i + w_j) <= tol * 0.04 nm^2 * 2 / (1 u) -- 1e-13 at tol = 1e-12: rounding level
    assert ex <= 2 * tol * (1 + 1e-3) + 4e-16 and ev <= tol * 0.08 + 1e-13, (ex, ev)


# ---- 1. it runs at all
@pytest.mark.parametrize("hangles", [False, True])
def test_general_cluster_engine_is_created(Engine, tol_box, hangles):
    s, v = tol_box
    g = Engine(general_ligand(s, hangles), integ(1e-8).to_data(precision=0))
    try:
        g.set_velocities(v)
        g.step(2)
        st = g.stats()
        assert np.all(np.isfinite(g.get_positions()))
        assert st["clusters"] >= 321, st   # 320 rigid waters (their slots padded to whole waves) + the one general cluster
    finally:
        g.close()


def test_capacity_is_stated(Engine):
    from blues_amd.engine import EngineError
    with pytest.raises(EngineError, match=r"130 atoms and 129 constraints.*128 atoms, 192 constraints"):
        Engine(chain_system(130), integ(1e-8).to_data(precision=1))


# ---- 2. parity with the oracle, double precision, constraint_tolerance 1e-12
LAYOUTS = {
    "periodic": lambda s: s,
    "frozen": mostly_frozen,
    "pme": systems.with_reciprocal_space,
    "nocutoff": nocutoff,
}


@pytest.mark.parametrize("hangles", [False, True])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_parity_with_the_oracle_converged(Engine, oracle_mod, tol_box, layout, hangles):
    s0, v = tol_box
    s = LAYOUTS[layout](general_ligand(s0, hangles))
    it = integ(1e-12)
    check_tight(s, gpu_run(Engine, s, v, it, 1), oracle_run(oracle_mod, (layout, hangles, 1e-12), s, v, it), 1e-12)


# ---- 3. default tolerance, mixed and double
@pytest.mark.parametrize("hangles", [False, True])
@pytest.mark.parametrize("precision,bar", [(1, 1e-5), (0, 2e-4)])
def test_default_tolerance(Engine, oracle_mod, tol_box, precision, bar, hangles):
    s0, v = tol_box
    s = mostly_frozen(general_ligand(s0, hangles))
    it = integ(1e-8)
    wg, xg, vg, _ = gpu_run(Engine, s, v, it, precision)
    wo, xo, vo = oracle_run(oracle_mod, ("frozen", hangles, 1e-8), s, v, it)
    print("work", wg[-1], wo[-1], "dW", np.abs(wg - wo).max(), "dx", np.abs(xg - xo).max())
    assert np.all(np.abs(wg - wo) <= bar * np.maximum(1.0, np.abs(wo))), (wg, wo)
    assert constraint_errors(s, xg, vg)[0] <= 2e-8 * (1 + 1e-3)


# ---- 4. other programs
@pytest.mark.parametrize("splitting,nprop", [("R V O H O V R", 1), ("H V R O R V H", 2)])
def test_other_programs(Engine, oracle_mod, tol_box, splitting, nprop):
    s0, v = tol_box
    s = mostly_frozen(general_ligand(s0, True))
    it = integ(1e-12, splitting=splitting, nprop=nprop)
    check_tight(s, gpu_run(Engine, s, v, it, 1), oracle_run(oracle_mod, ("frozen", splitting, nprop), s, v, it), 1e-12)


def test_md_leg(Engine, oracle_mod, tol_box):
    s0, v = tol_box
    s = general_ligand(s0, True)
    s.alchemical_atoms = np.zeros(0, np.int32)
    it = integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=3); it.setConstraintTolerance(1e-12)
    data = it.to_data(precision=1)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    try:
        g.set_velocities(v); o.set_velocities(v)
        g.step(NSTEPS); o.step(NSTEPS)
        xg, vg = g.get_positions(), g.get_velocities()
        print("dx", np.abs(xg - o.get_positions()).max(), "dv", np.abs(vg - o.get_velocities()).max(), constraint_errors(s, xg, vg))
        assert np.abs(xg - o.get_positions()).max() <= 1e-9 and np.abs(vg - o.get_velocities()).max() <= 1e-9
        assert constraint_errors(s, xg, vg)[0] <= 2e-12 * (1 + 1e-3) + 4e-16
    finally:
        g.close()


def test_velocities_to_temperature_are_constrained(Engine, tol_box):
    s0, _ = tol_box
    s = general_ligand(s0, True)
    g = Engine(s, integ(1e-12).to_data(precision=1))
    try:
        g.set_velocities_to_temperature(300.0, 17)
        x, v = g.get_positions(), g.get_velocities()
        assert np.abs(v[LIG]).max() > 0.05
        ca = np.asarray(s.constraint_atoms)
        r = systems.min_image(x[ca[:, 0]] - x[ca[:, 1]], s.box)
        assert np.abs(((v[ca[:, 0]] - v[ca[:, 1]]) * r).sum(1)).max() <= 1e-12 * 0.08 + 1e-13
    finally:
        g.close()


# ---- 5. more than one atom per lane, more than one cluster per chain
def test_chain_of_100(Engine, oracle_mod):
    s = chain_system(100)
    it = integ(1e-12)
    data = it.to_data(precision=1)
    o = oracle_mod.Oracle(s, data)
    o.set_velocities_to_temperature(300.0, 11)
    v = o.get_velocities()
    wg, xg, vg, st = gpu_run(Engine, s, v, it, 1)
    o.step(NSTEPS)
    ex, ev = constraint_errors(s, xg, vg)
    print("dx", np.abs(xg - o.get_positions()).max(), "dv", np.abs(vg - o.get_velocities()).max(), "cons", ex, ev, "work", wg[-1], o.get_global("protocol_work"))
    assert np.abs(xg - o.get_positions()).max() <= 1e-9
    assert ex <= 2e-12 * (1 + 1e-3) + 4e-16
    assert np.abs(xg - s.positions).max() > 1e-3   # (it moved)


def test_two_general_clusters_beside_small_ones(Engine, oracle_mod, tol_box):
    s0, v0 = tol_box
    s = systems.tile_system(general_ligand(s0, False), (2, 1, 1))
    v = np.concatenate([v0, v0], axis=0)
    it = integ(1e-12)
    wg, xg, vg, _ = gpu_run(Engine, s, v, it, 1)
    wo, xo, vo = oracle_run(oracle_mod, ("two", 1e-12), s, v, it)
    print("dW", np.abs(wg - wo).max(), "dx", np.abs(xg - xo).max(), "dv", np.abs(vg - vo).max())
    assert np.all(np.abs(wg - wo) <= 1e-9 * np.maximum(1.0, np.abs(wo)))
    assert np.abs(xg - xo).max() <= 1e-9 and np.abs(vg - vo).max() <= 1e-9
    assert constraint_errors(s, xg, vg)[0] <= 2e-12 * (1 + 1e-3) + 4e-16


# ---- 6. batch = solo, bitwise
def test_batch_equals_lone_chain_bitwise(Engine, tol_box, tune):
    from blues_amd.engine import NativeBatch
    s0, v0 = tol_box
    s = mostly_frozen(general_ligand(s0, False))
    R, n1, n2 = 8, 20, 25
    tune(assume_batch=R)   # (the lone chain lays itself out as a batch member does, as in tests/test_gpu_batch.py; nothing else pinned)
    it = lambda r: integrators.AlchemicalExternalLangevinIntegrator(FUNCS, splitting="H V R O R V H", temperature=300.0, timestep=0.002,
                                                                    nsteps_neq=n1 + n2, seed=40 + r)
    rot = lambda r: moves.RandomLigandRotationMove(LIG, s.mass[LIG], random_state=300 + r)

    def make(r):
        e = Engine(s, it(r).to_data(precision=0, replica=r))
        e.set_velocities(v0 * (1.0 + 0.01 * r))
        return e
    lone = []
    for r in range(R):
        e = make(r)
        e.step(n1)
        snap = e.snapshot(positions=True, velocities=False)
        assert e.set_positions_from_snapshot_edited(snap, LIG, rot(r).propose(e.get_positions()[LIG]))   # the whole ligand: one cluster
        snap.release()
        e.step(n2)
        lone.append((e.get_positions(), e.get_velocities(), e.get_global("protocol_work")))
        e.close()
    engs = [make(r) for r in range(R)]
    batch = NativeBatch(engs)
    try:
        batch.step(n1)
        snaps = batch.snapshot_all(positions=True, velocities=False)
        xl = batch.read_atoms_all(LIG, snaps)
        assert batch.restore_edited_all(snaps, LIG, np.stack([rot(r).propose(xl[r]) for r in range(R)]))
        for sn in snaps:
            sn.release()
        batch.step(n2)
        for r in range(R):
            assert np.array_equal(engs[r].get_positions(), lone[r][0]) and np.array_equal(engs[r].get_velocities(), lone[r][1]), r
            assert engs[r].get_global("protocol_work") == lone[r][2], r
        st = batch.stats()
        assert st["fallback_steps"] == 0 and st["lockstep_steps"] > 0, st
    finally:
        batch.close()
        for e in engs:
            e.close()


# ---- 7. nothing fails silently
def test_unconverged_solver_is_an_error(Engine):
    """The 100-atom chain (one general cluster, nothing else) from its exact geometry with a tolerance below double rounding:
    |d^2 - r^2| <= 2e-17 d^2 is less than a unit in the last place of d^2, so after the first drift the 99 constraints are
    practically never all accepted in one sweep; the sweeps stay finite, reach 500, and the step ends in the engine's error."""
    from blues_amd.engine import EngineError
    s = chain_system(100)
    g = Engine(s, integ(1e-17).to_data(precision=1))
    try:
        g.set_velocities_to_temperature(300.0, 11)
        with pytest.raises(EngineError, match="constraint solver did not converge"):
            g.step(2)
            g.get_positions()
    finally:
        g.close()


def test_measuring_integrator_is_refused(Engine, tol_box):
    from blues_amd.engine import EngineError
    s0, _ = tol_box
    it = integrators.AlchemicalExternalLangevinIntegrator(FUNCS, splitting="H V R O R V H", temperature=300.0, timestep=0.002, nsteps_neq=NSTEPS,
                                                          measure_shadow_work=True)
    with pytest.raises(EngineError, match="measure_shadow_work / measure_heat are not supported on a System with general constraint clusters"):
        Engine(general_ligand(s0, False), it.to_data(precision=1))
