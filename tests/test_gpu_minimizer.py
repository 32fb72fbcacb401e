"""GPU suite: the device-resident minimiser (kernels_minimize.h) -- FIRE under the engine's constraints, lone and as
one launch sequence over a replica batch -- against its numpy reference (tests/fire_reference.py) on the CPU oracle's forces.
Constraint tolerance 1e-10 and the default FIRE constants throughout.

Tolerances.  The reference solves every cluster to 1e-13; the engine's SHAKE stops at 2e-10 d^2 and polishes once (quadratic: below
rounding), RATTLE is one linear solve.  Forces agree with the oracle's to 1e-10 in double precision (tests/test_gpu_parity.py).  Over
25 iterations of a descent (no chaos: every iterate is a smooth function of the forces as long as the discrete decisions agree, which
the fixture guarantees by construction and the test asserts from the reference's record) that leaves positions to 1e-9 nm and fmax to
1e-8 relative; dt and alpha are products of the constants alone: 1e-12."""
import copy
import os

import numpy as np
import pytest

import fire_reference as fr
from blues_amd import amber, integrators, systems
from blues_amd._abi import NB_NOCUTOFF, SystemData

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIG = np.arange(15)
FUNCS = {"lambda_sterics": "1 - 0.3*sin(3.141592653589793*lambda)", "lambda_electrostatics": "1 - 0.5*sin(3.141592653589793*lambda)"}
TOL_CONS = 1e-10
# mixed precision, case 3: how far the projected fmax recomputed from get_forces() may exceed the tolerance.  The minimiser's last
# pass and get_forces() run the same kernels on the same image, so the excess measured is 0 (profiles/minimizer/README.md); twice
# that is 0, and what remains is the reference projection's own rounding against the device's: the double-precision allowance.
MIXED_EXCESS = 0.0


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def integ(nsteps=20, seed=7):
    return integrators.AlchemicalExternalLangevinIntegrator(FUNCS, splitting="H V R O R V H", temperature=300.0, timestep=0.002,
                                                            constraint_tolerance=TOL_CONS, nsteps_neq=nsteps, seed=seed)


def mostly_frozen(s):
    near = systems.nearest_molecules(s, LIG, 60, exclude_idx=LIG)
    return systems.freeze_except(s, np.concatenate([LIG, near]))


def jittered(s, amount, seed):
    mob = np.asarray(s.mass) > 0
    x = np.array(s.positions, dtype=np.float64)
    x[mob] += amount * np.random.RandomState(seed).uniform(-1.0, 1.0, (int(mob.sum()), 3))
    return x


def inverse_mass(s):
    mob = np.asarray(s.mass) > 0
    return np.where(mob, 1.0 / np.where(mob, s.mass, 1.0), 0.0)


def constraints_of(s):
    return fr.Constraints(s.constraint_atoms, s.constraint_dist, inverse_mass(s), box=None if s.nonbonded_method == NB_NOCUTOFF else s.box)


def constraint_errors(s, x, v):
    ca = np.asarray(s.constraint_atoms); m = (s.mass[ca[:, 0]] > 0) | (s.mass[ca[:, 1]] > 0)
    ca, cd = ca[m], np.asarray(s.constraint_dist)[m]
    r = x[ca[:, 0]] - x[ca[:, 1]]
    if s.nonbonded_method != NB_NOCUTOFF:
        r = systems.min_image(r, s.box)
    return (np.abs((r * r).sum(1) - cd * cd) / (cd * cd)).max(), np.abs(((v[ca[:, 0]] - v[ca[:, 1]]) * r).sum(1)).max()


_shared = {}


def lj13_reference(oracle_mod, tolerance):
    """The CPU reference's LJ13 converged to `tolerance`: computed once per tolerance."""
    if ("lj13", tolerance) not in _shared:
        s = fr.lj13()
        forces, energy = fr.oracle_forces(oracle_mod.Oracle(s, integ().to_data(precision=1)))
        x, res, _ = fr.minimize(s.positions, constraints_of(s), forces, tolerance)
        assert res["converged"] == 1
        _shared[("lj13", tolerance)] = (s, x, energy(x))
    return _shared[("lj13", tolerance)]


# ---- 1. known answer
@pytest.mark.parametrize("precision,tolerance,e_tol", [(1, 1e-3, 1e-9), (0, 0.05, 1e-6)])
def test_lj13_known_answer(Engine, oracle_mod, precision, tolerance, e_tol):
    """The energy is compared with the CPU reference converged to the SAME tolerance: stopping at fmax <= 0.05 leaves the cluster 1.9e-5
    kJ/mol (1.4e-6 relative) above the structure converged to 1e-3, in fp64 as in mixed precision -- that gap belongs to the tolerance,
    not to the engine."""
    s, x_ref, e_ref = lj13_reference(oracle_mod, tolerance)
    g = Engine(s, integ().to_data(precision=precision))
    r = g.minimize(tolerance)
    x = g.get_positions(); g.close()
    print("LJ13 precision %d: %s; reference energy %.12f" % (precision, r, e_ref))
    assert r["converged"] == 1 and r["fmax"] <= tolerance
    assert abs(r["e_final"] - e_ref) <= e_tol * abs(e_ref), (r["e_final"], e_ref)
    if precision == 1:
        assert fr.kabsch_rmsd_max(x_ref, x) <= 1e-6


# ---- 2. iterate parity
@pytest.mark.parametrize("reciprocal", [False, True])
def test_iterate_parity_with_the_reference(Engine, oracle_mod, tol_box, reciprocal):
    s = mostly_frozen(tol_box[0])
    if reciprocal:
        s = systems.with_reciprocal_space(s)
    x0 = jittered(s, 0.005, seed=0)
    data = integ().to_data(precision=1)
    forces, _ = fr.oracle_forces(oracle_mod.Oracle(s, data))
    x_ref, ref, rec = fr.minimize(x0, constraints_of(s), forces, 1e-9, 25)
    # condition on the fixture: no discrete decision of these 25 iterations is close enough to its threshold to differ legitimately
    assert ref["iterations"] == 25 and ref["converged"] == 0
    assert all(abs(q["P"]) >= 1e-6 * np.sqrt(q["GG"] * q["VV"]) for q in rec[1:-1])
    assert all(q["clip"] >= 1e-6 for q in rec[:-1])
    assert any(q["P"] < 0.0 for q in rec[1:-1])   # (the uphill branch is part of the 25)
    g = Engine(s, data)
    g.set_positions(x0)
    r = g.minimize(1e-9, 25)
    x = g.get_positions(); g.close()
    print("parity (reciprocal %s): engine %s\n   reference %s; dx %.3e" % (reciprocal, r, ref, np.abs(x - x_ref).max()))
    assert r["iterations"] == ref["iterations"] and r["n_pos"] == ref["n_pos"] and r["converged"] == 0
    assert abs(r["dt"] - ref["dt"]) <= 1e-12 * ref["dt"] and abs(r["alpha"] - ref["alpha"]) <= 1e-12 * ref["alpha"]
    assert abs(r["fmax"] - ref["fmax"]) <= 1e-8 * ref["fmax"]
    assert np.abs(x - x_ref).max() <= 1e-9


# ---- 3. properties
def case3_system(tol_box):
    return mostly_frozen(tol_box[0]), tol_box[1]


@pytest.mark.parametrize("precision", [1, 0])
def test_properties_of_a_converged_run(Engine, tol_box, precision):
    s, v = case3_system(tol_box)
    g = Engine(s, integ().to_data(precision=precision))
    g.set_positions(jittered(s, 0.01, seed=1)); g.set_velocities(v)
    g.step(2)   # (inside a switch: step, lambda and protocol work are not at their initial values)
    before = {k: g.get_global(k) for k in ("step", "lambda", "lambda_step", "protocol_work", "lambda_sterics", "lambda_electrostatics")}
    x_before = g.get_positions()
    r = g.minimize(10.0, 3000)
    x, vel = g.get_positions(), g.get_velocities()
    print("properties precision %d: %s" % (precision, r))
    assert r["converged"] == 1 and r["fmax"] <= 10.0 and 0 < r["iterations"] < 3000
    cons = constraints_of(s); mob = np.asarray(s.mass) > 0
    fmax_np = np.abs(cons.project_force(x, g.get_forces())[mob]).max()
    print("   projected fmax recomputed in numpy: %.12g (engine %.12g); excess over the tolerance %.3e" % (fmax_np, r["fmax"], fmax_np - 10.0))
    assert fmax_np <= 10.0 * (1 + 1e-6) + (2 * MIXED_EXCESS if precision == 0 else 0.0)
    assert r["e_final"] < r["e_initial"] and r["e_final"] == g.potential_energy()
    ex, ev = constraint_errors(s, x, vel)
    assert ex <= 1e-8, ex
    # RATTLE is one linear solve in fp64: (v_i - v_j).r is left at rounding level of |v| |r| ~ 1 nm/ps x 0.15 nm
    assert ev <= 1e-12, ev
    assert np.array_equal(x[~mob], x_before[~mob]) and not np.array_equal(x[mob], x_before[mob])
    after = {k: g.get_global(k) for k in before}
    assert after == before, (before, after)
    g.close()


# ---- 4. no residue
def test_minimising_leaves_no_residue_in_a_later_switch(Engine, tol_box):
    """Snapshot, minimise, restore, 12-step switch: work trace and final state bitwise those of an engine that never minimised.
    The engine that never minimised takes and restores its snapshot too: a restore alone moves the later work trace by 3e-13 kJ/mol against
    an untouched engine, with or without a minimisation in between (measured, profiles/minimizer/README.md: older than the minimiser),
    so like is compared with like.
    48 iterations: three read-backs of the state, and short of the 64-iteration poll at which the list builder may ask for a new
    order -- a re-sort is a new layout, not state, and like a re-sort while stepping it changes the order of later sums (1e-13)."""
    s, v = case3_system(tol_box)
    data = integ(nsteps=12).to_data(precision=1)

    def run(minimise):
        g = Engine(s, data); g.set_velocities(v)
        snap = g.snapshot()
        if minimise:
            r = g.minimize(10.0, 48)
            assert r["iterations"] == 48 and r["e_final"] < r["e_initial"] and g.stats()["resorts"] == 0
            assert not np.array_equal(g.get_positions(), snap.read(1))
        g.set_positions_from_snapshot(snap); g.set_velocities_from_snapshot(snap)
        w = g.run_switch(12, trace=True)
        out = (w, g.get_positions(), g.get_velocities(), g.get_global("protocol_work"), g.get_global("step"))
        g.close()
        return out
    wa, xa, va, pa, sa = run(True)
    wb, xb, vb, pb, sb = run(False)
    assert np.array_equal(wa, wb), np.abs(wa - wb).max()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert pa == pb and sa == sb == 12


# ---- 5. lists stay valid
def test_lists_stay_valid_on_the_fragment_list_path(Engine, tol_box, tune):
    s = tol_box[0]
    tune(k1_mode=3)
    g = Engine(s, integ().to_data(precision=0))
    assert g.stats()["nonbonded_kernel"] == 3, g.stats()
    g.set_positions(jittered(s, 0.02, seed=2))
    builds = g.stats()["list_builds"]
    r = g.minimize(10.0, 300)
    st = g.stats()
    print("fragment lists: %s; list builds %d -> %d" % (r, builds, st["list_builds"]))
    assert r["iterations"] > 100
    assert g.audit_lists()[1] == 0
    assert st["list_builds"] > builds + 1
    assert r["e_final"] < r["e_initial"]
    g.close()


# ---- 6. batch = solo
def test_batch_members_are_bitwise_the_lone_runs(Engine, tol_box, tune):
    from blues_amd.engine import NativeBatch
    s, v = case3_system(tol_box)
    R = 8
    tune(assume_batch=R)
    keys = ("converged", "iterations", "n_pos", "fmax", "dt", "alpha", "e_initial", "e_final")

    def make(r, x):
        g = Engine(s, integ(seed=30 + r).to_data(precision=1, replica=r))
        g.set_positions(x); g.set_velocities(v * (1.0 + 0.01 * r))
        return g
    starts = [jittered(s, 0.01, seed=10 + r) for r in range(6)]
    solo, res_solo = [], []
    for r in range(6):
        solo.append(make(r, starts[r])); res_solo.append(solo[r].minimize(10.0, 3000))
    starts.append(solo[0].get_positions())        # member 6 starts where member 0 ended
    solo.append(make(6, starts[6])); res_solo.append(solo[6].minimize(10.0, 3000))
    starts.append(jittered(s, 0.01, seed=17))     # member 7 sits the call out
    bat = [make(r, starts[r]) for r in range(R)]
    x7, v7 = bat[7].get_positions(), bat[7].get_velocities()
    batch = NativeBatch(bat)
    errors, res = batch.minimize_all(10.0, 3000, active=[1] * 7 + [0])
    assert not any(errors) and res[7] is None
    print("batch = solo: iterations %s" % [q["iterations"] for q in res[:7]])
    for r in range(7):
        assert {k: res[r][k] for k in keys} == {k: res_solo[r][k] for k in keys}, (r, res[r], res_solo[r])
        assert res[r]["converged"] == 1
        assert np.array_equal(bat[r].get_positions(), solo[r].get_positions()), r
        assert np.array_equal(bat[r].get_velocities(), solo[r].get_velocities()), r
    assert np.array_equal(bat[7].get_positions(), x7) and np.array_equal(bat[7].get_velocities(), v7)
    assert len(set(q["iterations"] for q in res[:6])) > 1      # the members finish at different iterations
    assert res[6]["iterations"] < min(q["iterations"] for q in res[:6])
    print("   batch counters: %s" % batch.stats())
    batch.close()
    for g in solo + bat:
        g.close()


# ---- 7. other force paths, lone
def gb_system(name, alchemical):
    prm = amber.read_prmtop(os.path.join(GOLDEN, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, name + ".inpcrd"))
    return amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=alchemical, nonbonded_method="NoCutoff", implicit_solvent="OBC2")


def gb_integ(precision):
    return integrators.generateNCMCIntegrator(nstepsNC=20, dt=0.002, temperature=300.0, seed=7).to_data(precision=precision)


@pytest.mark.parametrize("precision", [1, 0])
def test_implicit_solvent_system_converges(Engine, precision):
    """vacDivaline in OBC2, every atom mobile -- the solute-in-GB System of tests/test_gpu_implicit_solvent.py."""
    s = gb_system("vacDivaline", list(range(22, 32)))
    g = Engine(s, gb_integ(precision))
    r = g.minimize(10.0, 3000)
    x = g.get_positions()
    print("GB vacDivaline precision %d: %s" % (precision, r))
    assert r["converged"] == 1 and r["fmax"] <= 10.0 and r["e_final"] < r["e_initial"]
    assert r["e_final"] == g.potential_energy()
    assert np.abs(constraints_of(s).project_force(x, g.get_forces())).max() <= 10.0 * (1 + 1e-6)
    assert constraint_errors(s, x, g.get_velocities())[0] <= 1e-8
    g.close()


def test_implicit_solvent_droplet_descends(Engine):
    """The other GB System of that file: the TOL-parm water droplet, molecules within 0.8 nm of the ligand mobile (438 atoms).  It
    does NOT reach 10 kJ/mol/nm in a test's time and convergence is not asserted: the droplet keeps relaxing (E -13696 -> -15352 ->
    -15787 -> -16039 kJ/mol after 1000, 2000, 3000 iterations, -17494 after 30000 with fmax still 15.9), while its forces are the
    energy's gradient to 1e-9 by central differences at the start and after 3000 iterations, and the same System without GB converges
    in 2227 iterations (profiles/minimizer/README.md).  Asserted: the descent, and that the minimiser's projected fmax is the one numpy
    forms from get_forces() at the final positions (both sum the GB force into the environment's and the alchemical atoms' share)."""
    s = gb_system("TOL-parm", list(range(15)))
    lig = np.asarray(s.alchemical_atoms)
    d = np.sqrt(((s.positions[:, None, :] - s.positions[None, lig, :]) ** 2).sum(-1)).min(1)
    res = np.asarray(s.residue_of_atom)
    s = copy.deepcopy(s)
    s.mass = np.where(np.isin(res, np.unique(res[d <= 0.8])), s.mass, 0.0)   # (whole molecules near the ligand stay mobile)
    g = Engine(s, gb_integ(1))
    r = g.minimize(10.0, 500)
    x = g.get_positions(); mob = s.mass > 0
    print("GB droplet: %s" % r)
    assert r["iterations"] == 500 and r["e_final"] < r["e_initial"] and r["e_final"] == g.potential_energy()
    fmax_np = np.abs(constraints_of(s).project_force(x, g.get_forces())[mob]).max()
    assert abs(fmax_np - r["fmax"]) <= 1e-9 * r["fmax"], (fmax_np, r["fmax"])
    assert constraint_errors(s, x, g.get_velocities())[0] <= 1e-8
    g.close()


def test_vacuum_chain_with_bond_constraints_converges(Engine):
    """A zigzag chain in vacuum whose constraints are pairs (0,1), (2,3), ...: clusters of two atoms, the other bonds harmonic."""
    n, d = 40, 0.15
    i = np.arange(n)
    x = np.stack([i * d * np.cos(np.pi / 6), (i % 2) * d * np.sin(np.pi / 6), np.zeros(n)], axis=1)
    x += 0.01 * np.random.RandomState(4).uniform(-1, 1, x.shape)
    excl = [(a, a + 1) for a in range(n - 1)] + [(a, a + 2) for a in range(n - 2)]
    s = SystemData(box=np.zeros(3), mass=np.full(n, 12.0), charge=np.zeros(n), sigma=np.full(n, 0.2), epsilon=np.full(n, 0.3),
                   exclusions=np.array(sorted(excl), dtype=np.int32),
                   bond_atoms=np.array([(a, a + 1) for a in range(1, n - 1, 2)], dtype=np.int32), bond_params=np.tile([d, 2.0e5], (len(range(1, n - 1, 2)), 1)),
                   constraint_atoms=np.array([(a, a + 1) for a in range(0, n - 1, 2)], dtype=np.int32), constraint_dist=np.full(n // 2, d),
                   alchemical_atoms=np.arange(3, dtype=np.int32), nonbonded_method=NB_NOCUTOFF, cutoff=1.0, ewald_alpha=0.0,
                   dispersion_correction=False, remove_cm_motion=True, positions=x)
    g = Engine(s, integ().to_data(precision=1))
    r = g.minimize(1.0, 5000)
    xs = g.get_positions()
    print("chain: %s" % r)
    assert r["converged"] == 1 and r["e_final"] < r["e_initial"]
    assert constraint_errors(s, xs, g.get_velocities())[0] <= 1e-8
    fmax_np = np.abs(constraints_of(s).project_force(xs, g.get_forces())).max()
    assert fmax_np <= 1.0 * (1 + 1e-6)
    g.close()


# ---- 8. refusals and the Python surface
def test_refusals(Engine, tol_box):
    from blues_amd.engine import EngineError
    s = tol_box[0]
    ba, bp = np.asarray(s.bond_atoms), np.asarray(s.bond_params)
    m = np.isin(ba[:, 0], LIG) & np.isin(ba[:, 1], LIG)
    gen = copy.copy(s)
    gen.constraint_atoms = np.concatenate([np.asarray(s.constraint_atoms).reshape(-1, 2), ba[m]]).astype(np.int32)
    gen.constraint_dist = np.concatenate([np.asarray(s.constraint_dist), bp[m][:, 0]])
    gen.bond_atoms, gen.bond_params = ba[~m], bp[~m]
    g = Engine(mostly_frozen(gen), integ().to_data(precision=1))
    with pytest.raises(EngineError, match="general clusters"):
        g.minimize(10.0)
    g.close()
    g = Engine(mostly_frozen(s), integ().to_data(precision=1))
    with pytest.raises(EngineError, match="tolerance"):
        g.minimize(0.0)
    with pytest.raises(EngineError, match="max_iterations"):
        g.minimize(10.0, -1)
    g.set_positions(jittered(mostly_frozen(s), 0.01, seed=1))
    r = g.minimize(10.0, 5)
    assert r["converged"] == 0 and r["iterations"] == 5
    g.close()


def test_python_surface_reaches_the_same_numbers(Engine, tol_box):
    from blues_amd import unit
    from blues_amd.context import LocalEnergyMinimizer, Simulation
    s, v = case3_system(tol_box)
    x0 = jittered(s, 0.01, seed=1)
    g = Engine(s, integ().to_data(precision=1)); g.set_positions(x0)
    ref = g.minimize(10.0, 400)
    x_ref = g.get_positions(); g.close()
    sim = Simulation(None, s, integ(), precision="double")
    sim.context._engine.set_positions(x0)
    got = sim.minimizeEnergy(unit.Quantity(10.0, "kilojoule/(nanometer*mole)"), 400, method="device")
    assert got == ref and np.array_equal(sim.context._engine.get_positions(), x_ref)
    sim2 = Simulation(None, s, integ(), precision="double")
    sim2.context._engine.set_positions(x0)
    got2 = LocalEnergyMinimizer.minimize(sim2.context, 10, 400)
    assert got2 == ref and np.array_equal(sim2.context._engine.get_positions(), x_ref)
    with pytest.raises(ValueError):
        sim2.minimizeEnergy(method="lbfgs")
    sim.context._engine.close(); sim2.context._engine.close()
