"""GPU suite: NoCutoff (vacuum) Systems on the HIP engine -- the all-pairs path (kernels_nocutoff.h) and the alchemical kernel over a
static list of every environment atom -- against the CPU oracle, whose NoCutoff path tests/test_nocutoff_cpu.py pins to an
independent numpy loop.  Tolerances as tests/test_gpu_parity.py: double 1e-10, mixed 1e-5."""
import copy
import os

import numpy as np
import pytest

from blues_amd import amber, integrators, moves, simulation, unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYSTEMS = {"TOL-parm": list(range(15)), "vacDivaline": list(range(22, 32))}
LAMBDAS = ((1.0, 1.0), (0.5, 0.3), (0.05, 0.0), (0.0, 0.0))


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def nocutoff_system(name):
    prm = amber.read_prmtop(os.path.join(GOLDEN, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, name + ".inpcrd"))
    return amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=SYSTEMS[name], nonbonded_method="NoCutoff")


def _integ(nsteps=20, dt=0.002, seed=7):
    return integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=dt, temperature=300.0, seed=seed)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


def _check_parity(g, o, tol, mass=None):
    mob = slice(None) if mass is None else mass > 0
    for ls, le in LAMBDAS:
        eo, fo, to = o.energy_forces(ls, le)
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        tg = g.energy_terms()
        for k in range(10):
            assert abs(tg[k] - to[k]) <= tol * max(abs(to[k]), 1.0), (ls, le, k, tg[k], to[k])
        assert abs(tg.sum() - eo) <= tol * max(abs(eo), 1.0), (ls, le, tg.sum(), eo)
        assert tg[8] == 0.0 and tg[9] == 0.0
        fg = g.get_forces()
        assert _rel(fg[mob], fo[mob]) <= tol, (ls, le, _rel(fg[mob], fo[mob]))
        if mass is not None:
            assert np.all(fg[mass == 0] == 0.0)   # forces on frozen atoms are never used by the path and are not computed (as periodic)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("precision,tol", [(1, 1e-10), (0, 1e-5)])
def test_parity_with_oracle(Engine, oracle_mod, name, precision, tol):
    s = nocutoff_system(name)
    data = _integ().to_data(precision=precision)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    _check_parity(g, o, tol)
    st = g.stats()
    assert st["nonbonded_kernel"] == 4 and st["list_builds"] == 0, st
    g.close()


@pytest.mark.parametrize("precision,tol", [(1, 1e-10), (0, 1e-5)])
def test_no_minimum_image(Engine, oracle_mod, precision, tol):
    s = nocutoff_system("TOL-parm")
    x = s.positions.copy()
    x[[15, 16, 17]] += np.array([50.0, 0.0, 0.0])   # the first water, 50 nm away (far outside the 2.2 nm box it came in)
    s.positions = x
    data = _integ().to_data(precision=precision)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    _check_parity(g, o, tol)
    g.close()


@pytest.mark.parametrize("precision", [1, 0])
def test_box_does_nothing(Engine, precision):
    s = nocutoff_system("vacDivaline")
    g = Engine(s, _integ().to_data(precision=precision))
    t0, f0 = g.energy_terms(), g.get_forces()
    for box in ((7.0, 8.0, 9.0), (0.0, 0.0, 0.0), (0.3, 0.3, 0.3)):
        g.set_box(box)
        assert np.allclose(np.diag(g.get_box()), box)
        assert np.array_equal(g.energy_terms(), t0) and np.array_equal(g.get_forces(), f0)
    g.close()


@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("precision,tol", [(1, 1e-9), (0, 1e-5)])
def test_short_switch_against_oracle(Engine, oracle_mod, name, precision, tol):
    s = nocutoff_system(name)
    data = _integ(nsteps=20).to_data(precision=precision)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    o.set_velocities_to_temperature(300.0, 11)
    g.set_velocities(o.get_velocities())
    wg = g.run_switch(20, trace=True)
    wo = []
    for _ in range(20):
        o.step(1); wo.append(o.get_global("protocol_work"))
    assert np.abs(wg - np.array(wo)).max() <= tol * max(1.0, np.abs(wo).max()), (wg[-1], wo[-1])
    assert np.abs(g.get_positions() - o.get_positions()).max() <= (1e-8 if precision == 1 else 1e-4)
    g.close()


def test_full_switch_double(Engine, oracle_mod):
    s = nocutoff_system("TOL-parm")
    data = _integ(nsteps=500).to_data(precision=1)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    o.set_velocities_to_temperature(300.0, 5)
    g.set_velocities(o.get_velocities())
    g.run_switch(500)
    o.step(500)
    wo = o.get_global("protocol_work")
    assert abs(g.get_global("protocol_work") - wo) <= 1e-6 * max(1.0, abs(wo)), (g.get_global("protocol_work"), wo)
    g.close()


@pytest.mark.parametrize("precision,tol", [(1, 1e-8), (0, 1e-4)])
def test_md_leg_against_oracle(Engine, oracle_mod, precision, tol):
    s = nocutoff_system("vacDivaline")
    data = integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=3).to_data(precision=precision)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    o.set_velocities_to_temperature(300.0, 2)
    g.set_velocities(o.get_velocities())
    g.step(50); o.step(50)
    assert np.abs(g.get_positions() - o.get_positions()).max() <= tol
    assert abs(g.potential_energy() - o.potential_energy()) <= 1e-4 * abs(o.potential_energy()) + 1e-6
    g.close()


@pytest.mark.parametrize("R", [8, 64])
def test_batch_equals_lone_chain(Engine, oracle_mod, R):
    from blues_amd.engine import NativeBatch
    s = nocutoff_system("TOL-parm")
    o = oracle_mod.Oracle(s, _integ().to_data(precision=0))
    starts = []
    for r in range(R):
        o.set_velocities_to_temperature(300.0, 100 + r); starts.append(o.get_velocities())

    def make(r):
        e = Engine(s, _integ(nsteps=20, seed=40 + r).to_data(precision=0, replica=r))
        e.set_velocities(starts[r])
        return e
    lone = []
    for r in range(R):
        e = make(r)
        w = e.run_switch(20, trace=True)
        lone.append((w, e.get_positions(), e.get_velocities()))
        e.close()
    engs = [make(r) for r in range(R)]
    batch = NativeBatch(engs)
    k0 = [e.stats()["kernel_launches"] for e in engs]
    _, w = batch.step(20, trace=True)
    for r in range(R):
        assert np.array_equal(w[r], lone[r][0]), r
        assert np.array_equal(engs[r].get_positions(), lone[r][1]) and np.array_equal(engs[r].get_velocities(), lone[r][2]), r
    st = batch.stats()
    # every step in lock step: the leader issues each kernel once with gridDim.y = R (the other members' launch calls are dry) ...
    assert st["fallback_steps"] == 0 and st["lockstep_steps"] > 0, st
    # ... in one launch sequence: the leader's launch calls and every dry member's are the same calls, so each member counts the
    # same number -- a leader that issued per-member launches would count R times more than the others
    per_member = {e.stats()["kernel_launches"] - k for e, k in zip(engs, k0)}
    assert len(per_member) == 1, per_member
    assert all(e.stats()["list_builds"] == 0 for e in engs)
    batch.close()
    for e in engs:
        e.close()


def test_batch_refuses_mixed_methods(Engine, tol_box):
    from blues_amd.engine import EngineError, NativeBatch
    a = Engine(nocutoff_system("TOL-parm"), _integ().to_data(precision=0))
    sp, _ = tol_box
    b = Engine(sp, _integ().to_data(precision=0, replica=1))
    try:
        with pytest.raises(EngineError, match="NoCutoff"):
            NativeBatch([a, b])
    finally:
        a.close(); b.close()


def _frozen_waters(s, count=25):
    """The last `count` waters of TOL-parm frozen (mass 0): frozen atoms exert forces and receive none."""
    s = copy.deepcopy(s)
    s.mass = s.mass.copy()
    s.mass[s.n_atoms - 3 * count:] = 0.0
    return s


@pytest.mark.parametrize("precision,tol", [(1, 1e-10), (0, 1e-5)])
def test_frozen_atoms_lone_and_batched_energies(Engine, oracle_mod, precision, tol):
    from blues_amd.engine import NativeBatch
    s = _frozen_waters(nocutoff_system("TOL-parm"))
    data = _integ().to_data(precision=precision)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    _check_parity(g, o, tol, s.mass)
    # new positions for the frozen atoms (what the MD leg's hand-over does): energies and forces follow
    x = s.positions.copy(); x[s.mass == 0.0] += np.array([0.05, -0.03, 0.02])
    g.set_positions(x); o.set_positions(x)
    _check_parity(g, o, tol, s.mass)
    g.close()
    # the batched energy evaluation (the driver's prefetch) of members with frozen atoms, after a hand-over of new positions
    R = 4
    engs, oracles = [], []
    for r in range(R):
        xr = x + 0.002 * r * (s.mass[:, None] > 0)
        d = _integ(seed=60 + r).to_data(precision=precision, replica=r)
        e = Engine(s, d); e.set_positions(xr); engs.append(e)
        oo = oracle_mod.Oracle(s, d); oo.set_positions(xr); oracles.append(oo)
    batch = NativeBatch(engs)
    batch.prefetch_energies(potential=True, kinetic=False)
    assert batch.stats()["batched_energy_evaluations"] >= 1
    for e, oo in zip(engs, oracles):
        eo = oo.energy_forces(1.0, 1.0)[0]
        assert abs(e.potential_energy() - eo) <= tol * abs(eo), (e.potential_energy(), eo)
    batch.close()
    for e in engs:
        e.close()


def _driver_chains(seed0, R=4, nsteps=10, nmd=6, nIter=2):
    from blues_amd.context import Simulation
    s = nocutoff_system("TOL-parm")
    md_sys = copy.copy(s); md_sys.alchemical_atoms = np.zeros(0, np.int32)
    lig = np.arange(15)
    o_v = np.random.RandomState(seed0)
    out = []
    for r in range(R):
        sim = Simulation(None, s, _integ(nsteps, seed=seed0 + r), precision="mixed", replica=r)
        md = Simulation(None, md_sys, integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=seed0 + 100 + r), precision="mixed", replica=r)
        alch = Simulation(None, md_sys, integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=seed0 + 200 + r), precision="mixed", replica=r)
        v = 0.3 * o_v.standard_normal((s.n_atoms, 3)) * (s.mass[:, None] > 0)
        md.context.setPositions(unit.Quantity(s.positions, "nanometer")); md.context.setVelocities(unit.Quantity(v, "nanometer/picosecond"))
        mover = moves.MoveEngine(moves.RandomLigandRotationMove(lig, s.mass[lig], random_state=seed0 + 300 + r))
        out.append(simulation.BLUESSimulation(simulation.SimulationSet(sim, md=md, alch=alch), {"nstepsNC": nsteps, "moveStep": nsteps // 2, "nIter": nIter, "nstepsMD": nmd},
                                              mover, rng=np.random.RandomState(seed0 + 400 + r)))
    return s, out


def _driver_run(seed0, nIter=2):
    s, cs = _driver_chains(seed0, nIter=nIter)
    B = simulation.BatchedBLUESSimulation(cs)
    assert B._batchable()
    records = []
    B.run(nIter=nIter, on_iteration=lambda N, last: records.append([dict(l) for l in last]))
    out = (records, [c._ncmc_sim.context._engine.get_positions() for c in cs], [c._md_sim.context._engine.get_positions() for c in cs],
           [c._md_sim.context._engine.get_velocities() for c in cs], [c.accept for c in cs])
    B.close()
    return s, out


def test_driver_random_ligand_rotation(Engine):
    """The reference's RandomLigandRotationMove test configuration (blues/tests/test_randomrotation.py: TOL-parm, NoCutoff, HBonds)
    through BatchedBLUESSimulation: every chain finishes, nothing is NaN, the ligand has moved, and one seed gives one result."""
    nIter = 2
    s, (rec, xn, xm, vm, acc) = _driver_run(1000, nIter)
    lig = np.arange(15)
    assert len(rec) == nIter and all(len(it) == 4 for it in rec)
    for it in rec:
        for r in it:
            assert np.isfinite(r["protocol_work"]) and np.isfinite(r["log_accept"]), r
    for r in range(4):
        assert np.all(np.isfinite(xn[r])) and np.all(np.isfinite(xm[r])) and np.all(np.isfinite(vm[r]))
        # the NCMC leg's final coordinates: the ligand was rotated at moveStep and has moved from where the run started
        assert np.abs(xn[r][lig] - s.positions[lig]).max() > 1e-3
    _, (rec2, xn2, xm2, vm2, acc2) = _driver_run(1000, nIter)
    assert acc == acc2
    for a, b in zip(rec, rec2):
        for ra, rb in zip(a, b):
            for key in ("accept", "log_accept", "correction", "randnum", "protocol_work"):
                assert ra[key] == rb[key], (key, ra[key], rb[key])
    for r in range(4):
        assert np.array_equal(xn[r], xn2[r]) and np.array_equal(xm[r], xm2[r]) and np.array_equal(vm[r], vm2[r])
