"""GPU suite: heat and shadow work of the Langevin switch measured on the device (measure_shadow_work / measure_heat, ABI 9) and the
first-law ledger they close:

    dE = d protocol_work + d shadow_work + d heat + sum dKE_cm,      E = potential + kinetic energy,

dKE_cm = -|p|^2 / (2 M) being what the CMMotionRemover takes at the head of a pass (p, M: momentum and mass of the mobile atoms).
Tolerances are those of test_velocity_verlet_switching_matches_the_oracle: tol = 1e-9 (double) / 2e-4 (mixed) times
max(1, |protocol_work|), plus 5e-7 |E| in mixed precision for what differences total energies."""
import copy
import os

import numpy as np
import pytest

from blues_amd import amber, integrators, moves, simulation, systems, unit

pytestmark = pytest.mark.gpu
CASES = [(1, 1e-9, 0.002), (0, 2e-4, 0.0015)]   # precision, tol, timestep (tests/test_gpu_switching.py:32-36 on the mixed step)
KT = integrators.KB * 300.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _integ(dt, nsteps=12, seed=3, shadow=True, heat=True, **kw):
    if kw:
        return integrators.AlchemicalExternalLangevinIntegrator(dict(integrators.DEFAULT_ALCHEMICAL_FUNCTIONS), temperature=300.0, timestep=dt,
                                                                nsteps_neq=nsteps, seed=seed, measure_shadow_work=shadow, measure_heat=heat, **kw)
    return integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=dt, temperature=300.0, seed=seed, measure_shadow_work=shadow, measure_heat=heat)


def _cm(system, cm):
    s = copy.copy(system); s.remove_cm_motion = bool(cm)
    return s


def _dke_cm(system, v):
    """Kinetic energy the CMMotionRemover takes from velocities v: -|p|^2 / (2 M) over the mobile atoms (0 with the remover off)."""
    if not system.remove_cm_motion:
        return 0.0
    m = np.asarray(system.mass, dtype=float)
    p = (m[:, None] * v).sum(0)
    return -float(p @ p) / (2.0 * m.sum())


def _E(e):
    return e.potential_energy() + e.kinetic_energy()


def _start(Engine, system, v=None):
    """A start state the first-step block leaves as it is.  That block constrains positions and velocities and books nothing; the
    fixtures' positions satisfy the constraints to the 1e-8 they were written with, and the block's SHAKE polish of them moves the
    potential energy of the toluene box by 2.6e-5 kJ/mol -- outside the ledger by definition, and far above its 1e-9 tolerance.  So the
    ledgers below start from the fixture after one first-step block (an engine with a switch of 0 steps runs that block and nothing else)."""
    g = Engine(system, integrators.generateNCMCIntegrator(nstepsNC=0, dt=0.002, temperature=300.0, seed=1).to_data(precision=1))
    if v is None:
        g.set_velocities_to_temperature(300.0, seed=5)
    else:
        g.set_velocities(v)
    g.step(1)
    x, v = g.get_positions(), g.get_velocities()
    g.close()
    return x, v


def _ledger_run(g, system, nsteps, tol, slack_rel, o=None, move_at=None, mover=None):
    """Steps g (and the oracle o) one step at a time; after every step checks heat against the oracle, the shadow work against the
    oracle-derived dE - dW - dQ - sum dKE_cm, and the identity on the engine's own numbers.  Returns the largest |shadow|, |heat|."""
    E0g, cm_g = _E(g), 0.0
    E0o, cm_o = (_E(o), 0.0) if o is not None else (0.0, 0.0)
    big_s = big_q = 0.0
    for k in range(nsteps):
        if move_at is not None and k == move_at:
            x = mover(g.get_positions())
            g.set_positions(x)
            if o is not None:
                o.set_positions(x)
        cm_g += _dke_cm(system, g.get_velocities())
        g.step(1)
        W, S, Q = g.get_global("protocol_work"), g.get_global("shadow_work"), g.get_global("heat")
        Eg = _E(g)
        bound = tol * max(1.0, abs(W)) + slack_rel * abs(Eg)
        resid = (Eg - E0g) - W - S - Q - cm_g
        print("step %2d engine: W %+.9f shadow %+.9f heat %+.9f sum dKE_cm %+.9f residual %+.3e (bound %.3e)" % (k + 1, W, S, Q, cm_g, resid, bound))
        assert abs(resid) <= bound, ("ledger", k + 1, resid, bound)
        if o is not None:
            cm_o += _dke_cm(system, o.get_velocities())
            o.step(1)
            Wo, Qo = o.get_global("protocol_work"), o.get_global("heat")
            So = (_E(o) - E0o) - Wo - Qo - cm_o
            print("        oracle: W %+.9f shadow %+.9f heat %+.9f   d heat %+.3e d shadow %+.3e" % (Wo, So, Qo, Q - Qo, S - So))
            assert abs(Q - Qo) <= tol * max(1.0, abs(Wo)), ("heat", k + 1, Q, Qo)
            assert abs(S - So) <= tol * max(1.0, abs(Wo)) + slack_rel * abs(Eg), ("shadow", k + 1, S, So)
        big_s, big_q = max(big_s, abs(S)), max(big_q, abs(Q))
    return big_s, big_q


@pytest.mark.parametrize("cm", [False, True])
@pytest.mark.parametrize("precision,tol,dt", CASES)
def test_heat_and_shadow_work_match_the_oracle(Engine, oracle_mod, tol_box, precision, tol, dt, cm):
    """Tests 1 and 2 of the issue: heat after every step; shadow work against dE - dW - dQ - sum dKE_cm of the oracle."""
    s, v = tol_box
    s = _cm(s, cm)
    data = _integ(dt).to_data(precision=precision)
    assert data.measure_shadow_work == 1 and data.measure_heat == 1
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    x, v = _start(Engine, s, v)
    g.set_positions(x); o.set_positions(x); g.set_velocities(v); o.set_velocities(v)
    big_s, big_q = _ledger_run(g, s, 12, tol, 0.0 if precision else 5e-7, o=o)
    assert big_q > 1e-3 and big_s > 1e-3   # (there is something to compare)
    g.close()


def _frozen(s, v):
    lig = np.arange(15)
    near = systems.nearest_molecules(s, lig, 120, exclude_idx=lig)
    sf = systems.freeze_except(s, np.concatenate([lig, near]))
    return sf, v * (sf.mass[:, None] > 0)


def _tol_parm():
    prm = amber.read_prmtop(os.path.join(GOLDEN, "TOL-parm.prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "TOL-parm.inpcrd"))
    return amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=list(range(15)), nonbonded_method="NoCutoff")


@pytest.mark.parametrize("kind", ["all_mobile", "mostly_frozen", "pme", "nocutoff"])
@pytest.mark.parametrize("precision,tol,dt", CASES)
def test_ledger_closes_on_the_engines_own_numbers(Engine, tol_box, precision, tol, dt, kind):
    """Test 3: the identity from blues_get_energy and the three globals, no oracle involved."""
    s, v = tol_box
    if kind == "mostly_frozen":
        s, v = _frozen(s, v)
    elif kind == "pme":
        s = systems.with_reciprocal_space(s)
    elif kind == "nocutoff":
        s, v = _tol_parm(), None
    g = Engine(s, _integ(dt).to_data(precision=precision))
    x, v = _start(Engine, s, v)
    g.set_positions(x); g.set_velocities(v)
    big_s, big_q = _ledger_run(g, s, 12, tol, 0.0 if precision else 5e-7)
    assert big_s > 0.0 and big_q > 0.0
    g.close()


@pytest.mark.parametrize("program", ["RVOHOVR", "nprop2", "move"])
def test_other_programs(Engine, oracle_mod, tol_box, program):
    """Test 4, double precision: the class default splitting, nprop = 2 inside the prop window, a switch with a ligand rotation at the
    middle step -- the identity and equality with the oracle-derived value.  (CM removal off: with nprop > 1 the remover acts at the
    head of every pass, which velocities taken between steps do not show.)"""
    s, v = tol_box
    s = _cm(s, False)
    lig = np.arange(15)
    kw = {"RVOHOVR": dict(splitting="R V O H O V R"), "nprop2": dict(splitting="H V R O R V H", nprop=2, prop_lambda=0.3), "move": {}}[program]
    data = _integ(0.002, **kw).to_data(precision=1)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    x, v = _start(Engine, s, v)
    g.set_positions(x); o.set_positions(x); g.set_velocities(v); o.set_velocities(v)
    mover = None
    if program == "move":
        mv = moves.RandomLigandRotationMove(lig, s.mass[lig], random_state=70)

        def mover(x):   # (the Move's own geometry -- a random rotation about the ligand's centre of mass -- applied through set_positions)
            x = x.copy(); x[lig] = mv.propose(x[lig])
            return x
    # (the work of the Move is protocol work -- perturbed_pe - unperturbed_pe -- so the ledger's baseline moves with it: _ledger_run
    # keeps its baseline from before the Move, and dW carries the jump)
    big_s, _ = _ledger_run(g, s, 12, 1e-9, 0.0, o=o, move_at=6 if program == "move" else None, mover=mover)
    assert big_s > 1e-3
    if program == "nprop2":
        assert g.get_global("nprop") == 2.0
    g.close()


def test_batch_members_equal_lone_chains_bit_for_bit(Engine, tol_box, tune):
    """Test 5: eight members with their own seeds, against each one alone; a batch mixing measuring and plain members is refused."""
    from blues_amd.engine import EngineError, NativeBatch
    s, v = tol_box
    R, n = 8, 12
    tune(assume_batch=R)
    rng = np.random.RandomState(11)
    vels = [v * (1.0 + 0.05 * r) + 0.01 * rng.standard_normal(v.shape) * (s.mass[:, None] > 0) for r in range(R)]

    def make(shadow=True):
        out = []
        for r in range(R):
            g = Engine(s, _integ(0.002, nsteps=n, seed=100 + r, shadow=shadow).to_data(precision=0, replica=r))
            g.set_velocities(vels[r]); out.append(g)
        return out
    solo = make()
    for g in solo:
        g.step(5); g.step(n - 5)
    bat = make()
    B = NativeBatch(bat)
    B.step(5); B.step(n - 5)
    assert B.stats()["fallback_steps"] == 0
    B.prefetch_energies()
    for r in range(R):
        for k in ("heat", "shadow_work", "protocol_work"):
            a, b = solo[r].get_global(k), bat[r].get_global(k)
            assert a == b, (r, k, a, b)
        assert np.array_equal(solo[r].get_positions(), bat[r].get_positions())
        assert abs(solo[r].get_global("shadow_work")) > 1e-3
    assert solo[0].get_global("shadow_work") != solo[1].get_global("shadow_work")
    B.close()
    mixed = make()[:1] + make(shadow=False)[1:2]
    with pytest.raises(EngineError, match="measure_shadow_work"):
        NativeBatch(mixed).step(1)


def test_drivers_use_the_measured_shadow_work(Engine, tol_box):
    """Test 6: one BLUESSimulation and one BatchedBLUESSimulation iteration with measure_shadow_work=True; reset() semantics."""
    from blues_amd.context import Simulation
    s, v = tol_box
    lig = np.arange(15)
    nsteps = 12

    def chain(r):
        integ = _integ(0.002, nsteps=nsteps, seed=500 + r)
        sim = Simulation(None, s, integ, precision="double", replica=r)
        sim.context.setVelocities(unit.Quantity(v * (1.0 + 0.05 * r), "nanometer/picosecond"))
        mover = moves.MoveEngine(moves.RandomLigandRotationMove(lig, s.mass[lig], random_state=70 + r))
        return simulation.BLUESSimulation(simulation.SimulationSet(sim), {"nstepsNC": nsteps, "moveStep": nsteps // 2, "nIter": 1}, mover)

    def check(c):
        e = c._ncmc_sim.context._engine
        W, S = e.get_global("protocol_work"), e.get_global("shadow_work")
        assert c.last["work_ncmc"] == -(W + S) / KT, (c.last, W, S)
        assert S != 0.0 and abs(S) > 1e-6
        return e

    c = chain(0)
    np.random.seed(1); c.currentIter = 0
    c._syncStatesMDtoNCMC(); c._stepNCMC(nsteps, nsteps // 2); c._acceptRejectMove()
    e = check(c)
    heat = e.get_global("heat")
    assert heat != 0.0
    e.reset()
    assert e.get_global("shadow_work") == 0.0 and e.get_global("heat") == heat and e.get_global("protocol_work") == 0.0
    e.set_global("shadow_work", 1.5); e.set_global("heat", -2.5)
    assert e.get_global("shadow_work") == 1.5 and e.get_global("heat") == -2.5

    bat = [chain(r) for r in range(3)]
    B = simulation.BatchedBLUESSimulation(bat)
    for r, cb in enumerate(bat):
        cb.currentIter = 0; cb._syncStatesMDtoNCMC()
    B._stepNCMC(nsteps, nsteps // 2)
    np.random.seed(2)
    B._decide_batched(300.0)
    for cb in bat:
        check(cb)
    B.close()


def test_a_box_edit_between_steps_restarts_the_bracket(Engine, tol_box):
    """U(x, box) changed from outside between two stepping calls is nobody's shadow work: the bracket restarts, and the identity closes
    over the steps after the edit as it did before (double precision, tolerance of test 3).  (A hand-set lambda restarts the bracket
    in the same way, but the next H op returns to the schedule's lambda and books the slot difference of the schedule: there is no
    identity to check across it.)"""
    s, v = tol_box
    s = _cm(s, False)
    x, v = _start(Engine, s, v)
    g = Engine(s, _integ(0.002).to_data(precision=1))
    g.set_positions(x); g.set_velocities(v)
    g.step(3)
    E_before = g.potential_energy()
    g.set_box(np.diag(np.asarray(g.get_box()).reshape(3, 3)) * 1.002)
    assert abs(g.potential_energy() - E_before) > 1e-3   # (the edit moves U by far more than the tolerance)
    E0, W0, S0, Q0 = _E(g), g.get_global("protocol_work"), g.get_global("shadow_work"), g.get_global("heat")
    for k in range(3):
        g.step(1)
        W, S, Q = g.get_global("protocol_work"), g.get_global("shadow_work"), g.get_global("heat")
        resid = (_E(g) - E0) - (W - W0) - (S - S0) - (Q - Q0)
        print("box edit, step %d after it: residual %+.3e" % (k + 1, resid))
        assert abs(resid) <= 1e-9 * max(1.0, abs(W)), (k + 1, resid)
    g.close()


@pytest.mark.parametrize("flags", [dict(measure_heat=1), dict(measure_shadow_work=1)])
def test_one_flag_alone(Engine, oracle_mod, tol_box, flags):
    """Heat alone (IntegratorData(measure_heat=1)) and shadow work without heat: the measured global equals the one of the engine that
    measures both, the other reads 0 and refuses a set."""
    import dataclasses
    from blues_amd.engine import EngineError
    s, v = tol_box
    x, v = _start(Engine, s, v)
    both = _integ(0.002).to_data(precision=1)
    one = dataclasses.replace(both, measure_shadow_work=flags.get("measure_shadow_work", 0), measure_heat=flags.get("measure_heat", 0))
    out = []
    for d in (both, one):
        g = Engine(s, d); g.set_positions(x); g.set_velocities(v); g.step(4)
        out.append((g.get_global("heat"), g.get_global("shadow_work"), g.get_global("protocol_work"))); last = g
    assert out[0][2] == out[1][2]
    if "measure_heat" in flags:
        assert out[1][0] == out[0][0] != 0.0 and out[1][1] == 0.0
        with pytest.raises(EngineError, match="shadow work is not measured"):
            last.set_global("shadow_work", 1.0)
    else:
        assert out[1][1] == out[0][1] != 0.0 and out[1][0] == 0.0


@pytest.mark.parametrize("kind,precision", [("pme", 0), ("pme", 1), ("nocutoff", 0), ("nocutoff", 1), ("box", 1)])
def test_batch_equals_solo_other_systems_and_batch_reset(Engine, tol_box, tune, kind, precision):
    """The batched ledger sums over PME and NoCutoff members and in double precision, bit for bit against lone chains; then
    blues_batch_reset: shadow_work and protocol_work go, heat stays."""
    from blues_amd.engine import NativeBatch
    s, v = tol_box
    if kind == "pme":
        s = systems.with_reciprocal_space(s)
    elif kind == "nocutoff":
        s, v = _tol_parm(), None
    R, n = 4, 6
    tune(assume_batch=R)
    x, v = _start(Engine, s, v)

    def make():
        out = []
        for r in range(R):
            g = Engine(s, _integ(0.002, nsteps=n, seed=100 + r).to_data(precision=precision, replica=r))
            g.set_positions(x); g.set_velocities(v * (1.0 + 0.05 * r)); out.append(g)
        return out
    solo = make()
    for g in solo:
        g.step(n)
    bat = make()
    B = NativeBatch(bat)
    B.step(n)
    for r in range(R):
        for k in ("heat", "shadow_work", "protocol_work"):
            assert solo[r].get_global(k) == bat[r].get_global(k), (r, k, solo[r].get_global(k), bat[r].get_global(k))
        assert solo[r].get_global("shadow_work") != 0.0
    heats = [g.get_global("heat") for g in bat]
    B.reset_all()
    for r, g in enumerate(bat):
        assert g.get_global("shadow_work") == 0.0 and g.get_global("protocol_work") == 0.0 and g.get_global("heat") == heats[r] != 0.0
    B.close()


def test_flags_off_reads_zero_and_refuses_the_set(Engine, tol_box):
    """Test 7."""
    from blues_amd.engine import EngineError
    s, v = tol_box
    g = Engine(s, _integ(0.002, shadow=False).to_data(precision=1))
    g.set_velocities(v)
    g.step(3)
    assert g.get_global("heat") == 0.0 and g.get_global("shadow_work") == 0.0
    with pytest.raises(EngineError, match="shadow work is not measured"):
        g.set_global("shadow_work", 1.0)
    g.close()


def test_engine_refuses_the_flags_with_a_switching_mode(Engine, tol_box):
    import ctypes
    from blues_amd import _abi, _lib
    s, v = tol_box
    d = _abi.IntegratorData(timestep=0.002, temperature=300.0, nsteps_neq=2, lambda_sterics=np.ones(3), lambda_electrostatics=np.ones(3),
                            switching_mode=_abi.SWITCH_VV)
    desc, keep = d.to_desc()
    desc.measure_shadow_work = 1   # (past the host mirror's own check)
    sd, skeep = s.to_desc()
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.blues_engine_create(ctypes.byref(sd), ctypes.byref(desc), 0, ctypes.byref(h)) != 0
    assert b"measure_shadow_work" in lib.blues_last_error(None)
