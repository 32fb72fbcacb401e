"""GPU suite: GB-OBC implicit solvent of NoCutoff Systems (kernels_gb.h) against the numpy reference tests/gb_reference.py, which
tests/test_implicit_solvent_cpu.py pins by itself; everything that is not GB against the CPU oracle (which has no GB) and against the
same System's engine without implicit solvent.  Bars as tests/test_gpu_nocutoff.py: 1e-10 double, 1e-5 mixed."""
import copy
import dataclasses
import os

import numpy as np
import pytest

import gb_reference as gbr
import symmetry as sym
from blues_amd import _abi, amber, integrators, moves, simulation, unit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYSTEMS = {"TOL-parm": list(range(15)), "vacDivaline": list(range(22, 32))}
LAMBDAS = ((1.0, 1.0), (0.5, 0.3), (0.05, 0.0), (0.0, 0.0))
PRECISIONS = [(1, 1e-10), (0, 1e-5)]


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


_cache = {}


def gb_system(name, model="OBC2"):
    if (name, model) not in _cache:
        prm = amber.read_prmtop(os.path.join(GOLDEN, name + ".prmtop"))
        pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, name + ".inpcrd"))
        _cache[(name, model)] = amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=SYSTEMS[name], nonbonded_method="NoCutoff",
                                                        implicit_solvent=model)
    return copy.deepcopy(_cache[(name, model)])


def plain(s):
    return dataclasses.replace(s, implicit_solvent=None)


def mostly_frozen(s, radius=0.8):
    """TOL-parm with only the molecules that have an atom within `radius` of the ligand mobile."""
    lig = np.asarray(s.alchemical_atoms)
    d = np.sqrt(((s.positions[:, None, :] - s.positions[None, lig, :]) ** 2).sum(-1)).min(1)
    s = copy.deepcopy(s)
    res = np.asarray(s.residue_of_atom)
    near = np.isin(res, np.unique(res[d <= radius]))      # (whole molecules: a constraint cannot join a mobile atom to a frozen one)
    s.mass = np.where(near, s.mass, 0.0)
    assert 15 < (s.mass > 0).sum() < 0.5 * s.n_atoms      # (mostly frozen: more than half of the atoms)
    return s


def ion_pair(r, rho=(0.15, 0.2), S=(0.8, 0.85), q=(1.0, -0.7), model=_abi.GB_OBC2):
    """Two ions, no Lennard-Jones, no bonds; the second one alchemical."""
    x = np.array([[0.3, -0.2, 0.1], [0.3, -0.2, 0.1]]) + np.array([[0.0, 0, 0], [r * 0.6, r * 0.0, r * 0.8]])
    return _abi.SystemData(box=np.zeros(3), mass=np.array([22.99, 35.45]), charge=np.array(q, dtype=np.float64), sigma=np.array([0.3, 0.3]), epsilon=np.zeros(2),
                           alchemical_atoms=np.array([1], np.int32), nonbonded_method=_abi.NB_NOCUTOFF, positions=x,
                           implicit_solvent=_abi.ImplicitSolventData(model, np.array(rho, dtype=np.float64), np.array(S, dtype=np.float64)))


def _integ(nsteps=20, dt=0.002, seed=7):
    return integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=dt, temperature=300.0, seed=seed)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


def _check_parity(Engine, oracle_mod, s, precision, tol):
    """Terms [8], [9], the total and the forces against oracle + numpy GB at the four lambda pairs; in double precision terms [0..7]
    are bit-identical to the engine without GB (the GB kernels touch none of their partials).  forces - GB forces cannot be: k_finalize
    adds the GB force to f + f_alch on the device and rounds the sum, so (total - reference GB force) differs from the plain engine's
    force by that rounding and by the reference's own.  It is held to 1e-12 of the largest force instead (seen: 2e-16 to 9e-14, the
    largest on the 975 all-mobile atoms of TOL-parm; printed below)."""
    data = _integ().to_data(precision=precision)
    g, gp, o = Engine(s, data), Engine(plain(s), data), oracle_mod.Oracle(plain(s), data)
    coef = gbr.system_coefficients(s)
    mob = s.mass > 0
    for ls, le in LAMBDAS:
        eo, fo, to = o.energy_forces(ls, le)
        pol, sa, fgb = gbr.evaluate(coef, le)
        for e in (g, gp):
            e.set_global("lambda_sterics", ls); e.set_global("lambda_electrostatics", le)
        tg, tp = g.energy_terms(), gp.energy_terms()
        print("GB parity n=%d precision=%d (%.2f, %.2f): polar %.12g ref %.12g, surface %.12g ref %.12g" % (s.n_atoms, precision, ls, le, tg[8], pol, tg[9], sa))
        assert abs(tg[8] - pol) <= tol * max(abs(pol), 1.0), (ls, le, tg[8], pol)
        assert abs(tg[9] - sa) <= tol * max(abs(sa), 1.0), (ls, le, tg[9], sa)
        for k in range(8):
            assert abs(tg[k] - to[k]) <= tol * max(abs(to[k]), 1.0), (ls, le, k, tg[k], to[k])
        assert tp[8] == 0.0 and tp[9] == 0.0
        if precision == 1:
            assert np.array_equal(tg[:8], tp[:8]), (tg[:8], tp[:8])
        ref = eo + pol + sa
        assert abs(tg.sum() - ref) <= tol * max(abs(ref), 1.0), (ls, le, tg.sum(), ref)
        assert abs(g.potential_energy() - ref) <= tol * max(abs(ref), 1.0)
        fg, fp = g.get_forces(), gp.get_forces()
        fref = fo + fgb
        print("   forces: total rel %.3e, GB part rel-to-total %.3e" % (_rel(fg[mob], fref[mob]), np.abs((fg - fp)[mob] - fgb[mob]).max() / np.abs(fref[mob]).max()))
        assert _rel(fg[mob], fref[mob]) <= tol, (ls, le, _rel(fg[mob], fref[mob]))
        assert np.abs((fg - fp)[mob] - fgb[mob]).max() <= tol * np.abs(fref[mob]).max()
        if precision == 1:
            rest = np.abs((fg - fgb)[mob] - fp[mob]).max() / np.abs(fg[mob]).max()
            print("   forces - GB forces against the plain engine's: %.3e of the largest force (bar 1e-12)" % rest)
            assert rest <= 1e-12, (ls, le, rest)
        assert np.all(fg[~mob] == 0.0)
    g.close(); gp.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("case", ["overlapping", "far", "engulfed", "obc1"])
def test_ion_pairs(Engine, oracle_mod, case, precision, tol):
    s = {"overlapping": lambda: ion_pair(0.3), "far": lambda: ion_pair(5.0), "obc1": lambda: ion_pair(0.3, model=_abi.GB_OBC1),
         "engulfed": lambda: ion_pair(0.1, rho=(0.06, 0.3), S=(0.8, 0.9))}[case]()
    o, sc = s.implicit_solvent.radius - 0.009, s.implicit_solvent.scale * (s.implicit_solvent.radius - 0.009)
    r = np.linalg.norm(s.positions[1] - s.positions[0])
    if case == "engulfed":
        assert o[0] < sc[1] - r
    if case == "far":
        assert r > 10 * sc.max()
    if case in ("overlapping", "obc1"):
        assert abs(r - sc[1]) < o[0] < r + sc[1]
    _check_parity(Engine, oracle_mod, s, precision, tol)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("case", ["vacDivaline", "vacDivaline-OBC1", "TOL-parm", "TOL-parm-frozen"])
def test_parity(Engine, oracle_mod, case, precision, tol):
    s = gb_system(case.split("-OBC1")[0].replace("-frozen", ""), "OBC1" if case.endswith("OBC1") else "OBC2")
    if case.endswith("frozen"):
        s = mostly_frozen(s)
    _check_parity(Engine, oracle_mod, s, precision, tol)


def _neighbours(s, atoms):
    pairs = np.concatenate([np.asarray(s.bond_atoms).reshape(-1, 2), np.asarray(s.constraint_atoms).reshape(-1, 2)])
    inside = set(int(a) for a in atoms)
    return sorted({int(b if a in inside else a) for a, b in pairs if (int(a) in inside) != (int(b) in inside)})


def test_gb_force_is_the_gradient_of_the_engines_energy(Engine):
    """Double precision, vacDivaline at lambda = (0.45, 0.2): total force - plain engine's force against central differences (h = 1e-5 nm)
    of terms[8] + terms[9], on two alchemical atoms, the atom the alchemical region is bonded to and one bonded to that, and the two farthest ones.  The bar is ten times
    the gap the numpy reference shows between ITS forces and ITS central differences at the same h and atoms (truncation of the
    difference quotient, not the engine's: 7.8e-7 kJ/mol/nm on these atoms for the reference and for the engine alike, printed by the test)."""
    s = gb_system("vacDivaline")
    near = _neighbours(s, SYSTEMS["vacDivaline"])
    rest = [a for a in range(s.n_atoms) if a not in near and a not in SYSTEMS["vacDivaline"]]
    dist = np.sqrt(((s.positions[rest][:, None, :] - s.positions[None, SYSTEMS["vacDivaline"], :]) ** 2).sum(-1)).min(1)
    second = [a for a in _neighbours(s, SYSTEMS["vacDivaline"] + near) if a not in near]
    bonded = (near + second)[:2]                     # (the region hangs on one atom: that atom and one bonded to it)
    rest = [a for a in rest if a not in bonded]
    dist = np.sqrt(((s.positions[rest][:, None, :] - s.positions[None, SYSTEMS["vacDivaline"], :]) ** 2).sum(-1)).min(1)
    atoms = [22, 27] + bonded + [rest[i] for i in np.argsort(dist)[-2:]]
    assert len(set(atoms)) == 6
    le, h = 0.2, 1e-5
    data = _integ().to_data(precision=1)
    g, gp = Engine(s, data), Engine(plain(s), data)
    for e in (g, gp):
        e.set_global("lambda_sterics", 0.45); e.set_global("lambda_electrostatics", le)
    f_gb = g.get_forces() - gp.get_forces()

    def e_engine(x):
        g.set_positions(x); t = g.energy_terms(); return t[8] + t[9]

    def e_numpy(x):
        pol, sa, _ = gbr.evaluate(gbr.system_coefficients(s, x), le); return pol + sa

    def differences(energy):
        out = np.zeros((6, 3))
        for n, a in enumerate(atoms):
            for k in range(3):
                xp = s.positions.copy(); xp[a, k] += h
                xm = s.positions.copy(); xm[a, k] -= h
                out[n, k] = -(energy(xp) - energy(xm)) / (2.0 * h)
        return out
    gap_ref = np.abs(differences(e_numpy) - gbr.evaluate(gbr.system_coefficients(s), le)[2][atoms]).max()
    gap = np.abs(differences(e_engine) - f_gb[atoms]).max()
    print("GB force vs central differences: engine %.3e, numpy reference %.3e kJ/mol/nm (max |f_gb| %.3e)" % (gap, gap_ref, np.abs(f_gb).max()))
    assert gap <= 10.0 * gap_ref, (gap, gap_ref)
    g.close(); gp.close()


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_gb_forces_sum_to_zero(Engine, name):
    s = gb_system(name)
    data = _integ().to_data(precision=1)
    g, gp = Engine(s, data), Engine(plain(s), data)
    for le in (1.0, 0.3):
        for e in (g, gp):
            e.set_global("lambda_electrostatics", le)
        f = g.get_forces() - gp.get_forces()
        assert np.abs(f).max() > 1.0
        assert np.abs(f.sum(0)).max() <= 1e-10 * np.abs(f).max(), (le, f.sum(0), np.abs(f).max())
    g.close(); gp.close()


@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("precision,tol", [(1, 1e-9), (0, 1e-5)])
def test_work_of_every_step(Engine, oracle_mod, name, precision, tol):
    """20 steps of "H V R O R V H", one at a time: a step's work is [U(x0; L+1) - U(x0; L)] + [U(x1; L+2) - U(x1; L+1)] at its first and
    last positions; the part that is not GB from the oracle, the GB part from the numpy coefficients E1, E2.
    The switch starts from coordinates that satisfy the HBonds constraints (two steps of the MD leg's engine from the fixture's): from
    the inpcrd's seven decimals the first step's work is not that sum at get_positions() -- by 8e-4 kJ/mol on TOL-parm, for the engine
    without GB and the oracle alike, which agree with each other -- so the identity would be tested on 19 steps instead of 20.
    Engine and reference share the positions the engine reached: this checks the energy coefficients E1, E2 and their booking as work,
    not the GB force that moved the atoms -- that rests on the parity and gradient tests above."""
    s = gb_system(name)
    md = Engine(dataclasses.replace(s, alchemical_atoms=np.zeros(0, np.int32)), integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=3).to_data(precision=precision))
    md.step(2)
    s.positions = md.get_positions()
    md.close()
    n = 20
    data = _integ(nsteps=n).to_data(precision=precision)
    ls, le = np.asarray(data.lambda_sterics), np.asarray(data.lambda_electrostatics)
    g, o = Engine(s, data), oracle_mod.Oracle(plain(s), data)
    o.set_velocities_to_temperature(300.0, 11)
    g.set_velocities(o.get_velocities())

    def du(x, a, b):
        o.set_positions(x)
        c = gbr.system_coefficients(s, x)
        e1, e2 = c["polar"][1] + c["surface"][1], c["polar"][2]
        return (o.energy_forces(ls[b], le[b])[0] - o.energy_forces(ls[a], le[a])[0]) + (le[b] - le[a]) * e1 + (le[b] ** 2 - le[a] ** 2) * e2
    x0, w_prev, got, want = g.get_positions(), 0.0, [], []
    for k in range(n):
        g.step(1)
        x1, w = g.get_positions(), g.get_global("protocol_work")
        got.append(w - w_prev); want.append(du(x0, 2 * k, 2 * k + 1) + du(x1, 2 * k + 1, 2 * k + 2))
        x0, w_prev = x1, w
    got, want = np.array(got), np.array(want)
    scale = max(1.0, np.abs(np.cumsum(want)).max())
    print("GB work per step %s precision=%d: max |dW - dU| %.3e, cumulative %.3e, scale %.3e" % (name, precision, np.abs(got - want).max(), np.abs(np.cumsum(got) - np.cumsum(want)).max(), scale))
    assert np.abs(want).max() > 1e-3
    assert np.abs(got - want).max() <= tol * scale
    assert np.abs(np.cumsum(got) - np.cumsum(want)).max() <= tol * scale
    g.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_energy_at_one_and_md_leg(Engine, precision, tol):
    s = gb_system("vacDivaline")
    g = Engine(s, _integ().to_data(precision=precision))
    g.set_global("lambda_sterics", 1.0); g.set_global("lambda_electrostatics", 1.0)
    total = lambda terms: sum((float(v) for v in terms), 0.0)        # (in term order, as the engine adds them: numpy's sum pairs them up)
    e11 = total(g.energy_terms())
    g.set_global("lambda_sterics", 0.5); g.set_global("lambda_electrostatics", 0.3)
    # (served by the spare (1, 1) slot of an evaluation at the current lambdas: the same fp64 partial sums, with the alchemical
    # pairs summed through another slot of the alchemical kernel than a direct evaluation's: four units in the last place of the total)
    same = lambda a, b: abs(a - b) <= 4.0 * np.finfo(float).eps * abs(b)
    assert same(g.potential_energy_at(1.0, 1.0), e11)
    t = g.energy_terms()
    assert same(g.potential_energy_at(1.0, 1.0), e11) and same(g.potential_energy(), total(t)) and abs(total(t) - e11) > 1e-3
    g.close()
    # the MD leg's engine: no alchemical atoms, the plain Langevin integrator
    md = dataclasses.replace(s, alchemical_atoms=np.zeros(0, np.int32))
    m = Engine(md, integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=3).to_data(precision=precision))
    pol, sa, fgb = gbr.evaluate(gbr.system_coefficients(md), 1.0)
    tm = m.energy_terms()
    assert abs(tm[8] - pol) <= tol * abs(pol) and abs(tm[9] - sa) <= tol * abs(sa)
    assert abs(tm.sum() - e11) <= 10 * tol * abs(e11)       # the alchemical engine at lambda = (1, 1) is the plain System
    mp = Engine(plain(md), integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=3).to_data(precision=precision))
    assert np.abs((m.get_forces() - mp.get_forces()) - fgb).max() <= tol * np.abs(m.get_forces()).max()
    m.set_velocities_to_temperature(300.0, 5); m.step(10)
    assert np.all(np.isfinite(m.get_positions())) and np.abs(m.get_positions() - s.positions).max() > 1e-4
    m.close(); mp.close()


def test_driver_with_implicit_solvent(Engine):
    """BLUESSimulation with a RandomLigandRotationMove on vacDivaline in implicit solvent: 2 iterations of 10 NCMC + 10 MD steps."""
    from blues_amd.context import Simulation
    s = gb_system("vacDivaline")
    md_sys = dataclasses.replace(s, alchemical_atoms=np.zeros(0, np.int32))
    lig = np.asarray(SYSTEMS["vacDivaline"])
    sim = Simulation(None, s, _integ(10, seed=21), precision="mixed")
    md = Simulation(None, md_sys, integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=22), precision="mixed")
    alch = Simulation(None, md_sys, integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=23), precision="mixed")
    md.context.setPositions(unit.Quantity(s.positions, "nanometer"))
    md.context.setVelocities(unit.Quantity(0.3 * np.random.RandomState(2).standard_normal((s.n_atoms, 3)), "nanometer/picosecond"))
    mover = moves.MoveEngine(moves.RandomLigandRotationMove(lig, s.mass[lig], random_state=24))
    b = simulation.BLUESSimulation(simulation.SimulationSet(sim, md=md, alch=alch), {"nstepsNC": 10, "moveStep": 5, "nIter": 2, "nstepsMD": 10}, mover,
                                   rng=np.random.RandomState(25))
    b.run()
    assert b.accept + b.reject == 2
    assert np.isfinite(b.last["protocol_work"]) and np.isfinite(b.last["correction"]) and np.isfinite(b.last["log_accept"]), b.last
    assert sim.context._engine.energy_terms()[8] < 0.0 and md.context._engine.energy_terms()[8] < 0.0
    assert np.all(np.isfinite(md.context._engine.get_positions()))


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("name,R", [("vacDivaline", 3), ("TOL-parm", 2)])
def test_batch_equals_lone_chain(Engine, oracle_mod, name, R, precision, tol):
    from blues_amd.engine import NativeBatch
    s, n = gb_system(name), 15
    o = oracle_mod.Oracle(plain(s), _integ().to_data(precision=precision))
    starts = []
    for r in range(R):
        o.set_velocities_to_temperature(300.0, 100 + r); starts.append(o.get_velocities())

    def make(r):
        e = Engine(s, _integ(nsteps=n, seed=40 + r).to_data(precision=precision, replica=r))
        e.set_velocities(starts[r])
        return e
    lone = []
    for r in range(R):
        e = make(r)
        w = e.run_switch(n, trace=True)
        lone.append((w, e.get_positions(), e.get_velocities()))
        e.close()
    assert len({tuple(l[0]) for l in lone}) == R
    engs = [make(r) for r in range(R)]
    batch = NativeBatch(engs)
    k0 = [e.stats()["kernel_launches"] for e in engs]
    _, w = batch.step(n, trace=True)
    for r in range(R):
        assert np.array_equal(w[r], lone[r][0]), r
        assert np.array_equal(engs[r].get_positions(), lone[r][1]) and np.array_equal(engs[r].get_velocities(), lone[r][2]), r
    st = batch.stats()
    assert st["fallback_steps"] == 0 and st["lockstep_steps"] > 0, st
    assert len({e.stats()["kernel_launches"] - k for e, k in zip(engs, k0)}) == 1
    # the batched energy evaluation (the driver's prefetch: one set of launches, one gather that carries the GB partials too)
    # against oracle + numpy GB at every member's own coordinates
    for e in engs:
        e.reset()
    own = [e.stats()["own_energy_evaluations"] for e in engs]
    batch.prefetch_energies(potential=True, kinetic=False)
    assert batch.stats()["batched_energy_evaluations"] >= 1
    for e, k in zip(engs, own):
        x = e.get_positions(); o.set_positions(x)
        pol, sa, _ = gbr.evaluate(gbr.system_coefficients(s, x), 1.0)
        ref = o.energy_forces(1.0, 1.0)[0] + pol + sa
        assert abs(e.potential_energy() - ref) <= tol * max(1.0, abs(ref)), (e.potential_energy(), ref)
        assert e.stats()["own_energy_evaluations"] == k          # served from the prefetch
    batch.close()
    for e in engs:
        e.close()


def test_batch_refuses_members_with_and_without_gb(Engine):
    from blues_amd.engine import EngineError, NativeBatch
    s = gb_system("vacDivaline")
    a = Engine(s, _integ().to_data(precision=0))
    b = Engine(plain(s), _integ().to_data(precision=0, replica=1))
    try:
        for pair in ([a, b], [b, a]):
            with pytest.raises(EngineError, match="implicit solvent"):
                NativeBatch(pair)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("transform", ["scatter", "rotate"])
def test_symmetry(Engine, transform, precision, tol):
    """Permuted atom order; a rigid rotation plus translation (NoCutoff has no lattice: exact up to rounding).  Bars of
    tests/test_gpu_symmetry.py for its NoCutoff rows: 1e-10 double, 1e-5 mixed, energies relative to max(|E|, 1), forces to max |f|."""
    s = gb_system("vacDivaline")
    if transform == "scatter":
        perm = sym.scatter_perm(s.n_atoms, 11)
        s2, _, m = sym.permute_atoms(s, None, perm)
        s2 = dataclasses.replace(s2, implicit_solvent=s.implicit_solvent.subset(perm))      # (the helper permutes the per-atom arrays it knows)
    else:
        s2, _, m = sym.rotate(s, None, sym.rotation_matrix([0.3, -1.0, 0.5], 2.1), (0.7, -1.3, 0.4))
    data = _integ().to_data(precision=precision)
    g, g2 = Engine(s, data), Engine(s2, data)
    for ls, le in LAMBDAS:
        for e in (g, g2):
            e.set_global("lambda_sterics", ls); e.set_global("lambda_electrostatics", le)
        t0, t1 = g.energy_terms(), g2.energy_terms()
        assert t0[8] < 0.0 and t0[9] > 0.0
        res = [abs(t1[k] - t0[k]) / max(abs(t0[k]), 1.0) for k in range(10)]
        f0, f1 = g.get_forces(), m.vectors(g2.get_forces())
        print("GB symmetry %s precision=%d (%.2f, %.2f): energy %.3e forces %.3e" % (transform, precision, ls, le, max(res), _rel(f1, f0)))
        assert max(res) <= tol, (ls, le, res)
        assert _rel(f1, f0) <= tol
    g.close(); g2.close()


def _bad(tol_box):
    s = gb_system("vacDivaline")
    gb = s.implicit_solvent
    periodic, _ = tol_box
    small = copy.deepcopy(gb); small.radius[3] = 0.009
    return [
        ("NoCutoff", dataclasses.replace(periodic, implicit_solvent=_abi.ImplicitSolventData(2, np.full(periodic.n_atoms, 0.15), np.full(periodic.n_atoms, 0.8))), {}),
        ("radius", dataclasses.replace(s, implicit_solvent=small), {}),
        ("dielectric", dataclasses.replace(s, implicit_solvent=dataclasses.replace(gb, solvent_dielectric=-1.0)), {}),
        ("model 3", dataclasses.replace(s, implicit_solvent=dataclasses.replace(gb, model=3)), {}),
        ("custom forces", dataclasses.replace(s, custom_pair_mode=1), {}),
        ("custom forces", dataclasses.replace(s, centroid_bonds=(([0, 1], [1.0, 1.0], [20], [1.0], 10.0),)), {}),
        ("annihilate_electrostatics", dataclasses.replace(s, annihilate_electrostatics=False), {}),
        ("measure_shadow_work / measure_heat", s, {"measure_shadow_work": 1}),
        ("measure_shadow_work / measure_heat", s, {"measure_heat": 1}),
    ]


@pytest.mark.parametrize("case", range(9))
def test_creation_errors_of_the_library(Engine, tol_box, monkeypatch, case):
    """blues_engine_create_gb's own checks: the wrapper's check is switched off, so the descriptor reaches the C-ABI as a foreign caller's."""
    from blues_amd.engine import EngineError
    match, s, flags = _bad(tol_box)[case]
    data = _integ().to_data(precision=0)
    for k, v in flags.items():
        setattr(data, k, v)
    with pytest.raises(EngineError, match=match):      # the wrapper's own refusal
        Engine(s, data)
    monkeypatch.setattr(_abi.SystemData, "check_implicit_solvent", lambda self, integrator=None: None)
    monkeypatch.setattr(_abi.SystemData, "check_custom_forces", lambda self: None)
    with pytest.raises(EngineError, match=match):      # the library's
        Engine(s, data)


def test_library_refuses_null_arrays(Engine):
    import ctypes
    from blues_amd import _lib
    lib = _lib.load()
    s = gb_system("vacDivaline")
    sd, keep_s = s.to_desc()
    idesc, keep_i = _integ().to_data(precision=0).to_desc()
    gd, keep_g = s.implicit_solvent.to_desc()
    gd.scale = None
    h = ctypes.c_void_p()
    assert lib.blues_engine_create_gb(ctypes.byref(sd), ctypes.byref(idesc), ctypes.byref(gd), 0, ctypes.byref(h)) != 0
    assert "radius / scale arrays" in lib.blues_last_error(None).decode() and not h.value
    # NULL descriptor: blues_engine_create
    assert lib.blues_engine_create_gb(ctypes.byref(sd), ctypes.byref(idesc), None, 0, ctypes.byref(h)) == 0
    t = (ctypes.c_double * 10)()
    x = np.ascontiguousarray(s.positions)
    assert lib.blues_set_positions(h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), s.n_atoms) == 0
    assert lib.blues_get_energy_terms(h, t) == 0 and t[8] == 0.0 and t[9] == 0.0
    lib.blues_engine_destroy(h)


def test_launches_per_pass(Engine):
    """A GB engine adds its three kernels to a force pass and two to an energy evaluation; the plain engine's counts are what they were."""
    s = gb_system("vacDivaline")
    counts = {}
    for key, sysd in (("gb", s), ("plain", plain(s))):
        g = Engine(sysd, _integ().to_data(precision=0))
        g.set_velocities_to_temperature(300.0, 3)
        g.step(2)
        a = g.stats(); g.step(10); b = g.stats()
        counts[key] = ((b["kernel_launches"] - a["kernel_launches"]), b["force_passes"] - a["force_passes"])
        g.close()
    assert counts["gb"][1] == counts["plain"][1] == 10
    assert counts["gb"][0] - counts["plain"][0] == 3 * 10, counts
