"""GPU suite: the 'exact' alchemical PME treatment (SystemData.alchemical_pme_treatment = "exact"; kernels_pme.h: k_pme_exact_b in double
precision, the pruned in-LDS k_pme_exact_fast_b in mixed precision where the mobile atoms fit its cache -- the mostly frozen and the S23k cases below) against
the fp64 reference composed from the unchanged oracle (tests/exact_pme_reference.py): energies, terms and forces, the static + mobile +
alchemical meshes, the quadratic form in lambda_electrostatics, the work of a switch, the vanishing alchemical correction, batches, and
what the library refuses.  Tolerances are tests/test_gpu_pme.py's: 1e-10 (double) / 1e-5 (mixed) of max(|term|, 1) and of the largest
force; work 1e-9 / 1e-5 of max(1, max |W|)."""
import copy
import ctypes as C

import numpy as np
import pytest

import exact_pme_reference as xref
from blues_amd import _abi, integrators, systems

pytestmark = pytest.mark.gpu

LAMBDAS = ((1.0, 1.0), (0.5, 0.3), (0.0, 0.0), (0.2, 0.7))
FUNCS = {"lambda_sterics": "1 - 0.3*sin(3.141592653589793*lambda)", "lambda_electrostatics": "1 - 0.5*sin(3.141592653589793*lambda)"}   # tests/test_gpu_general_constraints.py
TOL = {1: 1e-10, 0: 1e-5}


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _integ(n=20, seed=7):
    return integrators.generateNCMCIntegrator(nstepsNC=n, dt=0.004, temperature=300.0, seed=seed)


def _exact(s):
    return systems.with_alchemical_pme_treatment(s, "exact")


def _system(name, tol_box):
    r = systems.with_reciprocal_space(tol_box[0])
    assert r.pme_grid == (9, 9, 9)
    if name == "methyl":      # one constraint cluster bonded to the environment: alchemical-environment exclusions and 1-4s, a charged background
        r = copy.copy(r); r.alchemical_atoms = np.array([0, 7, 8, 9], np.int32)
        assert abs(r.charge[r.alchemical_atoms].sum() - 0.078) < 5e-4
    if name == "corner":      # the ligand's centroid on a box corner: the alchemical stencil wraps the mesh on all three axes
        r = copy.copy(r); r.positions = r.positions - r.positions[:15].mean(0)
    return _exact(r)


@pytest.fixture(scope="module")
def cases(tol_box):
    """name -> (System, reference, {(ls, le): (E, F, terms)} at the System's positions): evaluated once, shared by both precisions."""
    out = {}
    for name in ("toluene", "methyl", "corner"):
        s = _system(name, tol_box)
        ref = xref.ExactPmeReference(s, openmp=True)
        out[name] = (s, ref, {lam: ref.evaluate(s.positions, *lam) for lam in LAMBDAS})
    return out


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def _compare(g, expect, tol, mobile=None):
    eo, fo, to = expect
    tg = g.energy_terms()
    gg, go = xref.group_terms(tg), xref.group_terms(to)
    print("groups (engine - reference):", " ".join("%.3e" % d for d in gg - go), " force rel:", end=" ")
    for k in range(len(go)):
        assert abs(gg[k] - go[k]) <= tol * max(abs(go[k]), 1.0), (k, gg[k], go[k])
    assert abs(tg.sum() - eo) <= tol * abs(eo)
    assert g.potential_energy() == pytest.approx(tg.sum(), rel=1e-14)
    f = g.get_forces()
    sel = slice(None) if mobile is None else mobile
    print("%.3e" % _rel(f[sel], fo[sel]))
    assert _rel(f[sel], fo[sel]) <= tol


def _assert_path(g, fast):
    """Which mesh kernel path served the alchemical class, from the counter the kernel keeps.  The pruned in-LDS pipeline serves mixed
    precision when the mobile and the alchemical atoms fit its atom cache (a few hundred; the environment's k_pme_fast has the same kind of
    limit); double precision and an all-mobile box take the general one."""
    st = g.stats()
    print("exact PME launches, fast / general:", st["exact_pme_fast_launches"], st["exact_pme_general_launches"])
    if fast:
        assert st["exact_pme_fast_launches"] > 0 and st["exact_pme_general_launches"] == 0
    else:
        assert st["exact_pme_general_launches"] > 0 and st["exact_pme_fast_launches"] == 0


# ---- 1. energies, terms, forces
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("name", ["toluene", "methyl", "corner"])
def test_energies_terms_and_forces_against_the_reference(Engine, cases, name, precision):
    s, ref, expect = cases[name]
    g = Engine(s, _integ().to_data(precision=precision))
    for (ls, le) in LAMBDAS:
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        _compare(g, expect[(ls, le)], TOL[precision])
    _assert_path(g, False)      # (975 mobile atoms)
    if name == "methyl":
        e1, e2 = ref.charge_coefficients(s.positions)
        assert abs(e1 - (-3.073)) < 2e-3 and abs(e2 - (-0.551)) < 2e-3       # (what the issue measured for this System)
    if precision == 1:
        # forces = -dE/dx by central differences on three ligand atoms.  Bound: the reference's own central difference at h = 1e-5 misses
        # its force by 7e-6 on 64 kJ/mol/nm (rounding of a 1.5e4 kJ/mol energy, 1e-11 / 2e-5, plus truncation); ten times that.
        ls, le = 0.5, 0.3
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        f = g.get_forces(); x0 = np.array(s.positions, dtype=np.float64); h = 1e-5
        for atom, axis in ((int(s.alchemical_atoms[0]), 0), (int(s.alchemical_atoms[1]), 1), (int(s.alchemical_atoms[-1]), 2)):
            xp, xm = x0.copy(), x0.copy(); xp[atom, axis] += h; xm[atom, axis] -= h
            g.set_positions(xp); ep = g.potential_energy()
            g.set_positions(xm); em = g.potential_energy()
            num = -(ep - em) / (2.0 * h)
            print("central difference:", atom, axis, f[atom, axis], num)
            assert abs(f[atom, axis] - num) <= 7e-5 * max(1.0, abs(num) / 64.0), (atom, axis, f[atom, axis], num)
    g.close()


# ---- 2. static + mobile + alchemical meshes
def _frozen(s):      # tests/test_gpu_energy_ledger.py::_frozen: the ligand and the 120 nearest atoms keep their mass
    lig = np.arange(15)
    near = systems.nearest_molecules(s, lig, 120, exclude_idx=lig)
    return systems.freeze_except(s, np.concatenate([lig, near]))


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("name", ["toluene", "corner"])
def test_mostly_frozen_box_static_mobile_and_alchemical_meshes(Engine, tol_box, name, precision):
    s = _frozen(_system(name, tol_box))
    ref = xref.ExactPmeReference(s, openmp=True)
    g = Engine(s, _integ().to_data(precision=precision))
    g.set_global("lambda_sterics", 0.5); g.set_global("lambda_electrostatics", 0.3)
    mob = s.mass > 0
    x = np.array(s.positions, dtype=np.float64)
    for rnd in range(2):
        _compare(g, ref.evaluate(x, 0.5, 0.3), TOL[precision], mobile=mob)
        x[mob] += np.random.RandomState(3).normal(scale=0.004, size=(int(mob.sum()), 3))
        g.set_positions(x)
    _assert_path(g, precision == 0)      # (135 mobile atoms: mixed precision runs the in-LDS pipeline, on a 9^3 mesh its blocks are the whole mesh)
    g.close()


@pytest.mark.parametrize("precision", [1, 0])
def test_frozen_alchemical_atoms_stay_in_the_alchemical_class(Engine, tol_box, precision):
    """The ligand frozen, the water mobile: the alchemical charges are in no static mesh, they are spread with the alchemical class every
    evaluation, and the mobile environment feels le q_j grad phi_alch."""
    s = systems.freeze_atoms(_system("toluene", tol_box), np.arange(15))
    ref = xref.ExactPmeReference(s, openmp=True)
    g = Engine(s, _integ().to_data(precision=precision))
    g.set_global("lambda_sterics", 0.5); g.set_global("lambda_electrostatics", 0.3)
    _compare(g, ref.evaluate(s.positions, 0.5, 0.3), TOL[precision], mobile=s.mass > 0)
    _assert_path(g, False)      # (960 mobile atoms)
    g.close()


def test_s23k_frozen_environment_mixed_precision(Engine):
    """Mesh 18 x 27 x 36, 275 mobile atoms: the environment's per-step launch and the alchemical class's both take the pruned in-LDS
    pipeline, which stats() reports from a counter the kernel keeps."""
    s, v = systems.s23k(mobile_atoms=275, frozen=True)
    s = _exact(systems.with_reciprocal_space(s))
    assert s.pme_grid == (18, 27, 36)
    ref = xref.ExactPmeReference(s, openmp=True)
    g = Engine(s, _integ().to_data(precision=0))
    g.set_global("lambda_sterics", 0.5); g.set_global("lambda_electrostatics", 0.3)
    _compare(g, ref.evaluate(s.positions, 0.5, 0.3), TOL[0], mobile=s.mass > 0)
    _assert_path(g, True)
    g.close()


# ---- 3. quadratic in lambda_electrostatics, on the device
@pytest.mark.parametrize("name", ["toluene", "methyl"])
def test_energy_is_quadratic_in_lambda_electrostatics(Engine, cases, name):
    s = cases[name][0]
    g = Engine(s, _integ().to_data(precision=1))
    u0, uh, u1, uq = (g.potential_energy_at(0.5, le) for le in (0.0, 0.5, 1.0, 0.3))
    e2 = 2.0 * (u1 - 2.0 * uh + u0); e1 = (u1 - u0) - e2
    print("parabola residual:", uq - (u0 + 0.3 * e1 + 0.09 * e2), "E1, E2:", e1, e2)
    assert abs(uq - (u0 + 0.3 * e1 + 0.09 * e2)) <= 1e-12 * abs(uq)
    assert abs(e2) > 0.1
    g.close()


# ---- 4. work of a switch
def _switch_integrator(n, seed=7):
    return integrators.AlchemicalExternalLangevinIntegrator(FUNCS, splitting="H V R O R V H", temperature=300.0, timestep=0.002, nsteps_neq=n, seed=seed)


def _start(Engine, system, v):
    """A start state the first-step block leaves as it is (tests/test_gpu_energy_ledger.py::_start): that block's SHAKE polish of the
    fixture's positions moves the potential energy by ~1e-5 kJ/mol, and the first H step is taken at the polished positions.  An engine
    with a switch of 0 steps runs that block and nothing else."""
    g = Engine(system, integrators.generateNCMCIntegrator(nstepsNC=0, dt=0.002, temperature=300.0, seed=1).to_data(precision=1))
    g.set_velocities(v)
    g.step(1)
    x, v = g.get_positions(), g.get_velocities()
    g.close()
    return x, v


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("name", ["toluene", "methyl"])
def test_work_of_a_switch_step_by_step(Engine, tol_box, cases, name, precision):
    s, ref, _ = cases[name]
    v = tol_box[1]
    n = 12
    data = _switch_integrator(n).to_data(precision=precision)
    ls, le = np.asarray(data.lambda_sterics), np.asarray(data.lambda_electrostatics)
    assert len(ls) == 2 * n + 1 and np.all(np.diff(ls[: n + 1]) != 0.0) and np.all(np.diff(le[: n + 1]) != 0.0)
    x0, v0 = _start(Engine, s, v)
    g = Engine(s, data); g.set_positions(x0); g.set_velocities(v0)

    def parts(x):      # U_exact(x; l) = A0(x; ls_l) + le_l E1(x) + le_l^2 E2(x)
        e1, e2 = ref.charge_coefficients(x)
        return lambda l: ref.sterics_part(x, ls[l]) + le[l] * e1 + le[l] * le[l] * e2
    w_prev, u_prev, got, want, cumulative = 0.0, parts(g.get_positions()), [], [], []
    for k in range(n):
        g.step(1)
        w = g.get_global("protocol_work"); got.append(w - w_prev); w_prev = w; cumulative.append(w)
        u_next = parts(g.get_positions())
        want.append((u_prev(2 * k + 1) - u_prev(2 * k)) + (u_next(2 * k + 2) - u_next(2 * k + 1)))
        u_prev = u_next
    got, want = np.array(got), np.array(want)
    scale = max(1.0, np.abs(np.cumsum(want)).max())
    print("work increments, max |engine - reference|:", np.abs(got - want).max(), "scale", scale)
    assert np.abs(got - want).max() <= (1e-9 if precision else 1e-5) * scale
    # the same switch in one call on a fresh engine: the same trace, bit for bit
    g2 = Engine(s, data); g2.set_positions(x0); g2.set_velocities(v0)
    trace = g2.run_switch(n, trace=True)
    print("trace, one call - step by step:", np.abs(trace - np.array(cumulative)).max())
    assert np.array_equal(trace, np.array(cumulative))
    # the treatment is in fact active
    d = Engine(systems.with_alchemical_pme_treatment(s, "direct-space"), data); d.set_positions(x0); d.set_velocities(v0)
    wd = d.run_switch(n, trace=True)
    assert abs(wd[-1] - trace[-1]) > 1e-4
    for e in (g, g2, d):
        e.close()


# ---- 5. the correction vanishes
def test_full_coupling_is_the_md_system_up_to_the_box_constant(Engine, cases):
    s = cases["toluene"][0]
    md = copy.copy(s); md.alchemical_atoms = np.zeros(0, np.int32); md.alchemical_pme_treatment = "direct-space"
    data = _integ().to_data(precision=1)
    ge, gm = Engine(s, data), Engine(md, data)
    lig = np.asarray(s.alchemical_atoms)
    const = systems.dispersion_correction_energy(s, zero_epsilon=lig) - systems.dispersion_correction_energy(s)
    x = np.array(s.positions, dtype=np.float64)
    d = []
    for rnd in range(2):
        ge.set_positions(x); gm.set_positions(x)
        d.append(ge.potential_energy() - gm.potential_energy())
        x = x + np.random.RandomState(5).normal(scale=0.003, size=x.shape)
    print("U_exact(1, 1) - U_md at two configurations:", d, "constant:", const)
    assert abs(d[0] - d[1]) <= 1e-9 and abs(d[0] - const) <= 1e-9
    ge.close(); gm.close()


def test_blues_iterations_differential_and_four_energy_forms_agree(Engine, tol_box, cases, tune):
    from blues_amd import moves, simulation, unit
    from blues_amd.context import Simulation
    s = cases["toluene"][0]
    v = tol_box[1]
    md_sys = copy.copy(s); md_sys.alchemical_atoms = np.zeros(0, np.int32); md_sys.alchemical_pme_treatment = "direct-space"
    plan = systems.alchemical_difference_plan(s, md_sys)
    assert plan is not None and plan["kind"] == "zero" and plan["treatment"] == "exact"
    lig = np.arange(15)
    R, nsteps, nmd, nIter = 2, 10, 10, 2
    tune(assume_batch=R)

    def chains(differential):
        out = []
        for r in range(R):
            sim = Simulation(None, s, integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=0.002, temperature=300.0, seed=700 + r), precision="double", replica=r)
            md = Simulation(None, md_sys, integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=800 + r), precision="double", replica=r)
            alch = Simulation(None, md_sys, integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=900 + r), precision="double", replica=r)
            md.context.setPositions(unit.Quantity(s.positions, "nanometer")); md.context.setVelocities(unit.Quantity(v * (1.0 + 0.03 * r), "nanometer/picosecond"))
            mover = moves.MoveEngine(moves.RandomLigandRotationMove(lig, s.mass[lig], random_state=90 + r))
            out.append(simulation.BLUESSimulation(simulation.SimulationSet(sim, md=md, alch=alch), {"nstepsNC": nsteps, "moveStep": nsteps // 2, "nIter": nIter, "nstepsMD": nmd},
                                                  mover, rng=np.random.RandomState(4000 + r), differential_correction=differential))
        return out

    results = {}
    for differential in (False, None):
        for batched in (True, False):
            cs = chains(differential)
            assert all((c._diff_plan is not None) == (differential is None) for c in cs)
            B = simulation.BatchedBLUESSimulation(cs, batched_boundary=batched)
            records = []
            B.run(nIter=nIter, on_iteration=lambda N, last: records.append([dict(l) for l in last]))
            e_scale = max(abs(c.stateTable["md"]["state0"]["potential_energy"]._value) for c in cs)
            results[(differential, batched)] = (records, [c._md_sim.context._engine.get_positions() for c in cs], e_scale)
            B.close()
    kT = 0.0083144626 * 300.0
    ref = results[(False, True)]
    for key in ((None, True), (None, False), (False, False)):
        rec, xs, _ = results[key]
        for N in range(nIter):
            for r in range(R):
                a, b = rec[N][r], ref[0][N][r]
                assert abs(a["correction"] - b["correction"]) <= 1e-9 * max(ref[2], abs(b["protocol_work"])) / kT, (key, N, r, a["correction"], b["correction"])
                assert a["accept"] == b["accept"] and a["protocol_work"] == pytest.approx(b["protocol_work"], rel=1e-9, abs=1e-9)
        for r in range(R):
            assert np.abs(xs[r] - ref[1][r]).max() < 1e-9
    # the differential form is identically zero: the two Systems differ by a constant of the switch's fixed box
    assert all(results[(None, True)][0][N][r]["correction"] == 0.0 for N in range(nIter) for r in range(R))


# ---- 6. batch = solo, bitwise
def test_batch_is_bitwise_solo_and_does_not_mix_treatments(Engine, tune):
    from blues_amd.engine import EngineError, NativeBatch
    s, v = systems.s23k(mobile_atoms=275, frozen=True)
    r = systems.with_reciprocal_space(s)
    x = _exact(r)
    R, n = 4, 12
    tune(assume_batch=8)

    def make(systems_):
        out = []
        for q in range(R):
            e = Engine(systems_[q], _integ(n, seed=40 + q).to_data(precision=0, replica=q)); e.set_velocities(v * (1 + 0.02 * q)); out.append(e)
        return out
    solo = make([x] * R); ws = [e.run_switch(n, trace=True) for e in solo]
    bat = make([x] * R); B = NativeBatch(bat); _, wb = B.step(n, trace=True)
    assert B.stats()["fallback_steps"] == 0
    for q in range(R):
        assert np.array_equal(wb[q], ws[q]) and np.array_equal(solo[q].get_positions(), bat[q].get_positions())
    evals = [e.stats()["own_energy_evaluations"] for e in bat]
    B.prefetch_energies(kinetic=False)      # no member has an energy cached: one shared evaluation, the new partials through the batch's gather
    for q in range(R):
        assert bat[q].potential_energy() == solo[q].potential_energy()
        assert bat[q].stats()["own_energy_evaluations"] == evals[q]      # (served from what the prefetch left, not by a launch of the member's own)
        _assert_path(bat[q], True)
    B.close()
    direct = make([r] * R); wd = direct[0].run_switch(n, trace=True)
    assert abs(wd[-1] - ws[0][-1]) > 1e-6
    mixed = make([x, r, x, r]); M = NativeBatch(mixed)
    with pytest.raises(EngineError, match="congruent"):
        M.step(2)
    M.close()


# ---- the device minimiser on an exact engine (its force passes run the same mesh launches)
@pytest.mark.parametrize("precision", [1, 0])
def test_minimiser_descends_the_exact_potential(Engine, cases, precision):
    s, ref, _ = cases["toluene"]
    g = Engine(s, _integ().to_data(precision=precision))
    g.set_global("lambda_sterics", 0.5); g.set_global("lambda_electrostatics", 0.3)
    out = g.minimize(tolerance=10.0, max_iterations=30)
    x = g.get_positions()
    eo, fo, _t = ref.evaluate(x, 0.5, 0.3)
    print("minimiser:", out, "reference energy at the end:", eo)
    assert out["e_final"] < out["e_initial"]
    assert abs(out["e_final"] - eo) <= TOL[precision] * abs(eo) and abs(g.potential_energy() - eo) <= TOL[precision] * abs(eo)
    assert _rel(g.get_forces(), fo) <= TOL[precision]
    g.close()


# ---- 7. what the library refuses
def _create_ext(s, data, treatment, struct_size=None):
    from blues_amd import _lib
    lib = _lib.load()
    sd, keep_s = s.to_desc(); idesc, keep_i = data.to_desc()
    ext = _abi.BluesSystemExt(); ext.struct_size = C.sizeof(_abi.BluesSystemExt) if struct_size is None else struct_size; ext.alchemical_pme_treatment = treatment
    h = C.c_void_p()
    rc = lib.blues_engine_create_ext(C.byref(sd), C.byref(idesc), None, C.byref(ext), 0, C.byref(h))
    msg = lib.blues_last_error(None).decode()
    if rc == 0:
        lib.blues_engine_destroy(h)
    return rc, msg


def test_library_side_refusals(Engine, tol_box):
    plain = tol_box[0]
    box = systems.with_reciprocal_space(plain)
    data = _integ().to_data(precision=1)
    assert _create_ext(box, data, 1)[0] == 0 and _create_ext(box, data, 0)[0] == 0
    rc, msg = _create_ext(plain, data, 1)
    assert rc and "needs nonbonded_method = PME with a mesh" in msg
    nc = copy.copy(plain); nc.nonbonded_method = _abi.NB_NOCUTOFF
    rc, msg = _create_ext(nc, data, 1)
    assert rc and "needs nonbonded_method = PME with a mesh" in msg
    dec = copy.copy(box); dec.annihilate_electrostatics = False
    rc, msg = _create_ext(dec, data, 1)
    assert rc and "annihilate_electrostatics = 1" in msg
    for flag in ("measure_shadow_work", "measure_heat"):
        d = _integ().to_data(precision=1); setattr(d, flag, 1)
        rc, msg = _create_ext(box, d, 1)
        assert rc and "measure_shadow_work / measure_heat is not supported" in msg
    d = _integ().to_data(precision=1); d.switching_mode = _abi.SWITCH_VV
    d.lambda_sterics = d.lambda_sterics[: d.nsteps_neq + 1]; d.lambda_electrostatics = d.lambda_electrostatics[: d.nsteps_neq + 1]
    rc, msg = _create_ext(box, d, 1)
    assert rc and "switching_mode integrator is not supported" in msg
    nogrid = copy.copy(box); nogrid.pme_grid = (0, 0, 0)      # PME named, no mesh: the library refuses what the Python side refuses
    rc, msg = _create_ext(nogrid, data, 1)
    assert rc and "needs nonbonded_method = PME with a mesh" in msg
    rc, msg = _create_ext(box, data, 2)
    assert rc and "the engine knows 0 ('direct-space') and 1 ('exact')" in msg
    rc, msg = _create_ext(box, data, 1, struct_size=4)
    assert rc and "struct_size" in msg
    # the mesh differential has nothing to offer such an engine
    from blues_amd.engine import EngineError
    g = Engine(_exact(box), data)
    with pytest.raises(EngineError, match="no mesh differential"):
        g.mesh_energy(True)
    g.close()
