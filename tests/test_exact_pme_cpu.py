"""CPU suite: the 'exact' alchemical PME treatment's Python surface (field, round trips, refusals before a library is loaded, the
difference plan) and the self-checks of the fp64 reference the GPU tests compare against (tests/exact_pme_reference.py)."""
import copy
import os

import numpy as np
import pytest

import exact_pme_reference as xref
from blues_amd import _abi, amber, integrators, systems

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def box(tol_box):
    return systems.with_reciprocal_space(tol_box[0])


@pytest.fixture(scope="module")
def ref(box):
    return xref.ExactPmeReference(box)


def _data(**fields):
    d = integrators.generateNCMCIntegrator(nstepsNC=10, dt=0.002, temperature=300.0, seed=1).to_data(precision=1)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


# ---- the reference's self-checks
def test_reference_is_exactly_quadratic_in_lambda_electrostatics(box, ref):
    x = box.positions
    e0, e1, e2 = ref.coefficients(x, 0.5)
    le = 0.3
    u = ref.energy(x, 0.5, le)
    assert abs(u - (e0 + le * e1 + le * le * e2)) <= 1e-10 * max(1.0, abs(u))
    assert abs(e1) > 1.0 and abs(e2) > 1.0      # (both classes are there)


def test_reference_force_is_the_central_difference_of_its_energy(box, ref):
    x = np.array(box.positions, dtype=np.float64)
    h = 1e-5
    _, f, _ = ref.evaluate(x, 0.5, 0.3)
    for atom, axis in ((0, 0), (7, 2), (20, 1)):
        xp, xm = x.copy(), x.copy()
        xp[atom, axis] += h; xm[atom, axis] -= h
        num = -(ref.energy(xp, 0.5, 0.3) - ref.energy(xm, 0.5, 0.3)) / (2.0 * h)
        assert abs(f[atom, axis] - num) <= 1e-6 * max(1.0, abs(num)), (atom, axis, f[atom, axis], num)


def test_reference_direct_part_at_full_coupling_is_the_direct_space_oracles(box, ref, oracle_mod):
    """At le = 1 the composition's [3] + [4] + [6] equals the same sum of the oracle under the 'direct-space' treatment: the treatments
    differ in reciprocal space ([8]) only, and there by several kJ/mol."""
    o = oracle_mod.Oracle(box, _data())
    _, _, to = o.energy_forces(0.5, 1.0)
    _, _, tr = ref.evaluate(box.positions, 0.5, 1.0)
    assert abs((tr[3] + tr[4] + tr[6]) - (to[3] + to[4] + to[6])) <= 1e-9 * abs(to[3])
    for k in (0, 1, 2, 5, 7, 9):
        assert abs(tr[k] - to[k]) <= 1e-10 * max(1.0, abs(to[k]))
    assert abs(tr[8] - to[8]) > 1.0


def test_exact_system_at_full_coupling_is_the_plain_one_up_to_a_box_constant(box, ref, oracle_mod):
    plain = copy.copy(box); plain.alchemical_atoms = np.zeros((0,), np.int32)
    o = oracle_mod.Oracle(plain, _data())
    rng = np.random.RandomState(3)
    d = []
    for k in range(2):
        x = box.positions + (0.002 * rng.standard_normal(box.positions.shape) if k else 0.0)
        o.set_positions(x)
        d.append(ref.energy(x, 1.0, 1.0) - o.energy_forces(1.0, 1.0)[0])
    assert abs(d[0] - d[1]) <= 1e-9
    lig = np.asarray(box.alchemical_atoms)
    const = systems.dispersion_correction_energy(box, zero_epsilon=lig) - systems.dispersion_correction_energy(box)
    assert abs(d[0] - const) <= 1e-9


# ---- the field
def test_field_default_and_values(box):
    assert box.alchemical_pme_treatment == "direct-space"
    e = systems.with_alchemical_pme_treatment(box, "exact")
    assert e.alchemical_pme_treatment == "exact" and box.alchemical_pme_treatment == "direct-space"
    assert e.ext_desc().alchemical_pme_treatment == 1 and box.ext_desc() is None
    for bad in ("coulomb", "Exact", "", None, 1):
        with pytest.raises(ValueError, match="'direct-space' and 'exact'"):
            systems.with_alchemical_pme_treatment(box, bad)
    with pytest.raises(ValueError, match="'direct-space' and 'exact'"):
        _abi.SystemData(box=box.box, mass=box.mass, charge=box.charge, sigma=box.sigma, epsilon=box.epsilon, alchemical_pme_treatment="coulomb")


def test_field_survives_the_helpers_and_the_file_round_trip(box, tmp_path):
    e = systems.with_alchemical_pme_treatment(box, "exact")
    assert systems.freeze_atoms(e, [20, 21, 22]).alchemical_pme_treatment == "exact"
    assert systems.freeze_except(e, np.arange(15)).alchemical_pme_treatment == "exact"
    assert systems.restrain_positions(e, [0], 10.0).alchemical_pme_treatment == "exact"
    assert systems.with_reciprocal_space(e).alchemical_pme_treatment == "exact"
    assert systems.tile_system(e, (1, 1, 2)).alchemical_pme_treatment == "exact"
    assert copy.copy(e).alchemical_pme_treatment == "exact"
    systems.save_system(str(tmp_path / "e.npz"), e)
    systems.save_system(str(tmp_path / "d.npz"), box)
    assert systems.load_system(str(tmp_path / "e.npz"))[0].alchemical_pme_treatment == "exact"
    assert systems.load_system(str(tmp_path / "d.npz"))[0].alchemical_pme_treatment == "direct-space"
    assert "alchemical_pme_treatment" not in np.load(str(tmp_path / "d.npz")).files     # (a default System's file is what it was)
    assert systems.toluene_box()[0].alchemical_pme_treatment == "direct-space"           # (a file written before the field existed)


def test_system_from_amber_takes_the_treatment():
    prm = amber.read_prmtop(os.path.join(GOLDEN, "TOL-parm.prmtop"))
    pos, _, bx = amber.read_inpcrd(os.path.join(GOLDEN, "TOL-parm.inpcrd"))
    kw = dict(constraints="HBonds", alchemical_atoms=list(range(15)))
    assert amber.system_from_amber(prm, pos, bx, **kw).alchemical_pme_treatment == "direct-space"
    assert amber.system_from_amber(prm, pos, bx, alchemical_pme_treatment="exact", **kw).alchemical_pme_treatment == "exact"
    with pytest.raises(ValueError, match="'direct-space' and 'exact'"):
        amber.system_from_amber(prm, pos, bx, alchemical_pme_treatment="coulomb", **kw)
    with pytest.raises(ValueError, match="needs nonbonded_method = PME with a mesh"):
        amber.system_from_amber(prm, pos, bx, alchemical_pme_treatment="exact", reciprocal_space=False, **kw)
    with pytest.raises(ValueError, match="needs nonbonded_method = PME with a mesh"):
        amber.system_from_amber(prm, pos, None, alchemical_pme_treatment="exact", nonbonded_method="NoCutoff", **kw)


# ---- refusals, in Python, with the library not loaded
@pytest.fixture()
def no_library(monkeypatch):
    from blues_amd import engine

    def refuse():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(engine, "load", refuse)
    return engine


def _exact(s):
    e = copy.copy(s); e.alchemical_pme_treatment = "exact"
    return e


def test_refusals_before_a_library_is_loaded(box, tol_box, no_library):
    E, Err = no_library.NativeEngine, no_library.EngineError
    with pytest.raises(Err, match="needs nonbonded_method = PME with a mesh"):
        E(_exact(tol_box[0]), _data())                                     # direct-space-only PME
    nc = copy.copy(tol_box[0]); nc.nonbonded_method = _abi.NB_NOCUTOFF
    with pytest.raises(Err, match="needs nonbonded_method = PME with a mesh"):
        E(_exact(nc), _data())                                             # NoCutoff
    dec = _exact(box); dec.annihilate_electrostatics = False
    with pytest.raises(Err, match="annihilate_electrostatics = 1"):
        E(dec, _data())
    for flag in ("measure_shadow_work", "measure_heat"):
        with pytest.raises(Err, match="measure_shadow_work / measure_heat is not supported"):
            E(_exact(box), _data(**{flag: 1}))
    for mode in (_abi.SWITCH_VV, _abi.SWITCH_GHMC):
        d = _data(switching_mode=mode)
        with pytest.raises(Err, match="switching_mode integrator is not supported"):
            E(_exact(box), d)
    bad = copy.copy(box); bad.alchemical_pme_treatment = "coulomb"
    with pytest.raises(Err, match="'direct-space' and 'exact'"):
        E(bad, _data())


def test_a_library_without_the_entry_point_is_named(box, monkeypatch):
    from blues_amd import engine

    class Old:      # a library built before blues_engine_create_ext
        pass
    monkeypatch.setattr(engine, "load", lambda: Old())
    with pytest.raises(engine.EngineError, match="blues_engine_create_ext"):
        engine.NativeEngine(_exact(box), _data())
    assert "blues_engine_create_ext" in _abi.OPTIONAL_SYMBOLS


# ---- the driver's plan
def test_difference_plan_of_an_exact_pair_is_zero_without_mesh_work(box):
    plain = copy.copy(box); plain.alchemical_atoms = np.zeros((0,), np.int32)
    p = systems.alchemical_difference_plan(_exact(box), plain)
    assert p["kind"] == "zero" and p["treatment"] == "exact"
    assert "pairs" not in p and "atoms" not in p                        # no mesh launches, no host erf arithmetic
    lig = np.asarray(box.alchemical_atoms)
    assert p["const"] == pytest.approx(systems.dispersion_correction_energy(box) - systems.dispersion_correction_energy(box, zero_epsilon=lig), rel=1e-12)
    assert systems.alchemical_difference_plan(box, plain)["kind"] == "pme"                     # the default is what it was
    other = copy.copy(plain); other.charge = plain.charge * 1.01
    assert systems.alchemical_difference_plan(_exact(box), other) is None


def test_a_library_without_the_new_entries_still_minimises():
    """The minimiser asks for its own three symbols only: a library built before blues_engine_create_ext keeps everything but 'exact'."""
    from blues_amd import engine
    lib = type("L", (), {n: 1 for n in _abi.MINIMIZE_SYMBOLS})()
    assert not hasattr(lib, "blues_engine_create_ext")
    assert engine._minimize_desc(lib, {}) is None
    assert set(_abi.MINIMIZE_SYMBOLS) < set(_abi.OPTIONAL_SYMBOLS) and "blues_get_exact_pme_path" in _abi.OPTIONAL_SYMBOLS
