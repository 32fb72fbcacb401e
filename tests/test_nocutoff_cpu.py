"""NoCutoff (vacuum) Systems on the host side: system_from_amber's nonbonded_method, the CPU oracle's all-pairs path pinned
against an independent numpy loop (the GPU is checked against the oracle), and what the engine refuses before it is loaded."""
import dataclasses
import os

import numpy as np
import pytest

from blues_amd import _abi, amber, integrators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ONE_4PI_EPS0 = 138.935456

# (fixture, alchemical atoms): the reference's RandomLigandRotationMove ligand of TOL-parm, and the side chain of residue 1 of
# vacDivaline that its SideChainMove(struct, [1]) selects
SYSTEMS = {"TOL-parm": list(range(15)), "vacDivaline": list(range(22, 32))}


def nocutoff_system(name, **kw):
    prm = amber.read_prmtop(os.path.join(GOLDEN, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, name + ".inpcrd"))
    return amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=SYSTEMS[name], nonbonded_method="NoCutoff", **kw)


def numpy_nonbonded(s, x, ls, le):
    """Terms 3-6 and the forces of NonbondedForce (NoCutoff) + the alchemical softcore forms, all pairs, fp64, from the
    SystemData arrays alone."""
    n = s.n_atoms
    alch = np.zeros(n, bool); alch[s.alchemical_atoms] = True
    iu, ju = np.triu_indices(n, 1)
    excl = set(map(tuple, np.sort(s.exclusions, axis=1).tolist()))
    keep = np.array([(a, b) not in excl for a, b in zip(iu.tolist(), ju.tolist())])
    i, j = iu[keep], ju[keep]
    T = np.zeros(10); F = np.zeros((n, 3))

    def pairs(i, j, qq, sig, eps, term_plain):
        d = x[i] - x[j]
        r2 = (d * d).sum(1); r = np.sqrt(r2)
        ai, aj = alch[i], alch[j]
        plain = ~ai & ~aj
        both = ai & aj
        ls_eff = np.where(both & (not s.annihilate_sterics), 1.0, ls)
        le_eff = np.where(both & (not s.annihilate_electrostatics), 1.0, le)
        # plain 12-6 LJ and bare Coulomb
        sr6 = (sig * sig / r2) ** 3
        u_lj = 4 * eps * (sr6 * sr6 - sr6)
        f_lj = 4 * eps * (12 * sr6 * sr6 - 6 * sr6) / r2
        u_c = ONE_4PI_EPS0 * qq / r
        f_c = ONE_4PI_EPS0 * qq / (r * r2)
        # softcore LJ
        with np.errstate(divide="ignore", invalid="ignore"):
            q2 = r2 / (sig * sig); q6 = q2 ** 3
            xs = 1.0 / (s.softcore_alpha * (1.0 - ls_eff) + q6)
            u_sc = np.where((eps == 0) | (sig == 0), 0.0, ls_eff * 4 * eps * xs * (xs - 1))
            f_sc = np.where((eps == 0) | (sig == 0), 0.0, ls_eff * 4 * eps * (2 * xs - 1) * xs * xs * 6 * q2 * q2 / (sig * sig))
        T[term_plain] += (u_lj + u_c)[plain].sum()
        T[5] += u_sc[~plain].sum(); T[6] += (le_eff * u_c)[~plain].sum()
        fs = np.where(plain, f_lj + f_c, f_sc + le_eff * f_c)
        np.add.at(F, i, fs[:, None] * d); np.add.at(F, j, -fs[:, None] * d)

    pairs(i, j, s.charge[i] * s.charge[j], 0.5 * (s.sigma[i] + s.sigma[j]), np.sqrt(s.epsilon[i] * s.epsilon[j]), 3)
    ea, ep = s.exception_atoms, s.exception_params
    if len(ea):
        pairs(ea[:, 0], ea[:, 1], ep[:, 0], ep[:, 1], ep[:, 2], 4)
    return T, F


def test_system_from_amber_nocutoff_fields():
    for name in SYSTEMS:
        s = nocutoff_system(name)
        assert s.nonbonded_method == _abi.NB_NOCUTOFF
        assert tuple(s.pme_grid) == (0, 0, 0)
        assert s.dispersion_correction is False
        assert s.ewald_alpha == 0.0
    # box=None is a vacuum System's own box
    prm = amber.read_prmtop(os.path.join(GOLDEN, "vacDivaline.prmtop"))
    pos, _, _ = amber.read_inpcrd(os.path.join(GOLDEN, "vacDivaline.inpcrd"))
    s = amber.system_from_amber(prm, pos, None, nonbonded_method="NoCutoff")
    assert s.n_atoms == 35 and np.all(s.box == 0.0)
    with pytest.raises(ValueError):
        amber.system_from_amber(prm, pos, None)
    with pytest.raises(ValueError):
        amber.system_from_amber(prm, pos, None, nonbonded_method="CutoffPeriodic")


def test_system_from_amber_default_unchanged():
    prm = amber.read_prmtop(os.path.join(GOLDEN, "TOL-parm.prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "TOL-parm.inpcrd"))
    a = amber.system_from_amber(prm, pos, box)
    b = amber.system_from_amber(prm, pos, box, nonbonded_method="PME")
    assert a.nonbonded_method == _abi.NB_PME and a.dispersion_correction is True and all(k > 0 for k in a.pme_grid)
    for f in dataclasses.fields(a):
        va, vb = getattr(a, f.name), getattr(b, f.name)
        if isinstance(va, np.ndarray):
            assert np.array_equal(va, vb), f.name
        else:
            assert va == vb, f.name
    c = amber.system_from_amber(prm, pos, box, reciprocal_space=False)
    assert c.nonbonded_method == _abi.NB_PME_DIRECT and tuple(c.pme_grid) == (0, 0, 0)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_oracle_nocutoff_matches_numpy_all_pairs(name):
    from oracle import oracle
    s = nocutoff_system(name)
    # the nonbonded part alone: no bonded terms (their forces would hide the pair forces' agreement)
    s = dataclasses.replace(s, bond_atoms=np.zeros((0, 2), np.int32), bond_params=np.zeros((0, 2)),
                            angle_atoms=np.zeros((0, 3), np.int32), angle_params=np.zeros((0, 2)),
                            torsion_atoms=np.zeros((0, 4), np.int32), torsion_params=np.zeros((0, 3)))
    data = integrators.generateNCMCIntegrator(nstepsNC=10, dt=0.002, temperature=300.0, seed=1).to_data(precision=1)
    o = oracle.Oracle(s, data)
    x = np.asarray(s.positions)
    for ls, le in ((1.0, 1.0), (0.5, 0.3), (0.0, 0.0)):
        e, f, t = o.energy_forces(ls, le)
        T, F = numpy_nonbonded(s, x, ls, le)
        for k in (3, 4, 5, 6):
            assert abs(t[k] - T[k]) <= 1e-12 * max(1.0, abs(T[k])), (name, ls, le, k, t[k], T[k])
        assert t[8] == 0.0 and t[9] == 0.0
        assert np.abs(f - F).max() <= 1e-12 * np.abs(F).max(), (name, ls, le, np.abs(f - F).max())


def test_native_engine_refuses_custom_forces_before_loading(monkeypatch):
    from blues_amd import engine as engine_mod
    # what the ethylene known-answer System carries (tests/test_ethylene_known_answer.py): a custom pair force and a centroid bond
    s = dataclasses.replace(nocutoff_system("vacDivaline"), extras={"custom_pair_mode": 1, "centroid_bonds": [(0, 1, 2, 3, 100.0)]})
    called = []
    monkeypatch.setattr(engine_mod, "load", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("library loaded")))
    data = integrators.generateNCMCIntegrator(nstepsNC=10, dt=0.002, temperature=300.0, seed=1).to_data()
    with pytest.raises(engine_mod.EngineError, match="custom forces"):
        engine_mod.NativeEngine(s, data)
    assert not called


def test_barostat_on_nocutoff_system_raises():
    from blues_amd import context
    s = dataclasses.replace(nocutoff_system("vacDivaline"), barostat=(1.0, 300.0, 25))
    integ = integrators.LangevinIntegrator(300.0, 1.0, 0.002)
    with pytest.raises(ValueError, match="non-periodic"):
        context.Simulation(None, s, integ)
