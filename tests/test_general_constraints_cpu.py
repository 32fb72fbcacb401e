"""CPU suite: what system_from_amber(constraints=...) emits for HBonds / AllBonds / HAngles on the TOL-parm fixture (15-atom toluene in
320 waters), against arrays formed here from the prmtop, and the oracle stepping the HAngles System."""
import os

import numpy as np

from blues_amd import amber, integrators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIG = list(range(15))


def _load():
    prm = amber.read_prmtop(os.path.join(GOLDEN, "TOL-parm.prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "TOL-parm.inpcrd"))
    return prm, pos, box


def _system(constraints):
    prm, pos, box = _load()
    return prm, amber.system_from_amber(prm, pos, box, constraints=constraints, alchemical_atoms=LIG)


def _prmtop_tables(prm):
    """(bonds [(i, j, r0 nm)], angles [(i, j, k, theta0)], atomic numbers, water mask) straight from the prmtop sections"""
    def rows(name, w):
        a = prm.get(name)
        return np.zeros((0, w), int) if a is None or len(a) == 0 else np.asarray(a).reshape(-1, w)
    b = np.vstack([rows("BONDS_INC_HYDROGEN", 3), rows("BONDS_WITHOUT_HYDROGEN", 3)])
    a = np.vstack([rows("ANGLES_INC_HYDROGEN", 4), rows("ANGLES_WITHOUT_HYDROGEN", 4)])
    bonds = [(int(r[0]) // 3, int(r[1]) // 3, prm["BOND_EQUIL_VALUE"][int(r[2]) - 1] * 0.1) for r in b]
    angles = [(int(r[0]) // 3, int(r[1]) // 3, int(r[2]) // 3, prm["ANGLE_EQUIL_VALUE"][int(r[3]) - 1]) for r in a]
    atnum = np.asarray(prm["ATOMIC_NUMBER"])
    ptr = list(np.asarray(prm["RESIDUE_POINTER"]) - 1) + [len(atnum)]
    water = np.zeros(len(atnum), bool)
    for r, lab in enumerate(prm["RESIDUE_LABEL"]):
        if lab in amber.WATER_NAMES:
            water[ptr[r]:ptr[r + 1]] = True
    return bonds, angles, atnum, water


def _expected(prm, mode):
    """constraint list (pairs, distances) and the angles kept, in the loader's order: bonds in prmtop order, then the water H-H"""
    bonds, angles, atnum, water = _prmtop_tables(prm)
    pairs, dist = [], []
    for i, j, r0 in bonds:
        if mode == "AllBonds" or atnum[i] == 1 or atnum[j] == 1 or (water[i] and water[j]):
            pairs.append((i, j)); dist.append(r0)
    have = {frozenset(p) for p in pairs}
    d_of = {frozenset(p): d for p, d in zip(pairs, dist)}
    kept = []
    for i, j, k, th0 in angles:
        if water[i] and water[j] and water[k]:
            if frozenset((i, k)) not in have:
                d1, d2 = d_of[frozenset((i, j))], d_of[frozenset((k, j))]
                pairs.append((i, k)); dist.append(float(np.sqrt(d1 * d1 + d2 * d2 - 2 * d1 * d2 * np.cos(th0)))); have.add(frozenset((i, k)))
            continue
        kept.append((i, j, k))
    return np.array(pairs, np.int32), np.array(dist), np.array(kept, np.int32).reshape(-1, 3)


def test_hbonds_and_allbonds_are_unchanged():
    for mode in ("HBonds", "AllBonds"):
        prm, s = _system(mode)
        pairs, dist, kept = _expected(prm, mode)
        assert np.array_equal(s.constraint_atoms, pairs), mode
        assert np.array_equal(s.constraint_dist, dist), mode
        assert np.array_equal(s.angle_atoms, kept), mode
    # (AllBonds leaves no harmonic bond; HBonds keeps the 7 C-C bonds of the toluene)
    assert len(_system("AllBonds")[1].bond_atoms) == 0 and len(_system("HBonds")[1].bond_atoms) == 7


def test_hangles_adds_the_methyl_h_h_constraints():
    prm, s = _system("HAngles")
    _, ab = _system("AllBonds")
    bonds, angles, atnum, water = _prmtop_tables(prm)
    # the AllBonds set, unchanged (the new constraints stand where their angles stand in the prmtop: among the waters' H-H) ...
    as_dict = lambda q: {frozenset((int(i), int(j))): float(d) for (i, j), d in zip(q.constraint_atoms, q.constraint_dist)}
    got, base = as_dict(s), as_dict(ab)
    assert len(got) == len(s.constraint_atoms) == len(base) + 3
    assert all(got[p] == d for p, d in base.items())
    assert [tuple(p) for p in s.constraint_atoms if frozenset(map(int, p)) in base] == [tuple(p) for p in ab.constraint_atoms]
    extra = {p: d for p, d in got.items() if p not in base}
    # ... plus exactly the H-C-H angles of the toluene's methyl group (its aromatic carbons carry one hydrogen each; no oxygen in it)
    hxh = [(i, j, k, th) for i, j, k, th in angles if not water[j] and atnum[i] == 1 and atnum[k] == 1]
    assert len(hxh) == 3 and len({j for _, j, _, _ in hxh}) == 1
    assert set(extra) == {frozenset((i, k)) for i, _, k, _ in hxh}
    d_of = {frozenset((i, j)): r0 for i, j, r0 in bonds}
    for i, j, k, th in hxh:
        d1, d2 = d_of[frozenset((i, j))], d_of[frozenset((k, j))]
        assert abs(extra[frozenset((i, k))] - np.sqrt(d1 * d1 + d2 * d2 - 2 * d1 * d2 * np.cos(th))) < 1e-15
    # the three angles have left the harmonic list, nothing else has
    gone = {(i, j, k) for i, j, k, _ in hxh}
    assert [tuple(a) for a in s.angle_atoms] == [tuple(a) for a in ab.angle_atoms if tuple(a) not in gone]
    assert len(s.angle_atoms) == len(ab.angle_atoms) - 3
    # rigid water as it was: each water's H-H constraint once
    ca = [frozenset((int(i), int(j))) for i, j in s.constraint_atoms]
    hh_water = [p for p in ca if all(water[a] and atnum[a] == 1 for a in p)]
    assert len(hh_water) == len(set(hh_water)) == int(water.sum()) // 3


def test_hangles_sees_repartitioned_hydrogens():
    prm, pos, box = _load()
    a = amber.system_from_amber(prm, pos, box, constraints="HAngles", alchemical_atoms=LIG)
    b = amber.system_from_amber(prm, pos, box, constraints="HAngles", alchemical_atoms=LIG, hydrogen_mass=3.024)
    assert np.array_equal(a.constraint_atoms, b.constraint_atoms) and np.array_equal(a.angle_atoms, b.angle_atoms)
    atnum = np.asarray(prm["ATOMIC_NUMBER"])
    assert b.mass[atnum == 1].min() > 3.0
    # the methyl H-H constraints are there although no hydrogen of the repartitioned System is light
    lig_hh = [(int(i), int(j)) for i, j in b.constraint_atoms if i in LIG and j in LIG and atnum[i] == 1 and atnum[j] == 1]
    assert len(lig_hh) == 3


def test_oracle_steps_the_hangles_system(oracle_mod):
    _, s = _system("HAngles")
    tol = 1e-8
    it = integrators.AlchemicalExternalLangevinIntegrator({"lambda_sterics": "1 - 0.3*sin(3.141592653589793*lambda)"}, splitting="H V R O R V H",
                                                          temperature=300.0, timestep=0.002, constraint_tolerance=tol, nsteps_neq=5, seed=1)
    o = oracle_mod.Oracle(s, it.to_data(precision=1))
    o.set_velocities_to_temperature(300.0, 3)
    o.step(5)
    x = o.get_positions()
    ca, cd = np.asarray(s.constraint_atoms), np.asarray(s.constraint_dist)
    r = x[ca[:, 0]] - x[ca[:, 1]]
    r -= s.box * np.round(r / s.box)
    # the solvers' acceptance: |r^2 - d^2| <= 2 tol d^2 (the small clusters end far below it)
    assert (np.abs((r * r).sum(1) - cd * cd) / (cd * cd)).max() <= 2 * tol
    assert np.all(np.isfinite(x)) and np.isfinite(o.get_global("protocol_work"))
