"""Custom pair and centroid-bond forces on the host side: the typed SystemData fields and their marshalling (ABI 7), what is refused
before the library is loaded, and the CPU oracle's two custom forces pinned against an independent numpy evaluation written here from
the formulas alone (the GPU is checked against the oracle: tests/test_gpu_custom_forces.py)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import ethylene as eth
from blues_amd import _abi, integrators
from test_nocutoff_cpu import numpy_nonbonded, nocutoff_system

LAMBDAS = ((1.0, 1.0), (0.5, 0.3), (0.0, 0.0))


def _data():
    return integrators.generateNCMCIntegrator(nstepsNC=10, dt=0.002, temperature=300.0, seed=1).to_data(precision=1)


def _arr(ptr, n, dtype):
    return np.array([ptr[i] for i in range(n)], dtype=dtype)


def test_to_desc_carries_mode_and_flat_centroid_arrays():
    s = eth.divaline()
    d, keep = s.to_desc()
    assert d.custom_pair_mode == 1 and d.n_centroid_bonds == 2
    start = _arr(d.centroid_group_start, 5, np.int32)
    assert list(start) == [0, 4, 9, 12, 13]
    assert list(_arr(d.centroid_atoms, 13, np.int32)) == [4, 6, 8, 10, 22, 24, 26, 28, 30, 0, 14, 24, 33]
    assert list(_arr(d.centroid_weights, 13, float)) == [1.0, 2.5, 0.5, 3.0, 12.0, 1.0, 0.25, 4.0, 2.0, 3.0, 1.0, 2.0, 0.7]
    assert list(_arr(d.centroid_k, 2, float)) == [850.0, 120.0]
    e, _ = eth.load()[0].to_desc()
    assert e.custom_pair_mode == 1 and e.n_centroid_bonds == 1
    assert list(_arr(e.centroid_group_start, 3, np.int32)) == [0, 2, 4] and list(_arr(e.centroid_atoms, 4, np.int32)) == [0, 1, 2, 3]
    assert list(_arr(e.centroid_weights, 4, float)) == [1.0, 1.0, 12.01, 12.01] and e.centroid_k[0] == 100000.0


def test_defaults_leave_every_old_field_as_it_was():
    plain = nocutoff_system("vacDivaline")
    assert plain.custom_pair_mode == 0 and tuple(plain.centroid_bonds) == ()
    a, _ = plain.to_desc()
    b, _ = eth.divaline().to_desc()
    assert a.custom_pair_mode == 0 and a.n_centroid_bonds == 0
    new = {"custom_pair_mode", "n_centroid_bonds", "centroid_group_start", "centroid_atoms", "centroid_weights", "centroid_k"}
    assert new == {n for n, _ in _abi.BluesSystemDesc._fields_[-6:]}          # appended: every old field keeps its offset
    for name, ctype in _abi.BluesSystemDesc._fields_:
        if name in new:
            continue
        va, vb = getattr(a, name), getattr(b, name)
        if hasattr(ctype, "_type_") and not isinstance(va, (int, float)):      # pointer or array
            if hasattr(va, "contents"):
                count = {"mass": a.n_atoms, "charge": a.n_atoms, "sigma": a.n_atoms, "epsilon": a.n_atoms, "exclusions": 2 * a.n_exclusions,
                         "exception_atoms": 2 * a.n_exceptions, "exception_params": 3 * a.n_exceptions, "bond_atoms": 2 * a.n_bonds,
                         "bond_params": 2 * a.n_bonds, "angle_atoms": 3 * a.n_angles, "angle_params": 2 * a.n_angles,
                         "torsion_atoms": 4 * a.n_torsions, "torsion_params": 3 * a.n_torsions, "constraint_atoms": 2 * a.n_constraints,
                         "constraint_dist": a.n_constraints, "alchemical_atoms": a.n_alchemical, "restraint_atoms": a.n_restraints,
                         "restraint_x0": 3 * a.n_restraints}[name]
                assert [va[i] for i in range(count)] == [vb[i] for i in range(count)], name
            else:
                assert list(va) == list(vb), name
        else:
            assert va == vb, name
    assert ctypes.sizeof(_abi.BluesSystemDesc) % 8 == 0


# ---------------------------------------------------------------- the independent evaluation
def numpy_custom(s, x, ls, le):
    """Energy terms and forces of a NoCutoff System with pair mode 1 and centroid bonds, from the SystemData arrays and the formulas:
      pair (one alchemical, one non-alchemical atom, not excluded):  q_i q_j / r^2 -> term 6;  4 eps ((sig/r)^12 - (sig/r)^6) -> term 5,
            sig = 0.5 (sigma_i + sigma_j) ls,  eps = sqrt(eps_i eps_j) le;  no other regular pair interacts;
      exceptions: as without the mode (tests/test_nocutoff_cpu.py: numpy_nonbonded, regular pairs removed);
      centroid bond: 0.5 k |c1 - c2|^2 -> term 7,  c = sum(w x) / sum(w)."""
    n = s.n_atoms
    x = np.asarray(x, dtype=np.float64)
    T = np.zeros(10)
    alch = np.zeros(n, bool); alch[s.alchemical_atoms] = True
    excl = set(map(tuple, np.sort(np.asarray(s.exclusions).reshape(-1, 2), axis=1).tolist()))
    for i in range(n):
        for j in range(i + 1, n):
            if alch[i] == alch[j] or (i, j) in excl:
                continue
            r = np.linalg.norm(x[i] - x[j])
            sig = 0.5 * (s.sigma[i] + s.sigma[j]) * ls
            eps = np.sqrt(s.epsilon[i] * s.epsilon[j]) * le
            T[6] += s.charge[i] * s.charge[j] / r ** 2
            T[5] += 4.0 * eps * ((sig / r) ** 12 - (sig / r) ** 6)
    if len(s.exception_atoms):
        only_exc = dataclasses.replace(s, exclusions=np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32))
        Te, _ = numpy_nonbonded(only_exc, x, ls, le)
        T[4] += Te[4]; T[5] += Te[5]; T[6] += Te[6]
        assert Te[3] == 0.0
    for idx1, w1, idx2, w2, k in s.centroid_bonds:
        w1, w2 = np.asarray(w1, float), np.asarray(w2, float)
        c1 = (w1[:, None] * x[list(idx1)]).sum(0) / w1.sum()
        c2 = (w2[:, None] * x[list(idx2)]).sum(0) / w2.sum()
        T[7] += 0.5 * k * ((c1 - c2) ** 2).sum()
    return T


def numpy_forces(s, x, ls, le, h=1e-5):
    """Central differences of the numpy energy (terms 4-7: what the custom forces and the exceptions contribute)."""
    x = np.asarray(x, dtype=np.float64)
    F = np.zeros_like(x)
    for i in range(s.n_atoms):
        for k in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, k] += h; xm[i, k] -= h
            F[i, k] = -(numpy_custom(s, xp, ls, le)[4:8].sum() - numpy_custom(s, xm, ls, le)[4:8].sum()) / (2 * h)
    return F


def _no_bonded(s):
    return dataclasses.replace(s, bond_atoms=np.zeros((0, 2), np.int32), bond_params=np.zeros((0, 2)),
                               angle_atoms=np.zeros((0, 3), np.int32), angle_params=np.zeros((0, 2)),
                               torsion_atoms=np.zeros((0, 4), np.int32), torsion_params=np.zeros((0, 3)))


@pytest.mark.parametrize("which", ["ethylene", "vacDivaline+1bond"])
def test_oracle_custom_forces_match_numpy(which):
    from oracle import oracle
    oracle.build()
    if which == "ethylene":
        s = eth.load()[0]
    else:
        s = eth.divaline()
        s = dataclasses.replace(s, centroid_bonds=s.centroid_bonds[:1])
    s = _no_bonded(s)
    o = eth.make_oracle(oracle, s, _data())
    x = np.asarray(s.positions)
    for ls, le in LAMBDAS:
        e, f, t = o.energy_forces(ls, le)
        T = numpy_custom(s, x, ls, le)
        for k in range(10):
            assert abs(t[k] - T[k]) <= 1e-12 * max(1.0, abs(T[k])), (which, ls, le, k, t[k], T[k])
        assert t[3] == 0.0 and abs(e - T.sum()) <= 1e-12 * max(1.0, abs(T.sum()))
        if ls == 0.0 and not len(s.exception_atoms):
            assert t[5] == 0.0      # sigma = 0: the 12-6 part is an exact zero
        # second check: the oracle's analytic forces against central differences of the numpy energy (h = 1e-5 nm: truncation error
        # h^2 f''' / 6 ~ 1e-10 f''', round-off 1e-16 E / h ~ 1e-11 E: a relative 1e-6 of the largest force has room for both)
        F = numpy_forces(s, x, ls, le)
        assert np.abs(f - F).max() <= 1e-6 * np.abs(F).max(), (which, ls, le, np.abs(f - F).max(), np.abs(F).max())
    # term [6] does not depend on the lambdas in this form (for a System without alchemical exceptions)
    if which == "ethylene":
        assert o.energy_forces(0.0, 0.0)[2][6] == o.energy_forces(1.0, 1.0)[2][6]


def test_extras_form_round_trip():
    s, _ = eth.load()
    x = eth.extras_form(s)
    assert x.custom_pair_mode == 0 and tuple(x.centroid_bonds) == ()
    assert x.extras["custom_pair_mode"] == 1 and len(x.extras["centroid_bonds"]) == 1
    a, _ = x.to_desc()
    assert a.custom_pair_mode == 0 and a.n_centroid_bonds == 0


# ---------------------------------------------------------------- refused before the library is loaded
def _bad_systems():
    s = eth.divaline()
    b0 = s.centroid_bonds[0]
    periodic = dataclasses.replace(s, nonbonded_method=_abi.NB_PME_DIRECT, box=np.array([4.0, 4.0, 4.0]))
    return [
        ("custom_pair_mode 2", dataclasses.replace(s, custom_pair_mode=2)),
        ("NoCutoff", periodic),
        ("NoCutoff", dataclasses.replace(periodic, custom_pair_mode=0)),
        ("NoCutoff", dataclasses.replace(periodic, centroid_bonds=())),
        ("at most 4", dataclasses.replace(s, centroid_bonds=(b0,) * 5)),
        ("group of 9 atoms", dataclasses.replace(s, centroid_bonds=((list(range(9)), [1.0] * 9, [20], [1.0], 10.0),))),
        ("group of 0 atoms", dataclasses.replace(s, centroid_bonds=(([], [], [20], [1.0], 10.0),))),
        ("out of range", dataclasses.replace(s, centroid_bonds=(([0, 35], [1.0, 1.0], [20], [1.0], 10.0),))),
        ("out of range", dataclasses.replace(s, centroid_bonds=(([0, -1], [1.0, 1.0], [20], [1.0], 10.0),))),
        ("sum to zero", dataclasses.replace(s, centroid_bonds=(([0, 1], [1.0, -1.0], [20], [1.0], 10.0),))),
        ("no alchemical atom", dataclasses.replace(s, alchemical_atoms=np.zeros(0, np.int32))),
    ]


@pytest.mark.parametrize("case", range(11))
def test_invalid_custom_forces_are_refused_before_loading(monkeypatch, case):
    from blues_amd import engine as engine_mod
    match, s = _bad_systems()[case]
    called = []
    monkeypatch.setattr(engine_mod, "load", lambda: called.append(1) or (_ for _ in ()).throw(AssertionError("library loaded")))
    with pytest.raises(engine_mod.EngineError, match=match):
        engine_mod.NativeEngine(s, _data())
    assert not called
    with pytest.raises(ValueError, match=match):
        s.check_custom_forces()
