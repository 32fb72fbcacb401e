"""CPU suite: the numpy reference of the device-resident minimiser (tests/fire_reference.py) on the CPU oracle's
forces, and the Python wrappers' behaviour against a library that was built before the minimiser."""
import ctypes

import numpy as np
import pytest

import fire_reference as fr
from blues_amd import _abi, engine, integrators

FUNCS = {"lambda_sterics": "1 - 0.3*sin(3.141592653589793*lambda)", "lambda_electrostatics": "1 - 0.5*sin(3.141592653589793*lambda)"}
LJ13_LITERATURE = -44.3268   # epsilon (Hoare & Pal 1971; the Cambridge Cluster Database's LJ13 global minimum -44.326801)


def _data():
    return integrators.AlchemicalExternalLangevinIntegrator(FUNCS, temperature=300.0, timestep=0.002, constraint_tolerance=1e-10,
                                                            nsteps_neq=20, seed=1).to_data(precision=1)


@pytest.fixture(scope="module")
def lj13_run(oracle_mod):
    s = fr.lj13()
    o = oracle_mod.Oracle(s, _data())
    forces, energy = fr.oracle_forces(o)
    cons = fr.Constraints(s.constraint_atoms, s.constraint_dist, 1.0 / np.asarray(s.mass))
    x, res, rec = fr.minimize(s.positions, cons, forces, 1e-6)
    return s, x, res, rec, energy(x), energy(np.asarray(s.positions))


def test_lj13_converges(lj13_run):
    s, x, res, rec, e, e_start = lj13_run
    assert res["converged"] == 1 and res["fmax"] <= 1e-6 and res["iterations"] == len(rec) - 1
    assert e < e_start
    assert all(r["dt"] <= fr.DEFAULTS["dt_max"] for r in rec)
    assert any(r["P"] <= 0.0 for r in rec[1:]) and any(r["n_pos"] > fr.DEFAULTS["n_min"] for r in rec)   # both branches of the adaptation ran


def test_lj13_energy_is_the_literature_minimum(lj13_run):
    s, x, res, rec, e, _ = lj13_run
    eps = float(s.epsilon[0])
    print("LJ13: %.9f epsilon after %d iterations (literature %.4f)" % (e / eps, res["iterations"], LJ13_LITERATURE))
    assert abs(e / eps - LJ13_LITERATURE) <= 1e-4 * abs(LJ13_LITERATURE)


def test_projected_force_of_a_rigid_water_is_orthogonal_to_its_constraints():
    x = np.array([[0.0, 0.0, 0.0], [0.09572, 0.0, 0.0], [-0.023999, 0.092663, 0.0]]) + 0.3
    atoms = np.array([(0, 1), (0, 2), (1, 2)])
    dist = np.array([np.linalg.norm(x[i] - x[j]) for i, j in atoms])
    w = 1.0 / np.array([15.9994, 1.008, 1.008])
    cons = fr.Constraints(atoms, dist, w)
    assert len(cons.clusters) == 1
    F = np.random.RandomState(3).normal(0.0, 500.0, (3, 3))
    G = cons.project_force(x, F.copy())
    for (i, j), d in zip(atoms, dist):
        r = (x[i] - x[j]) / d
        # the acceleration difference along the bond: what the constraint forbids
        assert abs(((w[i] * G[i] - w[j] * G[j]) * r).sum()) <= 1e-12 * np.abs(w[:, None] * F).max()
    # the projection removes constraint forces only: total force and torque are what they were
    assert np.abs(G.sum(0) - F.sum(0)).max() <= 1e-10 and np.abs(np.cross(x, G).sum(0) - np.cross(x, F).sum(0)).max() <= 1e-10
    # shake then holds the distances, rattle the velocities
    y = cons.shake(x + 0.003 * np.random.RandomState(4).uniform(-1, 1, x.shape), x)
    assert max(abs(np.linalg.norm(y[i] - y[j]) - d) for (i, j), d in zip(atoms, dist)) <= 1e-13


class _OldLibrary(object):
    """A library from before the minimiser: every call but the three new symbols."""
    def blues_last_error(self, h):
        return b""


def test_wrappers_raise_cleanly_without_the_symbols():
    e = object.__new__(engine.NativeEngine)
    e._lib, e._h, e.n = _OldLibrary(), ctypes.c_void_p(1), 3
    with pytest.raises(engine.EngineError, match="blues_minimize"):
        e.minimize(10.0)
    e._h = None
    b = object.__new__(engine.NativeBatch)
    b._lib, b._h, b.engines, b.device_turn = _OldLibrary(), None, [e], None
    with pytest.raises(engine.EngineError, match="blues_batch_minimize"):
        b.minimize_all(10.0)
    with pytest.raises(engine.EngineError, match="unknown setting"):
        engine._minimize_desc(type("L", (), {n: 1 for n in _abi.OPTIONAL_SYMBOLS})(), {"step": 1.0})
    # the optional symbols are skipped by the prototype declaration of such a library, every other one is still demanded

    class Lib(object):
        def __getattr__(self, name):
            if name in _abi.OPTIONAL_SYMBOLS:
                raise AttributeError(name)
            fn = lambda *a: 0
            self.__dict__[name] = fn
            return fn
    assert set(_abi.OPTIONAL_SYMBOLS) <= set(_abi.declare_engine_prototypes(Lib()))
