"""GPU suite of the Lennard-Jones switching function on every periodic pair path of the HIP engine.

Expected values come from tests/lj_switch_reference.py: numpy fp64, independent of engine and oracle, of the DIFFERENCE the switch makes.
A switched engine minus an unswitched engine on the same System and positions must be that difference; what the switch does not touch
(Coulomb, exceptions, bonded terms, the mesh) must be the same bits in both.

Rows and tuning are those of tests/test_gpu_symmetry.py, each asserting the kernel it means to run: `tile` (the tile kernel, lone and
fused), `sub` (k1_mode = 1: the sub-tile kernel in mixed precision), `atom` (assume_batch = 1024: per-atom lists, pruned, dense
alchemical kernel in mixed precision), `frag` (k1_mode = 3, mixed only), `pme` (mesh on, terms [8] and [9] non-zero).

Tolerances are the project's contracts (tests/test_gpu_symmetry.py, tests/test_oracle_golden.py::test_forces_are_energy_gradient):
1e-10 for double-precision energies and forces (1e-9 on the S23k rows), 1e-5 for mixed precision, gradient check rel 2e-5 / abs 2e-3.
Energies are held relative to max(|value of the switched engine|, 1), forces to the largest force component of the mobile atoms.
Each case prints its residuals ("LJSWITCH ..." lines, pytest -s)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import alch_regions as ar
import lj_switch_reference as ref
from blues_amd import _abi, integrators, systems

pytestmark = pytest.mark.gpu

RS = 0.8
LAMBDAS = ((1.0, 1.0), (0.4, 0.2))
SAME_BITS = (0, 1, 2, 4, 6, 7, 8)          # bonded terms, exceptions, alchemical electrostatics, restraint, reciprocal space
S23K_ROWS = ("sub", "atom")


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _report(case, row, what, value, bound):
    print("LJSWITCH %-10s %-8s %-28s %.3e (bound %.1e)" % (case, row, what, value, bound))


_SYSTEMS = {}


def _row_system(row, tol_box):
    """(unswitched System, velocities) of a row; the switched one is systems.with_switch_distance(., RS)."""
    if row not in _SYSTEMS:
        s, v = tol_box
        if row in ("tile", "frag", "pme"):
            big = systems.tile_system(s, (1, 1, 2))
            if row == "pme":
                big = systems.with_reciprocal_space(big)
            _SYSTEMS[row] = (big, np.concatenate([v, v]))
        elif row in S23K_ROWS:
            if "s23k" not in _SYSTEMS:
                _SYSTEMS["s23k"] = systems.s23k(275, frozen=True)
            _SYSTEMS[row] = _SYSTEMS["s23k"]
        else:
            _SYSTEMS[row] = (s, v)
    return _SYSTEMS[row]


def _set_tuning(row, tune, **more):
    if row == "atom":
        tune(assume_batch=1024, **more)
    elif row == "sub":
        tune(assume_batch=1024, k1_mode=1, **more)
    elif row == "frag":
        tune(k1_mode=3, **more)
    elif more:
        tune(**more)


def _check_path(row, precision, g):
    st = g.stats()
    if row == "tile":
        assert st["nonbonded_kernel"] == 0, st
    elif row == "sub":
        if precision == 0:
            assert st["nonbonded_kernel"] == 1, st
    elif row == "atom":
        if precision == 0:
            assert st["nonbonded_kernel"] == 2 and st["pruned_lists"] == 1, st
    elif row == "frag":
        assert st["nonbonded_kernel"] == 3, st
    elif row == "pme":
        t = g.energy_terms()
        assert t[8] != 0.0 and t[9] != 0.0, t


def _data(precision, nsteps=12, seed=7, replica=0):
    return integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=0.004, temperature=300.0, seed=seed).to_data(precision=precision, replica=replica)


def _static(g, lambdas=LAMBDAS):
    out = []
    for ls, le in lambdas:
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        out.append((np.array(g.energy_terms()), g.potential_energy(), g.get_forces()))
    return out


_DELTAS = {}


def _delta(key, s, x, ls):
    """the reference's difference, computed once per (System, lambda_sterics) and shared"""
    if (key, ls) not in _DELTAS:
        _DELTAS[(key, ls)] = ref.delta(s, x, ls)
    return _DELTAS[(key, ls)]


def _differential(case, row, key, s_sw, x, g0, g1, tol):
    """Case 1's check: switched engine g1 minus unswitched engine g0 against the reference, at both lambda points."""
    mob = s_sw.mass > 0
    lig = np.asarray(s_sw.alchemical_atoms, dtype=np.int64)
    fails = []
    for (ls, le), (t0, e0, f0), (t1, e1, f1) in zip(LAMBDAS, _static(g0), _static(g1)):
        d = _delta(key, s_sw, x, ls)
        assert d["pairs"] > 1000 and abs(d["dE_env"]) > 1.0                          # the shell is populated: the differences compare something
        res = {"term[3]": abs((t1[3] - t0[3]) - d["dE_env"]) / max(abs(t1[3]), 1.0),
               "term[5]": abs((t1[5] - t0[5]) - d["dE_alch"]) / max(abs(t1[5]), 1.0),
               "potential_energy": abs((e1 - e0) - (d["dE"] + (t1[9] - t0[9]))) / max(abs(e1), 1.0),
               "forces": np.abs((f1 - f0)[mob] - d["dF"][mob]).max() / np.abs(f1[mob]).max()}
        for what, r in res.items():
            _report(case, row, "%s at (%g, %g)" % (what, ls, le), r, tol)
            if not r <= tol:
                fails.append((what, ls, le, r))
        assert np.abs(d["dF"][mob]).max() > 0.1                                          # ... and so do the forces (kJ/mol/nm)
        for k in SAME_BITS:
            assert t1[k] == t0[k], (k, t1[k], t0[k])
        assert np.all(f1[~mob] == 0.0)
        if t1[9] != 0.0:
            want = systems.dispersion_correction_energy(s_sw, zero_epsilon=lig)
            assert abs(t1[9] - want) <= 1e-12 * abs(want) and t1[9] != t0[9], (t1[9], want, t0[9])
        else:
            assert t0[9] == 0.0
    assert not fails, fails


# ---- 1. differential parity, double precision
@pytest.mark.parametrize("row", ("tile", "sub", "atom", "pme"))
def test_differential_parity_double(Engine, tol_box, tune, row):
    _set_tuning(row, tune)
    s, _ = _row_system(row, tol_box)
    sw = systems.with_switch_distance(s, RS)
    g0, g1 = Engine(s, _data(1)), Engine(sw, _data(1))
    try:
        assert g0.lj_switch() == (0.0, 0) and g1.lj_switch()[0] == RS
        _differential("double", row, row if row not in S23K_ROWS else "s23k", sw, np.asarray(s.positions), g0, g1, 1e-9 if row in S23K_ROWS else 1e-10)
        _check_path(row, 1, g0); _check_path(row, 1, g1)
        assert g0.lj_switch() == (0.0, 0) and g1.lj_switch()[1] > 0
    finally:
        g0.close(); g1.close()


# ---- 2. mixed precision against double, both switched
MIXED_CASES = [("tile", -1), ("sub", -1), ("atom", 0), ("atom", -1), ("atom", 2), ("frag", -1), ("pme", -1)]


@pytest.fixture(scope="module")
def switched_double(Engine, tol_box):
    """energy terms, energy and forces of the switched double-precision engine of a row's System (default tuning: the reference-grade
    kernels), made once and left unchanged"""
    cache = {}

    def get(row):
        key = "s23k" if row in S23K_ROWS else ("pme" if row == "pme" else "tile")
        if key not in cache:
            s, _ = _row_system(row, tol_box)
            g = Engine(systems.with_switch_distance(s, RS), _data(1))
            cache[key] = _static(g)
            g.close()
        return cache[key]
    return get


@pytest.mark.parametrize("row,k2_dense", MIXED_CASES)
def test_mixed_against_double(Engine, tol_box, tune, switched_double, row, k2_dense):
    """k2_dense = 0 / auto / 2 on the `atom` row: the lane layout, the fp32 dense body and the fp64 dense body of the alchemical kernel."""
    want = switched_double(row)                                                      # (under the default tuning)
    _set_tuning(row, tune, **({"k2_dense": k2_dense} if row == "atom" else {}))
    s, _ = _row_system(row, tol_box)
    sw = systems.with_switch_distance(s, RS)
    g = Engine(sw, _data(0))
    mob = s.mass > 0
    fails = []
    try:
        if row == "atom":
            assert g.stats()["alchemical_kernel"] == {0: 0, -1: 1, 2: 2}[k2_dense], g.stats()
        for (ls, le), (t0, e0, f0), (t1, e1, f1) in zip(LAMBDAS, want, _static(g)):
            res = {"terms": max(abs(t1[k] - t0[k]) / max(abs(t0[k]), 1.0) for k in range(10)),
                   "potential_energy": abs(e1 - e0) / max(abs(e0), 1.0),
                   "forces": np.abs(f1[mob] - f0[mob]).max() / np.abs(f0[mob]).max()}
            for what, r in res.items():
                _report("mixed", row if row != "atom" else "atom/%d" % k2_dense, "%s at (%g, %g)" % (what, ls, le), r, 1e-5)
                if not r <= 1e-5:
                    fails.append((what, ls, le, r))
        _check_path(row, 0, g)
        assert g.lj_switch()[0] == RS and g.lj_switch()[1] > 0
    finally:
        g.close()
    assert not fails, fails


# ---- 3. alchemical region sizes
@pytest.mark.parametrize("n_alch", (1, 17, 64))
def test_alchemical_region_sizes(Engine, tol_box, n_alch):
    """The smallest region, one past a power of two, the limit (tests/alch_regions.py: compact)."""
    s0, _ = tol_box
    s = ar.with_region(s0, ar.compact(s0, n_alch))
    sw = systems.with_switch_distance(s, RS)
    g0, g1 = Engine(s, _data(1)), Engine(sw, _data(1))
    try:
        _differential("regions", "n=%d" % n_alch, "tol_box/%d" % n_alch, sw, np.asarray(s.positions), g0, g1, 1e-10)
    finally:
        g0.close(); g1.close()


# ---- 4. force is the gradient of the energy
def test_force_is_energy_gradient(Engine, tol_box):
    s0, _ = tol_box
    sw = systems.with_switch_distance(s0, RS)
    x0 = np.array(sw.positions, dtype=np.float64)
    ls, le = LAMBDAS[1]
    d = _delta("tol_box/15", sw, x0, ls)
    shell = d["atoms_in_shell"]
    atoms = [0, 7, 14] + [int(a) for a in shell[np.argsort(-np.abs(d["dF"][shell]).max(1), kind="stable")[:4]]]     # ligand atoms and the atoms the switch pushes hardest
    g = Engine(sw, _data(1))
    try:
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        f = g.get_forces()
        h = 1e-5
        worst = 0.0
        for a in atoms:
            for k in range(3):
                xp = x0.copy(); xp[a, k] += h; g.set_positions(xp); ep = g.potential_energy()
                xm = x0.copy(); xm[a, k] -= h; g.set_positions(xm); em = g.potential_energy()
                num = -(ep - em) / (2 * h)
                worst = max(worst, abs(f[a, k] - num) / (2e-5 * abs(num) + 2e-3))
                assert f[a, k] == pytest.approx(num, rel=2e-5, abs=2e-3), (a, k)
        _report("gradient", "tol_box", "worst |f - num| / bound", worst, 1.0)
    finally:
        g.close()


# ---- 5. off means off
@pytest.mark.parametrize("precision", (1, 0))
def test_off_means_off(Engine, tol_box, precision):
    s, v = tol_box
    n = 12

    def run(system):
        g = Engine(system, _data(precision, n))
        st, none_yet = _static(g), g.lj_switch()
        g.close()
        g = Engine(system, _data(precision, n))                                          # (a fresh engine for the switch, as the symmetry tests take one)
        g.set_velocities(v)
        w = g.run_switch(n, trace=True)
        out = (st, w, g.get_positions(), g.lj_switch(), none_yet)
        g.close()
        return out
    base = run(s)
    assert base[3] == (0.0, 0)
    for d in (0.0, s.cutoff, 1.5):
        got = run(systems.with_switch_distance(s, d))
        assert got[3] == (0.0, 0)
        for (t0, e0, f0), (t1, e1, f1) in zip(base[0], got[0]):
            assert np.array_equal(t0, t1) and e0 == e1 and np.array_equal(f0, f1)
        assert np.array_equal(base[1], got[1]) and np.array_equal(base[2], got[2]) and np.abs(base[1]).max() > 1e-3
    on = run(systems.with_switch_distance(s, RS))
    assert on[3][0] == RS and on[3][1] > 0 and on[4][0] == RS
    assert on[0][0][1] != base[0][0][1] and not np.array_equal(on[1], base[1])


# ---- 6. batch
@pytest.mark.parametrize("precision", (0, 1))
def test_batch_equals_lone_chains(Engine, tol_box, precision):
    from blues_amd.engine import EngineError, NativeBatch
    s, v = tol_box
    sw = systems.with_switch_distance(s, RS)
    n = 12

    def chains(system_of):
        out = []
        for r in range(2):
            g = Engine(system_of(r), _data(precision, n, seed=11 + r, replica=r)); g.set_velocities(v * (1.0 + 0.1 * r)); out.append(g)
        return out
    lone = chains(lambda r: sw)
    want = [(g.run_switch(n, trace=True), g.get_positions(), g.get_global("protocol_work")) for g in lone]
    for g in lone:
        g.close()
    engs = chains(lambda r: sw)
    batch = NativeBatch(engs)
    _, w = batch.step(n, trace=True)
    for r, g in enumerate(engs):
        assert np.array_equal(w[r], want[r][0]) and np.array_equal(g.get_positions(), want[r][1]) and g.get_global("protocol_work") == want[r][2]
        assert g.lj_switch()[0] == RS
    assert engs[0].lj_switch()[1] > 0 and batch.stats()["fallback_steps"] == 0
    batch.close()
    for g in engs:
        g.close()
    mixed = chains(lambda r: sw if r == 0 else s) + chains(lambda r: systems.with_switch_distance(s, 0.9) if r == 0 else sw)
    for pair in (mixed[:2], mixed[2:]):
        with pytest.raises(EngineError, match="switch"):
            NativeBatch(pair)
    for g in mixed:
        g.close()


# ---- 7. box change
def test_box_change(Engine, tol_box):
    s = systems.with_reciprocal_space(tol_box[0])
    sw = systems.with_switch_distance(s, RS)
    scale = np.array([1.02, 1.03, 1.01])
    box2 = np.asarray(s.box, dtype=np.float64) * scale
    x2 = np.asarray(s.positions) * scale
    assert s.cutoff < 0.5 * box2.min() and s.cutoff < 0.5 * np.min(s.box)
    s2 = dataclasses.replace(sw, box=box2, positions=x2)                           # (the mesh stays the engine's: set_box keeps the grid)
    g0, g1 = Engine(s, _data(1)), Engine(sw, _data(1))
    try:
        before = g1.energy_terms()[9]
        for g in (g0, g1):
            g.set_box(box2); g.set_positions(x2)
        lig = np.asarray(s.alchemical_atoms, dtype=np.int64)
        want = systems.dispersion_correction_energy(s2, zero_epsilon=lig)
        t9 = g1.energy_terms()[9]
        assert abs(t9 - want) <= 1e-12 * abs(want) and t9 != before
        _differential("box", "pme", "tol_box/scaled", s2, x2, g0, g1, 1e-10)
    finally:
        g0.close(); g1.close()


# ---- 8. refusals
def test_refusals_name_their_reason(Engine, tol_box):
    from blues_amd import _lib
    lib = _lib.load()
    s = systems.with_switch_distance(tol_box[0], RS)
    sd, keep_s = s.to_desc(); idesc, keep_i = _data(1).to_desc()

    def create(distance, reserved=0.0, method=None):
        ext = s.ext_desc(); ext.lj_switch_distance = distance; ext.lj_switch_reserved = reserved
        h = ctypes.c_void_p()
        rc = lib.blues_engine_create_ext(ctypes.byref(sd), ctypes.byref(idesc), None, ctypes.byref(ext), 0, ctypes.byref(h))
        msg = lib.blues_last_error(None).decode()
        out = (ctypes.c_double * 2)(-1.0, -1.0)
        if rc == 0:
            assert lib.blues_get_lj_switch(h, out) == 0
            lib.blues_engine_destroy(h)
        return rc, msg, (out[0], out[1])
    for bad in (-0.1, float("nan"), float("inf")):
        rc, msg, _ = create(bad)
        assert rc != 0 and "lj_switch_distance" in msg and "switch" in msg, msg
    rc, msg, _ = create(RS, reserved=1.0)
    assert rc != 0 and "lj_switch_reserved" in msg
    assert create(RS)[::2] == (0, (RS, 0.0))
    assert create(0.0)[::2] == (0, (0.0, 0.0)) and create(s.cutoff)[::2] == (0, (0.0, 0.0)) and create(7.0)[::2] == (0, (0.0, 0.0))   # no switch, not an error
    # measure_shadow_work / measure_heat run on a switched System (they use the energy forms of the same pair bodies): nothing is refused
    data = integrators.generateNCMCIntegrator(nstepsNC=4, dt=0.004, temperature=300.0, seed=3, measure_shadow_work=True, measure_heat=True).to_data(precision=1)
    g = Engine(s, data)
    g.set_velocities(tol_box[1]); g.run_switch(4)
    assert np.isfinite(g.get_global("shadow_work")) and g.lj_switch()[0] == RS
    g.close()
