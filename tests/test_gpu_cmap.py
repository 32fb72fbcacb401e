"""GPU suite: CMAP torsion correction maps (kernels_bonded.h: T_CMAP) against the numpy / scipy reference tests/cmap_reference.py,
which tests/test_cmap_cpu.py pins by itself.  The CMAP part of an engine's numbers is what it gives minus what the same System
without maps gives; the bar for that subtraction in double precision is the one tests/test_gpu_implicit_solvent.py uses for its own:
1e-12 of the largest force."""
import copy
import ctypes
import dataclasses

import numpy as np
import pytest

import cmap_cases as cc
import cmap_reference as ref
import symmetry as sym
from blues_amd import _abi, integrators, systems

pytestmark = pytest.mark.gpu
TWO_PI = 2.0 * np.pi
EMPTY = np.zeros((0, 9), np.int32)


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _integ(nsteps=20, dt=0.002, seed=7, **kw):
    return integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=dt, temperature=300.0, seed=seed, **kw)


def without(s):
    return dataclasses.replace(s, cmap_maps=(), cmap_torsions=EMPTY)


def _box(s):
    return None if int(s.nonbonded_method) == _abi.NB_NOCUTOFF else np.asarray(s.box, dtype=np.float64).reshape(-1)[:3]


def _check_against_reference(g, gp, s, x, tag, force_bar=1e-12):
    """energy term [2], forces and angles of engine g minus those of gp (the same System without maps) against the reference at x"""
    g.set_positions(x); gp.set_positions(x)
    e_ref, f_ref = ref.energy_forces(s.cmap_maps, s.cmap_torsions, x, _box(s))
    tg, tp = g.energy_terms(), gp.energy_terms()
    fg, fp = g.get_forces(), gp.get_forces()
    mob = np.asarray(s.mass) > 0
    big = max(np.abs(fg).max(), np.abs(f_ref).max())
    de, df = abs((tg[2] - tp[2]) - e_ref), np.abs((fg - fp)[mob] - f_ref[mob]).max()
    da = np.abs(g.cmap_angles() - ref.angles(s.cmap_torsions, x, _box(s))).max()
    print("CMAP %s: energy %.12g (d %.2e), force part d %.2e of largest force %.4g, angles d %.2e" % (tag, e_ref, de, df / big, big, da))
    assert de <= 1e-12 * max(1.0, abs(e_ref)), (tag, tg[2] - tp[2], e_ref)
    for k in range(_abi.N_ENERGY_TERMS):
        if k != 2:
            assert abs(tg[k] - tp[k]) <= force_bar * max(1.0, abs(tp[k])), (tag, k, tg[k], tp[k])
    assert abs(g.potential_energy() - gp.potential_energy() - e_ref) <= max(1e-12, force_bar) * max(1.0, abs(gp.potential_energy()))
    assert df <= force_bar * big, (tag, df / big)
    assert np.all(fg[~mob] == 0.0)
    assert da <= 1e-12, (tag, da)
    return e_ref, f_ref


def _top_of_range():
    """five atoms whose first dihedral is a negative angle so small that the shift into [0, 2 pi) rounds to 2 pi itself: phi / delta
    rounds to n, and the patch index has to be clamped to n - 1"""
    for k in range(1, 400):
        x = cc.five_atoms(-k * 2e-17, 2.2)
        if ref.dihedral(x[:4])[0] == TWO_PI:
            return x
    raise AssertionError("no geometry found whose dihedral rounds to 2 pi")


# ---- 1. one term, every branch
@pytest.mark.parametrize("n", [4, 24])
def test_one_term_every_branch(Engine, n):
    """A five-atom chain, NoCutoff, double precision; (phi, psi) in an interior patch, in the first and the last patch of either axis
    within 1e-6 rad of the seam, on a grid point, and at a phi that rounds to 2 pi (patch n - 1, phi / delta = n)."""
    d = TWO_PI / n
    cases = {"interior": (1.37 * d, 2.61 * d), "phi just above 0": (5e-7, 2.2 * d), "phi just below 2 pi": (TWO_PI - 5e-7, 2.2 * d),
             "psi just above 0": (1.3 * d, 5e-7), "psi just below 2 pi": (1.3 * d, TWO_PI - 5e-7), "grid point": (2 * d, 3 * d),
             "last patches": ((n - 0.4) * d, (n - 0.7) * d)}
    geometries = {k: cc.five_atoms(*v) for k, v in cases.items()}
    geometries["phi rounds to 2 pi"] = _top_of_range()
    tors = [[0, 0, 1, 2, 3, 1, 2, 3, 4]]
    s = cc.chain(geometries["interior"], [cc.random_map(n, seed=n)], tors)
    data = _integ().to_data(precision=1)
    g, gp = Engine(s, data), Engine(without(s), data)
    for tag, x in geometries.items():
        a = ref.angles(tors, x)[0]
        if tag in cases:
            assert np.abs(a - np.array(cases[tag])).max() < 1e-12, (tag, a)      # (the geometry is where the case wants it)
            i, j = int(np.floor(a[0] / d)), int(np.floor(a[1] / d))
            expect = {"interior": (1, 2), "phi just above 0": (0, 2), "phi just below 2 pi": (n - 1, 2), "psi just above 0": (1, 0),
                      "psi just below 2 pi": (1, n - 1), "last patches": (n - 1, n - 1)}.get(tag)
            assert expect is None or (i, j) == expect, (tag, i, j)
        else:
            assert a[0] == TWO_PI and int(np.floor(a[0] / d)) == n
        e, f = _check_against_reference(g, gp, s, x, "n=%d %s" % (n, tag))
        assert np.abs(f).max() > 1.0       # (there is a force to compare)
    g.close(); gp.close()


# ---- 2. forces are the gradient, on device numbers only
def _fd_disagreement(g, x, atoms, h=1e-5):
    g.set_positions(x)
    f = g.get_forces()
    worst = 0.0
    for a in atoms:
        for k in range(3):
            xp, xm = x.copy(), x.copy(); xp[a, k] += h; xm[a, k] -= h
            g.set_positions(xp); ep = g.potential_energy()
            g.set_positions(xm); em = g.potential_energy()
            worst = max(worst, abs(-(ep - em) / (2 * h) - f[a, k]))
    return worst, np.abs(f).max()


def test_forces_are_the_gradient_of_the_energy(Engine):
    """Central differences of potential_energy() (h = 1e-5 nm) against get_forces() on the five atoms, with the map and -- the bar --
    on the same System without it (bonds and a plain torsion): the finite-difference error sets the bar, margin 10.  Measured:
    4.811e-5 kJ/mol/nm with the map, 4.814e-5 without (the stiff bonds' own finite-difference error; forces up to 2621)."""
    x = cc.five_atoms(2.1, 4.4)
    x += np.random.default_rng(3).normal(size=x.shape) * 0.004       # (off the bonds' minimum: every term pulls)
    s = cc.chain(cc.five_atoms(2.1, 4.4), [cc.surface_map(24)], [[0, 0, 1, 2, 3, 1, 2, 3, 4]])
    data = _integ().to_data(precision=1)
    g, gp = Engine(s, data), Engine(without(s), data)
    d_map, big_map = _fd_disagreement(g, x, range(5))
    d_plain, big_plain = _fd_disagreement(gp, x, range(5))
    _, f_ref = ref.energy_forces(s.cmap_maps, s.cmap_torsions, x)
    print("CMAP finite differences: with the map %.3e kJ/mol/nm (largest force %.4g), plain terms alone %.3e (largest force %.4g); CMAP force up to %.4g"
          % (d_map, big_map, d_plain, big_plain, np.abs(f_ref).max()))
    assert np.abs(f_ref).max() > 10.0
    assert d_map <= 10.0 * d_plain, (d_map, d_plain)
    g.close(); gp.close()


# ---- 3. two dihedrals: net force and net torque of the term
@pytest.mark.parametrize("form", ["five atoms", "eight atoms"])
def test_net_force_and_torque_vanish(Engine, form):
    rng = np.random.default_rng(17)
    x = np.cumsum(rng.normal(size=(8, 3)) * 0.09 + np.array([0.11, 0.0, 0.0]), axis=0)
    tors = [[0, 0, 1, 2, 3, 1, 2, 3, 4]] if form == "five atoms" else [[0, 0, 1, 2, 3, 4, 5, 6, 7]]
    s = cc.chain(x, [cc.random_map(12)], tors)
    data = _integ().to_data(precision=1)
    g, gp = Engine(s, data), Engine(without(s), data)
    _, f_ref = _check_against_reference(g, gp, s, x, form)
    f = g.get_forces() - gp.get_forces()
    big = np.abs(f).max()
    # (atoms outside the term: nothing but the rounding of bond forces at their minimum, which the two instantiations contract differently)
    assert big > 1.0 and (form == "five atoms") == bool(np.abs(f[5:]).max() <= 1e-12 * big)
    print("CMAP %s: net force %.2e, net torque %.2e of the largest force %.4g" % (form, np.abs(f.sum(0)).max() / big, np.abs(np.cross(x, f).sum(0)).max() / big, big))
    assert np.abs(f.sum(0)).max() <= 1e-10 * big
    assert np.abs(np.cross(x, f).sum(0)).max() <= 1e-10 * big
    g.close(); gp.close()


# ---- 4. real topologies
def _ring_path(s, start, length=5):
    """`length` atoms bonded in a row (harmonic bonds only: heavy atoms), from `start`"""
    nb = {}
    for a, b in np.asarray(s.bond_atoms):
        nb.setdefault(int(a), []).append(int(b)); nb.setdefault(int(b), []).append(int(a))
    def walk(path):
        if len(path) == length:
            return path
        for q in nb.get(path[-1], []):
            if q not in path:
                out = walk(path + [q])
                if out:
                    return out
        return None
    for first in range(start, start + 15):
        p = walk([first])
        if p:
            return p
    raise AssertionError("no bonded path")


def _toluene_box_with_map(tol_box, straddle):
    s = systems.with_reciprocal_space(tol_box[0])
    a = _ring_path(s, 0)        # (the box's one toluene: the ligand)
    s = dataclasses.replace(s, cmap_maps=(cc.surface_map(24) * 3.0,), cmap_torsions=np.array([[0, a[0], a[1], a[2], a[3], a[1], a[2], a[3], a[4]]], np.int32))
    x = np.array(s.positions, dtype=np.float64)
    box = _box(s)
    if straddle:      # everything translated so that the middle atom of the term sits on the box face, every atom wrapped into the box by itself
        x = x - x[a[2]] + np.array([0.0, 0.3, 0.4]) * box
        x = x - box * np.floor(x / box)
        assert len(set(np.round((x[a] - x[a[2]]) / box)[:, 0])) > 1          # (the term's atoms lie on both sides of the face)
    return s, x


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("case", ["vacDivaline", "toluene box", "toluene box, across a face"])
def test_real_topologies(Engine, tol_box, tune, case, precision):
    """Double precision: the CMAP part to 1e-12 of the largest force.  Mixed precision: everything that is not CMAP is computed by the
    same kernels from the same numbers in both engines (the decomposition pinned to be the same: an engine with maps never takes the
    fused force launch), the bonded entries are fp64 in both -- the same subtraction, the same bar."""
    tune(fuse_forces=0)
    if case == "vacDivaline":
        s = cc.divaline([cc.random_map(24)])
        x = s.positions
    else:
        s, x = _toluene_box_with_map(tol_box, case.endswith("face"))
    data = _integ().to_data(precision=precision)
    g, gp = Engine(s, data), Engine(without(s), data)
    for ls, le in ((1.0, 1.0), (0.4, 0.2)):       # (not alchemical: the same part at any lambda)
        for e in (g, gp):
            e.set_global("lambda_sterics", ls); e.set_global("lambda_electrostatics", le)
        _check_against_reference(g, gp, s, x, "%s precision=%d lambda=(%.1f, %.1f)" % (case, precision, ls, le))
    g.close(); gp.close()


# ---- 5. frozen atoms
@pytest.mark.parametrize("pattern", ["none", "one end", "the middle three", "all five"])
def test_frozen_atoms_of_the_term(Engine, pattern):
    rng = np.random.default_rng(23)
    x = np.cumsum(rng.normal(size=(7, 3)) * 0.09 + np.array([0.11, 0.0, 0.0]), axis=0)
    s = cc.chain(x, [cc.random_map(8)], [[0, 1, 2, 3, 4, 2, 3, 4, 5]])
    frozen = {"none": [], "one end": [1], "the middle three": [2, 3, 4], "all five": [1, 2, 3, 4, 5]}[pattern]
    sf = systems.freeze_atoms(s, frozen)
    data = _integ().to_data(precision=1)
    g, gp, g0 = Engine(sf, data), Engine(without(sf), data), Engine(s, data)
    e_ref, f_ref = _check_against_reference(g, gp, sf, x, "frozen: " + pattern)
    g0.set_positions(x)
    assert g.energy_terms()[2] == g0.energy_terms()[2]          # the energy does not know who is frozen
    f = g.get_forces()
    assert np.all(f[frozen] == 0.0) and np.abs(f_ref[frozen]).max(initial=1.0) > 0.0
    for e in (g, gp, g0):
        e.close()


# ---- 6. dynamics
def _mostly_frozen_box(tol_box):
    s, v = tol_box
    lig = np.arange(15)
    near = systems.nearest_molecules(s, lig, 120, exclude_idx=lig)
    sf = systems.freeze_except(s, np.concatenate([lig, near]))
    a = _ring_path(sf, 0)       # (on the ligand: mobile)
    sf = dataclasses.replace(sf, cmap_maps=(cc.surface_map(24) * 3.0,), cmap_torsions=np.array([[0, a[0], a[1], a[2], a[3], a[1], a[2], a[3], a[4]]], np.int32))
    return sf, v * (sf.mass[:, None] > 0)


def _dynamics_system(tol_box, kind):
    if kind == "vacDivaline":
        return cc.divaline([cc.random_map(24)]), None
    return _mostly_frozen_box(tol_box)


@pytest.mark.parametrize("kind", ["vacDivaline", "mostly frozen toluene box"])
def test_batch_member_equals_the_lone_chain(Engine, tol_box, tune, kind):
    """20 steps of the default switch: every member of a NativeBatch of 8 equals the same chain alone bit for bit, and the switch
    with the map is not the switch without it."""
    from blues_amd.engine import NativeBatch
    s, v = _dynamics_system(tol_box, kind)
    R, n = 8, 20
    tune(assume_batch=R)

    def make(system):
        out = []
        for r in range(R):
            g = Engine(system, _integ(nsteps=n, seed=40 + r).to_data(precision=0, replica=r))
            if v is None:
                g.set_velocities_to_temperature(300.0, seed=90 + r)
            else:
                g.set_velocities(v * (1.0 + 0.03 * r))
            out.append(g)
        return out
    solo = make(s)
    for g in solo:
        g.step(7); g.step(n - 7)
    bat = make(s)
    B = NativeBatch(bat)
    B.step(7); B.step(n - 7)
    assert B.stats()["fallback_steps"] == 0
    for r in range(R):
        assert solo[r].get_global("protocol_work") == bat[r].get_global("protocol_work"), r
        assert np.array_equal(solo[r].get_positions(), bat[r].get_positions()), r
        assert np.all(np.isfinite(bat[r].get_positions()))
    plain = make(without(s))[0]
    plain.step(n)
    assert not np.array_equal(plain.get_positions(), solo[0].get_positions())
    # a batch may not mix members with and without maps
    from blues_amd.engine import EngineError
    with pytest.raises(EngineError, match="CMAP"):
        NativeBatch(make(s)[:1] + make(without(s))[1:2]).step(1)
    B.close()


@pytest.mark.parametrize("kind", ["vacDivaline", "mostly frozen toluene box"])
def test_ledger_closes_with_the_map(Engine, tol_box, kind):
    """Double precision, measure_shadow_work = measure_heat = 1: dE = dW + shadow + heat + sum dKE_cm after every step to the bar of
    tests/test_gpu_energy_ledger.py (1e-9 max(1, |W|)): the energy form and the force form see the same term in every path."""
    s, v = _dynamics_system(tol_box, kind)
    s = dataclasses.replace(s, remove_cm_motion=False)
    start = Engine(s, _integ(nsteps=0, seed=1).to_data(precision=1))      # (a start state the first-step block leaves as it is)
    if v is None:
        start.set_velocities_to_temperature(300.0, seed=5)
    else:
        start.set_velocities(v)
    start.step(1)
    x, v = start.get_positions(), start.get_velocities()
    start.close()
    g = Engine(s, _integ(nsteps=20, seed=3, measure_shadow_work=True, measure_heat=True).to_data(precision=1))
    g.set_positions(x); g.set_velocities(v)
    E0 = g.potential_energy() + g.kinetic_energy()
    worst = big = 0.0
    for k in range(20):
        g.step(1)
        W, S, Q = g.get_global("protocol_work"), g.get_global("shadow_work"), g.get_global("heat")
        resid = (g.potential_energy() + g.kinetic_energy() - E0) - W - S - Q
        assert abs(resid) <= 1e-9 * max(1.0, abs(W)), (k + 1, resid, W)
        worst, big = max(worst, abs(resid)), max(big, abs(S))
    print("CMAP ledger %s: largest residual %.3e kJ/mol over 20 steps, largest |shadow work| %.3e" % (kind, worst, big))
    assert big > 0.0
    g.close()


def test_minimize_converges_with_the_map(Engine):
    s = cc.divaline([cc.random_map(24)])
    g = Engine(s, _integ().to_data(precision=1))
    e0 = g.potential_energy()
    out = g.minimize(tolerance=10.0, max_iterations=5000)
    print("CMAP minimise: %s" % (out,))
    assert out["converged"] == 1 and out["e_final"] < out["e_initial"] and out["e_final"] < e0      # (e_initial: after the constraints' polish of the start)
    assert abs(g.potential_energy() - out["e_final"]) <= 1e-9 * abs(out["e_final"])
    g.close()


def test_md_leg_runs_with_the_map(Engine):
    s = cc.divaline([cc.random_map(24)])
    data = integrators.LangevinIntegrator(300.0, 1.0, 0.002, seed=3).to_data(precision=0)
    g, gp = Engine(s, data), Engine(without(s), data)
    for e in (g, gp):
        e.set_velocities_to_temperature(300.0, seed=4)
        e.step(20)
    pe, ke = g.energies()
    assert np.isfinite(pe) and np.isfinite(ke) and np.all(np.isfinite(g.get_positions()))
    assert not np.array_equal(g.get_positions(), gp.get_positions())
    a = g.cmap_angles()
    assert a.shape == (1, 2) and np.abs(a - ref.angles(s.cmap_torsions, g.get_positions())).max() <= 1e-12      # (the current device positions)
    assert gp.cmap_angles().shape == (0, 2)
    g.close(); gp.close()


# ---- 7. permutation
def test_permuted_atoms(Engine):
    s = cc.divaline([cc.random_map(24)])
    perm = sym.scatter_perm(s.n_atoms, 12)
    sp, _, m = sym.permute_atoms(s, None, perm)
    new_of_old = np.empty(s.n_atoms, np.int64); new_of_old[perm] = np.arange(s.n_atoms)
    tors = np.array(s.cmap_torsions); tors[:, 1:] = new_of_old[tors[:, 1:]]
    sp = dataclasses.replace(sp, cmap_torsions=tors.astype(np.int32))
    data = _integ().to_data(precision=1)
    g, h = Engine(s, data), Engine(sp, data)
    ta, tb = g.energy_terms(), h.energy_terms()
    for k in range(_abi.N_ENERGY_TERMS):
        assert abs(ta[k] - tb[k]) <= 1e-12 * max(1.0, abs(ta[k])), (k, ta[k], tb[k])
    fa, fb = g.get_forces(), m.vectors(h.get_forces())
    assert np.abs(fa - fb).max() <= 1e-12 * np.abs(fa).max()
    assert np.abs(g.cmap_angles() - h.cmap_angles()).max() <= 1e-12
    g.close(); h.close()


# ---- 8. what the library refuses (the wrapper's own check switched off: the descriptor reaches the C-ABI as a foreign caller's would)
def _bad_systems():
    good = cc.divaline([cc.surface_map(8)])
    t = good.cmap_torsions
    def tor(col, val):
        q = t.copy(); q[0, col] = val
        return q
    inf = cc.surface_map(8); inf[3, 2] = np.inf
    r = dataclasses.replace
    return {"size 3": ("size 3x3; a map is n x n with n from 4 to 64", r(good, cmap_maps=(np.zeros((3, 3)),))),
            "size 65": ("size 65x65", r(good, cmap_maps=(np.zeros((65, 65)),))),
            "not finite": ("map 0: an energy is not finite", r(good, cmap_maps=(inf,))),
            "missing map": ("torsion 0: map 1 of 1", r(good, cmap_torsions=tor(0, 1))),
            "no maps": ("torsion 0: map 0 of 0", r(good, cmap_maps=())),
            "atom": ("torsion 0: atom index out of range", r(good, cmap_torsions=tor(8, 35))),
            "negative atom": ("torsion 0: atom index out of range", r(good, cmap_torsions=tor(1, -1))),
            "equal atoms": ("two equal atoms within one dihedral", r(good, cmap_torsions=tor(8, int(t[0, 6]))))}


@pytest.mark.parametrize("case", sorted(_bad_systems()))
def test_creation_errors_of_the_library(Engine, monkeypatch, case):
    from blues_amd.engine import EngineError
    match, s = _bad_systems()[case]
    with pytest.raises(EngineError, match=match):      # the wrapper's own refusal
        Engine(s, _integ().to_data(precision=0))
    monkeypatch.setattr(_abi.SystemData, "check_cmap", lambda self: None)
    with pytest.raises(EngineError, match=match):      # the library's
        Engine(s, _integ().to_data(precision=0))


def test_struct_sizes_the_library_accepts(Engine):
    """struct_size 8 (a caller from before the maps: none are read) and this library's; anything else is refused by name."""
    from blues_amd import _lib
    lib = _lib.load()
    s = cc.divaline([cc.surface_map(8)])
    sd, keep_s = s.to_desc(); idesc, keep_i = _integ().to_data(precision=0).to_desc()

    def create(size):
        ext = s.ext_desc(); ext.struct_size = size
        h = ctypes.c_void_p()
        rc = lib.blues_engine_create_ext(ctypes.byref(sd), ctypes.byref(idesc), None, ctypes.byref(ext), 0, ctypes.byref(h))
        msg = lib.blues_last_error(None).decode()
        out = np.full(2, -1.0)
        if rc == 0:
            x = np.ascontiguousarray(s.positions, dtype=np.float64)
            assert lib.blues_set_positions(h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), s.n_atoms) == 0
            assert lib.blues_get_cmap_angles(h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
            lib.blues_engine_destroy(h)
        return rc, msg, out
    rc, _, out = create(ctypes.sizeof(_abi.BluesSystemExt))
    assert rc == 0 and np.all(out >= 0.0)
    rc, _, out = create(_abi.SYSTEM_EXT_SIZE_V1)
    assert rc == 0 and np.all(out == -1.0)             # no maps were read: nothing is written
    for size in (4, 12, ctypes.sizeof(_abi.BluesSystemExt) + 8):
        rc, msg, _ = create(size)
        assert rc != 0 and "struct_size" in msg
