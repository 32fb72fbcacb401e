"""GPU suite: CHARMM's Urey-Bradley terms and harmonic impropers (kernels_bonded.h: T_UREY, T_IMPR) and the 1-4 exceptions of a chamber
topology against the numpy reference tests/charmm_reference.py, which tests/test_charmm_cpu.py pins by itself.  The terms' part of an
engine's numbers is what it gives minus what the same System without them gives; the bars are those of tests/test_gpu_cmap.py for
this same fp64 kernel: 1e-12 max(1, |E|) for energies, 1e-12 of the largest force for forces."""
import ctypes
import dataclasses

import numpy as np
import pytest

import charmm_cases as cc
import charmm_reference as ref
import symmetry as sym
from blues_amd import _abi, integrators, systems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _integ(nsteps=20, dt=0.002, seed=7, **kw):
    return integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=dt, temperature=300.0, seed=seed, **kw)


def _box(s):
    return None if int(s.nonbonded_method) == _abi.NB_NOCUTOFF else np.asarray(s.box, dtype=np.float64).reshape(-1)[:3]


def _check_against_reference(g, gp, s, x, tag):
    """energy terms [0] and [2], the total and the forces of engine g minus those of gp (the same System without the terms) against
    the reference at x; gp = None: a System that has nothing else, the engine's own numbers"""
    g.set_positions(x)
    eu, ei, f_ref = ref.energy_forces(s, x, _box(s))
    tg, fg, pg = g.energy_terms(), g.get_forces(), g.potential_energy()
    if gp is None:
        tp, fp, pp = np.zeros(_abi.N_ENERGY_TERMS), np.zeros_like(fg), 0.0
    else:
        gp.set_positions(x)
        tp, fp, pp = gp.energy_terms(), gp.get_forces(), gp.potential_energy()
    mob = np.asarray(s.mass) > 0
    big = max(np.abs(fg).max(), np.abs(f_ref).max())
    du, di, dt = abs((tg[0] - tp[0]) - eu), abs((tg[2] - tp[2]) - ei), abs((pg - pp) - (eu + ei))
    df = np.abs((fg - fp)[mob] - f_ref[mob]).max() if mob.any() else 0.0
    print("CHARMM %s: Urey-Bradley %.12g (d %.2e), improper %.12g (d %.2e), total d %.2e, force part d %.2e of largest force %.4g"
          % (tag, eu, du, ei, di, dt, df / big if big else 0.0, big))
    assert du <= 1e-12 * max(1.0, abs(eu)), (tag, tg[0] - tp[0], eu)
    assert di <= 1e-12 * max(1.0, abs(ei)), (tag, tg[2] - tp[2], ei)
    assert dt <= 1e-12 * max(1.0, abs(eu + ei), abs(pp)), (tag, pg - pp, eu + ei)
    for k in range(_abi.N_ENERGY_TERMS):
        if k not in (0, 2):
            assert abs(tg[k] - tp[k]) <= 1e-12 * max(1.0, abs(tp[k])), (tag, k, tg[k], tp[k])
    assert df <= 1e-12 * big, (tag, df / big)
    assert np.all(fg[~mob] == 0.0)
    return eu, ei, f_ref


# ---- 6. known geometries
@pytest.mark.parametrize("precision", [1, 0])
def test_one_improper_at_known_angles(Engine, precision):
    """Four atoms, NoCutoff, no charges, epsilon 0: psi = 0 exactly, +-1e-7 (where acos would keep half its digits), +-0.3, pi - 1e-7,
    and psi = -3.0 with psi0 = 3.0, where the wrapped difference is 2 pi - 6 and not -6."""
    k = 180.0
    data = _integ().to_data(precision=precision)
    s = cc.bare(ref.four_atoms(0.3), impr=([[0, 1, 2, 3]], [[0.0, k]]))
    g = Engine(s, data)
    for psi in (0.0, 1e-7, -1e-7, 0.3, -0.3, np.pi - 1e-7):
        x = ref.four_atoms(psi)
        assert abs(ref.improper_angles(s.improper_atoms, x)[0] - psi) <= 1e-12          # (the geometry is where the case wants it)
        if psi == 0.0:
            assert ref.improper_angles(s.improper_atoms, x)[0] == 0.0
        eu, ei, f = _check_against_reference(g, None, s, x, "psi = %r precision=%d" % (psi, precision))
        assert ei == pytest.approx(k * psi * psi, rel=1e-8, abs=1e-300) and (psi == 0.0) == (np.abs(f).max() == 0.0)
    g.close()
    s = cc.bare(ref.four_atoms(-3.0), impr=([[0, 1, 2, 3]], [[3.0, k]]))
    g = Engine(s, data)
    assert abs(ref.improper_angles(s.improper_atoms, s.positions)[0] + 3.0) <= 1e-12
    eu, ei, f = _check_against_reference(g, None, s, s.positions, "psi = -3, psi0 = 3 precision=%d" % precision)
    assert ei == pytest.approx(k * (2.0 * np.pi - 6.0) ** 2, rel=1e-10) and np.abs(f).max() > 1.0
    g.close()


@pytest.mark.parametrize("precision", [1, 0])
def test_one_urey_bradley_term_at_known_distances(Engine, precision):
    r0, k = 0.2179, 2.5e4
    u = np.array([0.6, -0.48, 0.64])          # (a unit vector)
    s = cc.bare(np.array([[0.1, 0.2, 0.3], [0.17, 0.31, 0.26], [0.1, 0.2, 0.3] + r0 * u]), ub=([[0, 2]], [[r0, k]]))
    g = Engine(s, _integ().to_data(precision=precision))
    for scale in (1.0, 0.9, 1.1):
        x = s.positions.copy(); x[2] = x[0] + scale * r0 * u
        assert abs(np.linalg.norm(x[2] - x[0]) - scale * r0) <= 1e-12
        eu, ei, f = _check_against_reference(g, None, s, x, "r = %.1f r0 precision=%d" % (scale, precision))
        assert eu == pytest.approx(0.5 * k * ((scale - 1.0) * r0) ** 2, rel=1e-9, abs=1e-20) and ei == 0.0
        assert np.all(f[1] == 0.0) and (scale == 1.0 or np.abs(f).max() > 100.0)
    g.close()


# ---- 7. real topologies
def _toluene_box_with_terms(tol_box, straddle):
    s, a = cc.with_ring_terms(systems.with_reciprocal_space(tol_box[0]))
    x = np.array(s.positions, dtype=np.float64)
    box = _box(s)
    if straddle:      # everything translated so that an atom of the terms sits on the box face, every atom wrapped into the box by itself
        x = x - x[a[2]] + np.array([0.0, 0.3, 0.4]) * box
        x = x - box * np.floor(x / box)
        assert len(set(np.round((x[a] - x[a[2]]) / box)[:, 0])) > 1          # (the terms' atoms lie on both sides of the face)
    return s, x


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("case", ["chamber vacDivaline", "toluene box", "toluene box, across a face"])
def test_real_topologies(Engine, tol_box, tune, case, precision):
    """Mixed precision: everything that is not one of the terms is computed by the same kernels from the same numbers in both engines
    (the decomposition pinned to be the same: an engine with the terms never takes the fused force launch), the bonded entries are
    fp64 in both -- the same subtraction, the same bar."""
    tune(fuse_forces=0)
    if case == "chamber vacDivaline":
        s = cc.chamber_divaline()
        x = s.positions
    else:
        s, x = _toluene_box_with_terms(tol_box, case.endswith("face"))
    data = _integ().to_data(precision=precision)
    g, gp = Engine(s, data), Engine(cc.without(s), data)
    for ls, le in ((1.0, 1.0), (0.4, 0.2)):       # (not alchemical: the same part at any lambda)
        for e in (g, gp):
            e.set_global("lambda_sterics", ls); e.set_global("lambda_electrostatics", le)
        eu, ei, _ = _check_against_reference(g, gp, s, x, "%s precision=%d lambda=(%.1f, %.1f)" % (case, precision, ls, le))
        assert eu > 0.0 and ei > 0.0
    g.close(); gp.close()


@pytest.mark.parametrize("precision", [1, 0])
def test_exceptions_of_the_chamber_system(Engine, precision):
    """Energy term [4] is the 1-4 sum over exception_params, which come from the topology's own table (no alchemical atom: every
    exception is booked there)."""
    s = dataclasses.replace(cc.chamber_divaline(), alchemical_atoms=np.zeros(0, np.int32))
    a = dataclasses.replace(cc.amber_divaline(), alchemical_atoms=np.zeros(0, np.int32))
    e_ref, _ = ref.exceptions(s.exception_atoms, s.exception_params, s.positions)
    e_amber, _ = ref.exceptions(a.exception_atoms, a.exception_params, a.positions)
    g = Engine(s, _integ().to_data(precision=precision))
    t = g.energy_terms()
    print("CHARMM 1-4 sum precision=%d: engine %.12g, reference %.12g (d %.2e); from the diagonal entries it would be %.12g" % (precision, t[4], e_ref, abs(t[4] - e_ref), e_amber))
    assert abs(t[4] - e_ref) <= 1e-12 * max(1.0, abs(e_ref))
    assert abs(e_ref - e_amber) > 1.0
    g.close()


# ---- 8. forces are the gradient of the engine's own energy
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
    """Central differences of potential_energy() (h = 1e-5 nm) against get_forces() on the atoms of the impropers of the chamber
    vacDivaline (no constraints: every bond harmonic), with the terms and -- the bar -- on the same System without them: at most twice
    that disagreement plus 1e-9 of the largest force (the stiff bonds' own finite-difference error dominates both).  Measured:
    2.274e-4 kJ/mol/nm with the terms (largest force 4114), 1.265e-4 without (3608); the terms' own force up to 2750."""
    s = cc.chamber_divaline(constraints=None)
    x = s.positions + np.random.default_rng(3).normal(size=s.positions.shape) * 0.002
    atoms = sorted(set(int(a) for a in np.asarray(s.improper_atoms).reshape(-1)))
    data = _integ().to_data(precision=1)
    g, gp = Engine(s, data), Engine(cc.without(s), data)
    d_with, big_with = _fd_disagreement(g, x, atoms)
    d_plain, big_plain = _fd_disagreement(gp, x, atoms)
    _, _, f_ref = ref.energy_forces(s, x)
    print("CHARMM finite differences: with the terms %.3e kJ/mol/nm (largest force %.4g), without %.3e (largest force %.4g); the terms' force up to %.4g"
          % (d_with, big_with, d_plain, big_plain, np.abs(f_ref).max()))
    assert np.abs(f_ref).max() > 10.0
    assert d_with <= 2.0 * d_plain + 1e-9 * big_with, (d_with, d_plain)
    g.close(); gp.close()


# ---- 9. frozen atoms
def _six_atoms():
    rng = np.random.default_rng(23)
    x = np.cumsum(rng.normal(size=(6, 3)) * 0.05 + np.array([0.12, 0.0, 0.0]), axis=0)
    return cc.bare(x, ub=([[0, 2], [3, 5]], [[0.2, 2.0e4], [0.3, 1.0e4]]), impr=([[0, 1, 2, 3], [2, 3, 4, 5]], [[0.2, 90.0], [-0.4, 60.0]]))


@pytest.mark.parametrize("frozen", [[0, 1, 2, 3], [0, 2, 3, 4, 5]])
def test_frozen_atoms_of_the_terms(Engine, frozen):
    """[0, 1, 2, 3]: the first improper and the first Urey-Bradley term have no mobile atom -- no entries, but their energy; the
    others' forces are the reference's rows.  [0, 2, 3, 4, 5]: one atom of the first improper is mobile."""
    s = _six_atoms()
    sf = systems.freeze_atoms(s, frozen)
    data = _integ().to_data(precision=1)
    g, g0 = Engine(sf, data), Engine(s, data)
    eu, ei, f_ref = _check_against_reference(g, None, sf, s.positions, "frozen %s" % (frozen,))
    g0.set_positions(s.positions)
    assert g.energy_terms()[0] == g0.energy_terms()[0] and g.energy_terms()[2] == g0.energy_terms()[2]      # the energy does not know who is frozen
    f, f0 = g.get_forces(), g0.get_forces()
    free = [a for a in range(6) if a not in frozen]
    assert np.all(f[frozen] == 0.0) and np.abs(f_ref[frozen]).min() > 0.0
    assert np.array_equal(f[free], f0[free])            # the forces of the others are unchanged
    g.close(); g0.close()


# ---- 10. dynamics
def _mostly_frozen_box(tol_box):
    s, v = tol_box
    lig = np.arange(15)
    near = systems.nearest_molecules(s, lig, 120, exclude_idx=lig)
    sf = systems.freeze_except(s, np.concatenate([lig, near]))
    sf, _ = cc.with_ring_terms(sf)      # (on the ligand: mobile)
    return sf, v * (sf.mass[:, None] > 0)


def _dynamics_system(tol_box, kind):
    if kind == "chamber vacDivaline":
        return cc.chamber_divaline(), None, 3
    return _mostly_frozen_box(tol_box) + (2,)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("kind", ["chamber vacDivaline", "mostly frozen toluene box"])
def test_batch_member_equals_the_lone_chain(Engine, tol_box, tune, kind, precision):
    """20 steps of the default switch: every member of a NativeBatch equals the same chain alone bit for bit, the switch with the
    terms is not the switch without them, and a batch refuses members whose improper lists differ."""
    from blues_amd.engine import EngineError, NativeBatch
    s, v, R = _dynamics_system(tol_box, kind)
    n = 20
    tune(assume_batch=R)

    def make(system, count=R):
        out = []
        for r in range(count):
            g = Engine(system, _integ(nsteps=n, seed=40 + r).to_data(precision=precision, replica=r))
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
    plain = make(cc.without(s), 1)[0]
    plain.step(n)
    assert not np.array_equal(plain.get_positions(), solo[0].get_positions())
    q = s.improper_params.copy(); q[0, 1] *= 1.25
    other = dataclasses.replace(s, improper_params=q)
    with pytest.raises(EngineError, match="impropers"):
        NativeBatch(make(s, 1) + make(other, 2)[1:]).step(1)
    with pytest.raises(EngineError, match="Urey-Bradley"):
        NativeBatch(make(s, 1) + make(dataclasses.replace(s, urey_bradley_atoms=s.urey_bradley_atoms[:-1], urey_bradley_params=s.urey_bradley_params[:-1]), 2)[1:]).step(1)
    B.close()


# ---- 11. the ledger, the minimiser
@pytest.mark.parametrize("kind", ["chamber vacDivaline", "mostly frozen toluene box"])
def test_ledger_closes_with_the_terms(Engine, tol_box, kind):
    """Double precision, measure_shadow_work = measure_heat = 1: dE = dW + shadow + heat after every step to the bar of
    tests/test_gpu_energy_ledger.py (1e-9 max(1, |W|)): the energy form and the force form see the same terms in every path."""
    s, v, _ = _dynamics_system(tol_box, kind)
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
    print("CHARMM ledger %s: largest residual %.3e kJ/mol over 20 steps, largest |shadow work| %.3e" % (kind, worst, big))
    assert big > 0.0
    g.close()


def test_minimize_unbends_an_improper(Engine):
    """four bonded atoms whose improper (psi0 = 0) starts bent by 0.5 rad"""
    x = ref.four_atoms(0.5)
    s = cc.bare(x, impr=([[0, 1, 2, 3]], [[0.0, 200.0]]), ub=([[0, 2]], [[np.linalg.norm(x[0] - x[2]), 1.0e4]]))
    pairs = np.array([[0, 1], [1, 2], [2, 3]], np.int32)
    s = dataclasses.replace(s, bond_atoms=pairs, bond_params=np.stack([np.full(3, 0.15), np.full(3, 2.0e5)], axis=1))
    g = Engine(s, _integ().to_data(precision=1))
    e0 = g.potential_energy()
    assert e0 == pytest.approx(200.0 * 0.25, rel=1e-9)
    out = g.minimize(tolerance=1.0, max_iterations=5000)
    print("CHARMM minimise: %s" % (out,))
    assert out["e_final"] < out["e_initial"] and out["e_final"] < 0.1 * e0
    pe = g.potential_energy()
    print("CHARMM minimise: potential_energy() %.17g, e_final %.17g, relative difference %.3e" % (pe, out["e_final"], abs(pe - out["e_final"]) / abs(out["e_final"])))
    assert abs(pe - out["e_final"]) <= 1e-9 * abs(out["e_final"])
    assert abs(ref.improper_angles(s.improper_atoms, g.get_positions())[0]) < 0.1
    g.close()


# ---- 12. permutation
def test_permuted_atoms(Engine):
    s = cc.chamber_divaline()
    perm = sym.scatter_perm(s.n_atoms, 12)
    sp, _, m = sym.permute_atoms(s, None, perm)
    new_of_old = np.empty(s.n_atoms, np.int64); new_of_old[perm] = np.arange(s.n_atoms)
    sp = dataclasses.replace(sp, urey_bradley_atoms=new_of_old[s.urey_bradley_atoms].astype(np.int32), improper_atoms=new_of_old[s.improper_atoms].astype(np.int32))
    data = _integ().to_data(precision=1)
    g, h = Engine(s, data), Engine(sp, data)
    ta, tb = g.energy_terms(), h.energy_terms()
    for k in range(_abi.N_ENERGY_TERMS):
        assert abs(ta[k] - tb[k]) <= 1e-12 * max(1.0, abs(ta[k])), (k, ta[k], tb[k])
    fa, fb = g.get_forces(), m.vectors(h.get_forces())
    assert np.abs(fa - fb).max() <= 1e-12 * np.abs(fa).max()
    eu, ei, _ = ref.energy_forces(sp, sp.positions)
    gp = Engine(cc.without(sp), data)
    assert abs(tb[2] - gp.energy_terms()[2] - ei) <= 1e-12 * max(1.0, ei) and abs(tb[0] - gp.energy_terms()[0] - eu) <= 1e-12 * max(1.0, eu)
    for e in (g, h, gp):
        e.close()


# ---- 13. what the library refuses (the wrapper's own check switched off: the descriptor reaches the C-ABI as a foreign caller's would)
@pytest.mark.parametrize("case", sorted(cc.bad_systems()))
def test_creation_errors_of_the_library(Engine, monkeypatch, case):
    from blues_amd.engine import EngineError
    match, s = cc.bad_systems()[case]
    with pytest.raises(EngineError, match=match):      # the wrapper's own refusal
        Engine(s, _integ().to_data(precision=0))
    monkeypatch.setattr(_abi.SystemData, "check_charmm", lambda self: None)
    with pytest.raises(EngineError, match=match):      # the library's
        Engine(s, _integ().to_data(precision=0))


def _raw_create(lib, s, ext):
    sd, keep_s = s.to_desc(); idesc, keep_i = _integ().to_data(precision=0).to_desc()
    h = ctypes.c_void_p()
    rc = lib.blues_engine_create_ext(ctypes.byref(sd), ctypes.byref(idesc), None, ctypes.byref(ext), 0, ctypes.byref(h))
    return rc, lib.blues_last_error(None).decode(), h


def test_counts_without_arrays_are_refused(Engine):
    from blues_amd import _lib
    lib = _lib.load()
    s = cc.chamber_divaline()
    for field in ("urey_bradley_atoms", "urey_bradley_params", "improper_atoms", "improper_params"):
        ext = s.ext_desc()
        setattr(ext, field, ctypes.cast(None, type(getattr(ext, field))))
        rc, msg, _ = _raw_create(lib, s, ext)
        assert rc != 0 and "without their arrays" in msg, (field, msg)
    ext = s.ext_desc(); ext.n_impropers = -1
    rc, msg, _ = _raw_create(lib, s, ext)
    assert rc != 0 and "-1 impropers" in msg


def test_struct_sizes_the_library_accepts(Engine):
    """struct_size 8 (nothing past the treatment is read), BLUES_SYSTEM_EXT_SIZE_V2 (BluesSystemExt, a caller without these terms: its maps are
    still honoured, the terms are not read) and BluesSystemExtV3's; anything else is refused by name."""
    import cmap_cases
    from blues_amd import _lib
    lib = _lib.load()
    s = cmap_cases.divaline([cmap_cases.surface_map(8)])
    c = cc.chamber_divaline()
    s = dataclasses.replace(s, urey_bradley_atoms=c.urey_bradley_atoms, urey_bradley_params=c.urey_bradley_params, improper_atoms=c.improper_atoms, improper_params=c.improper_params)
    x = np.ascontiguousarray(s.positions, dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)

    def create(size):
        ext = s.ext_desc(); ext.struct_size = size
        rc, msg, h = _raw_create(lib, s, ext)
        ang, terms = np.full(2, -1.0), np.zeros(_abi.N_ENERGY_TERMS)
        if rc == 0:
            assert lib.blues_set_positions(h, x.ctypes.data_as(dp), s.n_atoms) == 0
            assert lib.blues_get_cmap_angles(h, ang.ctypes.data_as(dp)) == 0
            assert lib.blues_get_energy_terms(h, terms.ctypes.data_as(dp)) == 0
            lib.blues_engine_destroy(h)
        return rc, msg, ang, terms
    eu, ei, _ = ref.energy_forces(s, x)
    rc, _, ang, full = create(ctypes.sizeof(_abi.BluesSystemExtV3))
    assert rc == 0 and np.all(ang >= 0.0)
    rc, _, ang, v2 = create(_abi.SYSTEM_EXT_SIZE_V2)
    assert rc == 0 and np.all(ang >= 0.0)              # the maps of a V2 caller are read ...
    assert abs(full[0] - v2[0] - eu) <= 1e-12 * max(1.0, eu) and abs(full[2] - v2[2] - ei) <= 1e-12 * max(1.0, ei) and eu > 0.0 and ei > 0.0      # ... the terms are not
    rc, _, ang, v1 = create(_abi.SYSTEM_EXT_SIZE_V1)
    assert rc == 0 and np.all(ang == -1.0) and v1[0] == v2[0] and v1[2] != v2[2]
    for size in (4, 12, ctypes.sizeof(_abi.BluesSystemExt) + 8, ctypes.sizeof(_abi.BluesSystemExtV3) + 8):
        rc, msg, _, _ = create(size)
        assert rc != 0 and "struct_size" in msg
