"""GPU suite: the reciprocal-space kernels (blues_amd/csrc/kernels_pme.h) over mesh shapes, block wraps and fallbacks -- the rows of
tests/pme_cases.py on the 975-atom toluene box against the fp64 oracle on the same SystemData, with the path each mixed-precision launch
took read from the counter the kernel keeps (stats()["pme_fast_launches"] / ["pme_general_launches"]).  Tolerances are
tests/test_gpu_pme.py's: 1e-10 (double) / 1e-5 (mixed) of max(|term|, 1) for energies and of the largest force component for forces.
Every comparison prints its residual (profiles/pme_shapes/README.md keeps a run's table)."""
import copy

import numpy as np
import pytest

import exact_pme_reference as xref
import pme_cases as pc
from blues_amd import integrators, systems

pytestmark = pytest.mark.gpu

TOL = {1: 1e-10, 0: 1e-5}
LAMBDAS = ((1.0, 1.0), (0.5, 0.3))
EXACT_LAMBDAS = ((1.0, 1.0), (0.5, 0.3), (0.0, 0.0), (0.2, 0.7))      # tests/test_gpu_exact_pme.py: LAMBDAS


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _integ(n=20, seed=7, dt=0.004):
    return integrators.generateNCMCIntegrator(nstepsNC=n, dt=dt, temperature=300.0, seed=seed)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


_expect = {}


def _reference(oracle_mod, key, system, lambdas=LAMBDAS, positions=None, box=None):
    """{(ls, le): (E, F, terms)} of the oracle on `system`: evaluated once per key, shared by both precisions, never changed"""
    if key not in _expect:
        o = oracle_mod.Oracle(system, _integ().to_data(precision=1), openmp=True)
        if box is not None:
            o.set_box(box)
        if positions is not None:
            o.set_positions(positions)
        _expect[key] = {lam: o.energy_forces(*lam) for lam in lambdas}
    return _expect[key]


def _counts(g):
    st = g.stats()
    return np.array([st["pme_fast_launches"], st["pme_general_launches"]])


def _parity(g, expect, precision, mob, label, nontrivial=True):
    """energy_terms() (all ten), potential_energy() and the forces on the mobile atoms against the oracle, at every lambda of `expect`"""
    tol = TOL[precision]
    for (ls, le), (eo, fo, to) in expect.items():
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        tg = g.energy_terms()
        f = g.get_forces()
        res_t = max(abs(tg[k] - to[k]) / max(abs(to[k]), 1.0) for k in range(10))
        print("RESIDUAL %s precision=%d lambda=(%g,%g) terms %.3e total %.3e forces %.3e" % (label, precision, ls, le, res_t, abs(tg.sum() - eo) / abs(eo), _rel(f[mob], fo[mob])))
        if nontrivial:
            assert abs(to[8]) > 100.0 and abs(to[9]) > 10.0
        for k in range(10):
            assert abs(tg[k] - to[k]) <= tol * max(abs(to[k]), 1.0), (label, k, tg[k], to[k])
        assert abs(tg.sum() - eo) <= tol * abs(eo)
        assert g.potential_energy() == pytest.approx(tg.sum(), rel=1e-14)
        assert _rel(f[mob], fo[mob]) <= tol, label


def _assert_counter(before, after, precision, path, label):
    """mixed precision: exactly the expected word moved; double precision: the pruned pipeline never ran"""
    d = after - before
    print("PATH %s precision=%d model=%s fast+%d general+%d" % (label, precision, path, d[0], d[1]))
    if precision == 1:
        assert after[0] == 0 and d[1] > 0, (label, d)
    elif path == "fast":
        assert d[0] > 0 and d[1] == 0, (label, path, d)
    else:
        assert d[1] > 0 and d[0] == 0, (label, path, d)


# ---- a. static parity over the table
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_parity_over_the_table(Engine, oracle_mod, case, precision):
    s = pc.build(case)
    path, L = pc.expected_path(s)
    assert path == case.kind
    expect = _reference(oracle_mod, case.id, s)
    g = Engine(s, _integ().to_data(precision=precision))
    c0 = _counts(g)
    _parity(g, expect, precision, s.mass != 0.0, "%s block=%s" % (case.id, "x".join(map(str, L))))
    _assert_counter(c0, _counts(g), precision, path, case.id)
    g.close()


# ---- b. the in-kernel fallback equals a dedicated general launch
@pytest.mark.parametrize("case", [c for c in pc.CASES if c.kind in ("general:atoms", "general:block")], ids=lambda c: c.id)
def test_fallback_equals_a_dedicated_general_launch(Engine, oracle_mod, tune, case):
    """k_pme_fast's two exits run pme_body<float, false, 5>, the body of k_pme<float, false>: the same template at the same order, so the
    results are required to be the same bits (measured so: profiles/pme_shapes/README.md), beyond the 1e-6 of the largest force asked for.
    The counter cannot tell an in-kernel exit from a general kernel the host chose: both add to word 1.  That the first engine starts
    k_pme_fast rests on the host's gate (asserted here: the mesh passes it) and on the default tuning, under which the engine is made AND
    evaluated before the second one pins pme_general = 1."""
    s = pc.build(case)
    expect = _reference(oracle_mod, case.id, s)
    mob = s.mass != 0.0
    from blues_amd import tuning
    K = s.pme_grid
    assert K[0] * K[1] * (K[2] // 2 + 1) <= pc.LDS_Y and tuning.current().pme_general == 0
    g1 = Engine(s, _integ().to_data(precision=0))
    c1 = _counts(g1)
    _parity(g1, expect, 0, mob, case.id + " fallback")
    _assert_counter(c1, _counts(g1), 0, case.kind, case.id + " fallback")
    f1, t1 = g1.get_forces(), g1.energy_terms()
    g1.close()
    tune(pme_general=1)
    g2 = Engine(s, _integ().to_data(precision=0))
    c2 = _counts(g2)
    _parity(g2, expect, 0, mob, case.id + " dedicated")
    _assert_counter(c2, _counts(g2), 0, "general:host", case.id + " dedicated")
    f2, t2 = g2.get_forces(), g2.energy_terms()
    print("FALLBACK %s forces differ by %.3e of the largest, bit-equal forces: %s, bit-equal terms: %s" % (case.id, _rel(f1[mob], f2[mob]), np.array_equal(f1, f2), np.array_equal(t1, t2)))
    assert _rel(f1[mob], f2[mob]) <= 1e-6
    assert np.array_equal(f1, f2) and np.array_equal(t1, t2)
    g2.close()


# ---- c. atoms exactly on mesh planes and on the box edge, and one ulp to either side
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("ulps", [0, 1, -1])
@pytest.mark.parametrize("name", ["20x18x27-45-corner", "18x20x32-45-corner"])
def test_atoms_on_mesh_planes_and_the_box_edge(Engine, oracle_mod, name, ulps, precision):
    s, planted = pc.on_planes(pc.build(pc.BY_ID[name]), ulps)
    path, L = pc.expected_path(s)
    expect = _reference(oracle_mod, (name, "planes", ulps), s)
    g = Engine(s, _integ().to_data(precision=precision))
    c0 = _counts(g)
    _parity(g, expect, precision, s.mass != 0.0, "%s on_planes(%+d)" % (name, ulps))
    _assert_counter(c0, _counts(g), precision, path, name)
    g.close()


# ---- d. no charged mobile atom (the empty block), and the qn_full launch of the same engine
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("n_mobile", [15, 45])
def test_no_charged_mobile_atom_and_the_full_charge_launch(Engine, oracle_mod, n_mobile, precision):
    s = pc.mobile_nearest(pc.build(pc.BY_ID["20x18x27-45"]), n_mobile)
    direct = pc.mobile_nearest(systems.toluene_box()[0], n_mobile)      # the same box without reciprocal space
    assert np.array_equal(direct.mass, s.mass) and np.array_equal(direct.positions, s.positions)
    plain = copy.copy(s); plain.alchemical_atoms = np.zeros(0, np.int32)
    mob, tol = s.mass != 0.0, TOL[precision]
    path, L = pc.expected_path(s)
    assert path == "fast" and (L == (1, 1, 1)) == (n_mobile == 15)
    expect = _reference(oracle_mod, ("lig", n_mobile), s)
    data = _integ().to_data(precision=precision)
    g, gd = Engine(s, data), Engine(direct, data)
    c0 = _counts(g)
    _parity(g, expect, precision, mob, "20x18x27-%d block=%s" % (n_mobile, "x".join(map(str, L))))
    c1 = _counts(g)
    _assert_counter(c0, c1, precision, path, "20x18x27-%d" % n_mobile)
    # the ligand's charges are 0 in the NonbondedForce ('direct-space' treatment): reciprocal space adds exactly nothing to its forces
    for e in (g, gd):
        e.set_global("lambda_sterics", 0.5); e.set_global("lambda_electrostatics", 0.3)
    f_rec = g.get_forces() - gd.get_forces()
    print("reciprocal forces: ligand max |f| %.3e, mobile water max |f| %.3e" % (np.abs(f_rec[:pc.N_LIG]).max(), np.abs(f_rec[mob][pc.N_LIG:]).max() if n_mobile > pc.N_LIG else 0.0))
    assert np.all(f_rec[:pc.N_LIG] == 0.0)
    if n_mobile > pc.N_LIG:
        assert np.abs(f_rec[mob][pc.N_LIG:]).max() > 10.0
    # the mesh energy without and with the alchemical charges (want_energy & 2: the block of the same engine is another one)
    o, op = oracle_mod.Oracle(s, data, openmp=True), oracle_mod.Oracle(plain, data, openmp=True)
    e0, e1 = pc.mesh_energy_of(s, o), pc.mesh_energy_of(plain, op)
    path_full, L_full = pc.expected_path(s, full_charges=True)
    assert path_full == "fast" and pc.block_class(s, L_full) == "partial" and (L_full != L or n_mobile > pc.N_LIG)
    m1 = g.mesh_energy(True); c2 = _counts(g)
    m0 = g.mesh_energy(False); c3 = _counts(g)
    print("RESIDUAL mesh_energy n_mobile=%d precision=%d: without alchemical charges %.3e, with %.3e (blocks %s / %s)" % (n_mobile, precision, abs(m0 - e0) / max(abs(e0), 1.0), abs(m1 - e1) / max(abs(e1), 1.0), L, L_full))
    assert abs(e1 - e0) > 0.01
    assert abs(m0 - e0) <= tol * max(abs(e0), 1.0) and abs(m1 - e1) <= tol * max(abs(e1), 1.0)
    _assert_counter(c1, c2, precision, path_full, "mesh_energy(True)")
    _assert_counter(c2, c3, precision, path, "mesh_energy(False)")
    # and the launch after it sees the engine's own block again
    _parity(g, expect, precision, mob, "20x18x27-%d after mesh_energy" % n_mobile)
    g.close(); gd.close()


# ---- e. have_static == 0 on the fast path
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("name", ["20x18x27-45", "9x9x9-150"])
def test_uncharged_frozen_atoms_no_static_meshes(Engine, oracle_mod, name, precision):
    charged = pc.build(pc.BY_ID[name])
    s = pc.uncharged_frozen(charged)
    path, L = pc.expected_path(s)
    expect = _reference(oracle_mod, (name, "uncharged"), s)
    data = _integ().to_data(precision=precision)
    launches = []
    for system in (s, charged):      # the same calls on both: the charged box has one launch more, once -- its static meshes
        g = Engine(system, data)
        k0 = g.stats()["kernel_launches"]; g.energy_terms(); k1 = g.stats()["kernel_launches"]
        g.set_positions(system.positions); g.energy_terms(); k2 = g.stats()["kernel_launches"]
        launches.append(((k1 - k0) - (k2 - k1), k1 - k0, k2 - k1))
        if system is s:
            c0 = _counts(g)
            _parity(g, expect, precision, s.mass != 0.0, name + " uncharged frozen", nontrivial=False)
            _assert_counter(c0, _counts(g), precision, path, name)
            assert abs(expect[(1.0, 1.0)][2][8]) > 1.0      # (the mobile water's self term and its excluded-pair corrections nearly cancel)
        g.close()
    print("kernel launches (first - second evaluation, first, second): uncharged frozen %s, charged %s" % (launches[0], launches[1]))
    assert launches[1][0] - launches[0][0] == 1 and launches[1][2] == launches[0][2]


# ---- f. a switch on the fast path
@pytest.mark.parametrize("precision,tol", [(1, 1e-9), (0, 1e-5)])
def test_switch_on_the_fast_path_across_the_box_edge(Engine, oracle_mod, precision, tol):
    s = pc.build(pc.BY_ID["24x24x30-45-corner"])
    v = np.array(pc.base()[1], dtype=np.float64); v[s.mass == 0.0] = 0.0
    n = 20
    data = _integ(n, dt=0.002).to_data(precision=precision)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data, openmp=True)
    g.set_velocities(v); o.set_velocities(v)
    c0 = _counts(g)
    wg = g.run_switch(n, trace=True)
    c1 = _counts(g)
    wo = []
    for _ in range(n):
        o.step(1); wo.append(o.get_global("protocol_work"))
    wo = np.array(wo)
    xg, xo = g.get_positions(), o.get_positions()
    print("RESIDUAL switch precision=%d work %.3e positions %.3e nm; launches fast+%d general+%d" % (precision, np.abs(wg - wo).max() / np.abs(wo).max(), np.abs(xg - xo).max(), c1[0] - c0[0], c1[1] - c0[1]))
    assert np.abs(wg - wo).max() <= tol * np.abs(wo).max()
    assert np.abs(xg - xo).max() < (1e-9 if precision else 2e-4)
    if precision == 0:
        assert c1[0] - c0[0] >= n and c1[1] == c0[1]
    else:
        assert c1[1] - c0[1] >= n and c1[0] == 0
    # the mobile atoms sit around the box corner: some cross a mesh plane during the switch, the block is derived anew every launch
    mob = s.mass != 0.0
    t0, t1 = pc.mesh_index(s.positions[mob], s.box, s.pme_grid)[0], pc.mesh_index(xo[mob], s.box, s.pme_grid)[0]
    assert (t0 != t1).any()
    assert pc.expected_path(s, xo)[0] == "fast" and all(pc.wraps(s, xo))
    g.close()


# ---- g. set_box on a PME engine
@pytest.mark.parametrize("precision", [1, 0])
def test_set_box_rebuilds_the_mesh_tables(Engine, oracle_mod, precision):
    s = pc.build(pc.BY_ID["20x18x27-45"])
    mob = s.mass != 0.0
    box, x = pc.scaled_box(s, (1.01, 0.99, 1.003))
    first = _reference(oracle_mod, "20x18x27-45", s)
    scaled = _reference(oracle_mod, ("20x18x27-45", "scaled"), s, positions=x, box=box)
    assert abs(scaled[(1.0, 1.0)][2][8] - first[(1.0, 1.0)][2][8]) > 0.1      # (the reference itself moves with the box: 0.44 kJ/mol in term 8)
    g = Engine(s, _integ().to_data(precision=precision))
    _parity(g, first, precision, mob, "20x18x27-45 before set_box")
    g.set_global("lambda_sterics", 1.0); g.set_global("lambda_electrostatics", 1.0)
    e_first = g.potential_energy()
    g.set_box(box); g.set_positions(x)
    c0 = _counts(g)
    _parity(g, scaled, precision, mob, "20x18x27-45 box x (1.01, 0.99, 1.003)")
    _assert_counter(c0, _counts(g), precision, pc.expected_path(s)[0], "after set_box")
    # (positions first: set_box sorts and tiles the atoms where it finds them, and the order of the fp64 sums follows that sort)
    g.set_positions(s.positions); g.set_box(np.asarray(s.box, dtype=np.float64))
    g.set_global("lambda_sterics", 1.0); g.set_global("lambda_electrostatics", 1.0)
    assert g.potential_energy() == e_first      # (bit-equal: the tables, the static meshes and the box constants are the first ones again)
    _parity(g, first, precision, mob, "20x18x27-45 box set back")
    g.close()


# ---- h. one launch, different exits
@pytest.mark.parametrize("inactive", [None, 2])
def test_batch_whose_members_take_different_exits(Engine, oracle_mod, tune, inactive):
    from blues_amd.engine import NativeBatch
    s = pc.build(pc.BY_ID["24x24x30-45"])
    v = np.array(pc.base()[1], dtype=np.float64); v[s.mass == 0.0] = 0.0
    x_apart = pc.scattered(s)
    paths = ["fast", "general:block", "fast", "general:block"]
    assert pc.expected_path(s)[0] == "fast" and pc.expected_path(s, x_apart)[0] == "general:block"
    R, n = 4, 12
    tune(assume_batch=8)
    mob = s.mass != 0.0

    def make():
        out = []
        for q in range(R):
            e = Engine(s, _integ(n, seed=40 + q).to_data(precision=0, replica=q))
            if paths[q] != "fast":
                e.set_positions(x_apart)
            e.set_velocities(v * (1 + 0.02 * q)); out.append(e)
        return out
    for q in (0, 1):      # each kind's first evaluation against the oracle (members 2 and 3 start from the same positions)
        probe = make()[q]
        expect = _reference(oracle_mod, "24x24x30-45" if paths[q] == "fast" else ("24x24x30-45", "apart"), s, positions=None if paths[q] == "fast" else x_apart)
        c = _counts(probe)
        _parity(probe, expect, 0, mob, "batch member %d (%s)" % (q, paths[q]))
        _assert_counter(c, _counts(probe), 0, paths[q], "batch member %d alone" % q)
    solo = make()
    ws = [e.run_switch(n, trace=True) for e in solo]
    bat = make(); B = NativeBatch(bat)
    c0 = [_counts(e) for e in bat]
    x0 = [e.get_positions() for e in bat]
    active = None if inactive is None else [q != inactive for q in range(R)]
    _, wb = B.step(n, trace=True, active=active)
    for q in range(R):
        d = _counts(bat[q]) - c0[q]
        print("PATH batch member %d model=%s fast+%d general+%d%s" % (q, paths[q], d[0], d[1], " (inactive)" if q == inactive else ""))
        if q == inactive:
            assert d[0] == 0 and d[1] == 0 and np.array_equal(bat[q].get_positions(), x0[q])
            continue
        assert np.array_equal(wb[q], ws[q]) and np.array_equal(solo[q].get_positions(), bat[q].get_positions())
        assert bat[q].potential_energy() == solo[q].potential_energy()
        if paths[q] == "fast":
            assert d[0] >= n and d[1] == 0
        else:
            assert d[1] >= n and d[0] == 0
        assert pc.expected_path(s, bat[q].get_positions())[0] == paths[q]      # (and the member stayed on it to the end)
    B.close()
    for e in solo + bat:
        e.close()


# ---- i. the exact treatment on partial, wrapped blocks
def _exact_compare(g, expect, tol, mob, label):
    """tests/test_gpu_exact_pme.py::_compare"""
    eo, fo, to = expect
    tg = g.energy_terms()
    gg, go = xref.group_terms(tg), xref.group_terms(to)
    f = g.get_forces()
    print("RESIDUAL exact %s groups %.3e forces %.3e" % (label, max(abs(gg[k] - go[k]) / max(abs(go[k]), 1.0) for k in range(len(go))), _rel(f[mob], fo[mob])))
    for k in range(len(go)):
        assert abs(gg[k] - go[k]) <= tol * max(abs(go[k]), 1.0), (label, k, gg[k], go[k])
    assert abs(tg.sum() - eo) <= tol * abs(eo)
    assert g.potential_energy() == pytest.approx(tg.sum(), rel=1e-14)
    assert _rel(f[mob], fo[mob]) <= tol, label


_exact_expect = {}


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("name", [m + "-" + sh for m in ("20x18x27-45", "18x20x32-45", "24x24x30-45", "24x24x30-150") for sh in ("corner", "centre")])
def test_exact_treatment_on_partial_wrapped_blocks(Engine, name, precision):
    row, sh = name.rsplit("-", 1)
    s = systems.with_alchemical_pme_treatment(pc.shift(pc.build(pc.BY_ID[row]), sh), "exact")
    mob = s.mass != 0.0
    if name not in _exact_expect:
        ref = xref.ExactPmeReference(s, openmp=True)
        _exact_expect[name] = {lam: ref.evaluate(s.positions, *lam) for lam in EXACT_LAMBDAS}
    g = Engine(s, _integ().to_data(precision=precision))
    for lam in EXACT_LAMBDAS:
        g.set_global("lambda_sterics", lam[0]); g.set_global("lambda_electrostatics", lam[1])
        _exact_compare(g, _exact_expect[name][lam], TOL[precision], mob, "%s precision=%d lambda=(%g,%g)" % (name, precision, lam[0], lam[1]))
    st = g.stats()
    fast = precision == 0 and row.endswith("-45")
    print("PATH exact %s precision=%d fast %d general %d; block of all charged mobile atoms %s" % (name, precision, st["exact_pme_fast_launches"], st["exact_pme_general_launches"], pc.expected_path(s, full_charges=True)[1]))
    if fast:      # tests/test_gpu_exact_pme.py::_assert_path
        assert st["exact_pme_fast_launches"] > 0 and st["exact_pme_general_launches"] == 0
        assert pc.block_class(s, pc.expected_path(s, full_charges=True)[1]) == "partial"
    else:
        assert st["exact_pme_general_launches"] > 0 and st["exact_pme_fast_launches"] == 0
    g.close()


# ---- j. long axes
# (8, 8, 256) and (256, 8, 8) leave the pruned pipeline -- 8 x 8 x 129 lines do not fit its X buffer, 256 x 8 x 5 fail the host's gate -- so
# two narrower meshes bring the longest axis the engine accepts onto it: 129 inputs per z line, 256 per x line
LONG_MESHES = ((8, 8, 64), (8, 8, 128), (8, 8, 256), (64, 8, 8), (128, 8, 8), (256, 8, 8), (6, 8, 256), (256, 6, 8))


@pytest.mark.parametrize("n_mobile", [45, 150])
@pytest.mark.parametrize("mesh", LONG_MESHES, ids=lambda m: "%dx%dx%d" % m)
def test_long_axes_in_mixed_precision(Engine, oracle_mod, tune, mesh, n_mobile):
    """The pruned passes advance their phase by one fp32 rotation per input, up to K inputs along an axis of K points (the engine accepts
    K <= 256).  Condition: the project's 1e-5 on the fast path wherever the model says a launch takes it, and on the general kernel on the
    same case."""
    s = copy.copy(pc.build(pc.BY_ID["9x9x9-150"] if n_mobile == 150 else pc.BY_ID["20x18x27-45"])); s.pme_grid = mesh
    path, L = pc.expected_path(s)
    mob = s.mass != 0.0
    expect = _reference(oracle_mod, ("long", mesh, n_mobile), s)
    g = Engine(s, _integ().to_data(precision=0))
    c0 = _counts(g)
    _parity(g, expect, 0, mob, "long %dx%dx%d-%d %s block=%s" % (mesh + (n_mobile, path, "x".join(map(str, L)))))
    _assert_counter(c0, _counts(g), 0, path, "long axis")
    g.close()
    tune(pme_general=1)
    g = Engine(s, _integ().to_data(precision=0))
    c0 = _counts(g)
    _parity(g, expect, 0, mob, "long %dx%dx%d-%d dedicated-general" % (mesh + (n_mobile,)))
    _assert_counter(c0, _counts(g), 0, "general:host", "long axis, general")
    g.close()
