"""GPU suite: alchemical regions of 1 to 64 atoms -- the range blues_engine_create accepts -- on every pair path, against the CPU oracle.

The alchemical kernels are shaped by PA, the region's size padded to a power of two: lanes per j-slot, the widths of the segmented
reductions and of the butterfly, the rows per sweep of the alchemical-by-alchemical block (kernels_alch.h: alchemical_body), the
PA-strided staging of the partial sums (kernels_integrate.h: fin_alch_self, its fused copy in the step kernel, the ledger), the
[9][64] table the integrator kernels read, the 256-entry trips over the exception rows, the staging rounds of the dense forms, the exact
PME treatment's per-atom arrays and the NoCutoff layout.  The rest of the suite reaches PA = 1, 4 and 16 with at most 27 exception rows and
one staging round.  Here: tests/alch_regions.py's regions at SIZES = 1 .. 64 (every PA, both sides of each power of two), with
NativeEngine.alchemical_layout() asserting which shape ran.

Bars (tests/test_gpu_parity.py, tests/test_gpu_nocutoff.py): double -- energy terms 1e-10 of max(|term|, 1), forces 1e-10 of the largest,
work trace 1e-9 of its scale; mixed -- 1e-5 each.  Positions after a switch as test_short_switch_work_trace: 1e-9 / 2e-4 nm.
The oracle's answers are cached per (System, region) at module scope and shared by precisions and layouts.
"""
import os

import numpy as np
import pytest

import alch_regions as ar
import exact_pme_reference as xref
import gb_reference as gbr
import test_gpu_energy_ledger as ledger
from blues_amd import amber, integrators, systems

pytestmark = pytest.mark.gpu

LAMBDAS = ((1.0, 1.0), (0.5, 0.3), (0.05, 0.0), (0.0, 0.0))
TOL = {1: 1e-10, 0: 1e-5}          # energy terms, forces
WTOL = {1: 1e-9, 0: 1e-5}          # work trace
PTOL = {1: 1e-9, 0: 2e-4}          # positions after the switch (nm)
PRECISIONS = [1, 0]
NSTEPS = 12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _integ(n=NSTEPS, dt=0.004, seed=7):
    return integrators.generateNCMCIntegrator(nstepsNC=n, dt=dt, temperature=300.0, seed=seed)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


# ---- the oracle's answers, once per (System, region)
_STATIC, _TRACE, _SYSTEMS = {}, {}, {}


def _static(oracle_mod, key, s, openmp=False):
    """{(ls, le): (E, F, terms)} at the System's positions"""
    if key not in _STATIC:
        o = oracle_mod.Oracle(s, _integ().to_data(precision=1), openmp=openmp)
        _STATIC[key] = {lam: o.energy_forces(*lam) for lam in LAMBDAS}
    return _STATIC[key]


def _trace(oracle_mod, key, s, v, dt=0.004):
    """(work after every step, final positions) of the NSTEPS-step switch; v = None: velocities drawn by the oracle (returned third)"""
    if key not in _TRACE:
        o = oracle_mod.Oracle(s, _integ(dt=dt).to_data(precision=1))
        if v is None:
            o.set_velocities_to_temperature(300.0, 11); v = o.get_velocities()
        else:
            o.set_velocities(v)
        w = []
        for _ in range(NSTEPS):
            o.step(1); w.append(o.get_global("protocol_work"))
        _TRACE[key] = (np.array(w), o.get_positions(), v)
    return _TRACE[key]


def _check_static(g, ref, precision, nterms=8, mobile=None, tag=""):
    tol = TOL[precision]
    sel = slice(None) if mobile is None else mobile
    for (ls, le) in LAMBDAS:
        eo, fo, to = ref[(ls, le)]
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        tg = g.energy_terms()
        fg = g.get_forces()
        worst = max(abs(tg[k] - to[k]) / max(abs(to[k]), 1.0) for k in range(nterms))
        print("ALCH-REGION %s precision=%d (%.2f, %.2f): terms %.3e total %.3e forces %.3e" % (tag, precision, ls, le, worst, abs(tg.sum() - eo) / max(abs(eo), 1.0), _rel(fg[sel], fo[sel])))
        for k in range(nterms):
            assert abs(tg[k] - to[k]) <= tol * max(abs(to[k]), 1.0), (tag, ls, le, k, tg[k], to[k])
        assert abs(tg.sum() - eo) <= tol * max(abs(eo), 1.0), (tag, ls, le, tg.sum(), eo)
        assert _rel(fg[sel], fo[sel]) <= tol, (tag, ls, le, _rel(fg[sel], fo[sel]))
    g.set_global("lambda_sterics", 1.0); g.set_global("lambda_electrostatics", 1.0)


def _check_trace(g, ref, precision, v, tag="", ptol=None):
    wo, xo = ref[0], ref[1]
    g.set_velocities(v)
    wg = g.run_switch(NSTEPS, trace=True)
    scale = max(1.0, np.abs(wo).max())
    dx = np.abs(g.get_positions() - xo).max()
    print("ALCH-REGION %s precision=%d trace: work %.3e of %.4g, positions %.3e nm" % (tag, precision, np.abs(wg - wo).max() / scale, scale, dx))
    assert np.abs(wg - wo).max() <= WTOL[precision] * scale, (tag, wg, wo)
    assert dx < (PTOL[precision] if ptol is None else ptol), (tag, dx)
    return wg


def _layout(g, n, jiter=None, entries=None):
    lay = g.alchemical_layout()
    assert lay is not None, "the library has no blues_get_alchemical_layout: rebuild it"
    assert lay[0] == ar.padded(n), (n, lay)
    if jiter is not None:
        assert lay[1] == min(jiter, ar.padded(n)), (n, jiter, lay)      # (the clamp to PA: an env block stages (256 / PA) * jiter entries)
    if entries is not None:
        assert lay[3] == entries, (n, lay)
    return lay


def _box_system(tol_box, kind, n):
    """name -> System over the toluene box"""
    key = (kind, n)
    if key not in _SYSTEMS:
        s = tol_box[0]
        if kind == "compact":
            out = ar.with_region(s, ar.compact(s, n))
        elif kind == "scattered":
            out = ar.with_region(s, ar.scattered(s, n))
        elif kind == "pme":
            out = systems.with_reciprocal_space(ar.with_region(s, ar.compact(s, n)))
        elif kind == "exact":
            out = systems.with_alchemical_pme_treatment(systems.with_reciprocal_space(ar.with_region(s, ar.compact(s, n))), "exact")
        elif kind.startswith("synthetic"):      # synthetic-<pairs>-<env pairs>
            _, pairs, env = kind.split("-")
            out = ar.with_synthetic_exceptions(s, ar.compact(s, n), int(pairs), 1, int(env))[0]
        _SYSTEMS[key] = out
    return _SYSTEMS[key]


LAYOUTS = (("lone", dict(assume_batch=0), 1), ("batch8", dict(assume_batch=8), 8))      # (name, tuning, the k2_jiter the host picks before its clamp to PA)


# ---- a. static parity over SIZES: the lone default (fused force launch) and the decomposition of a batch (k_alchemical + k_finalize)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", ar.SIZES)
def test_static_parity_compact_regions(Engine, oracle_mod, tol_box, tune, n, precision):
    s = _box_system(tol_box, "compact", n)
    ref = _static(oracle_mod, ("compact", n), s)
    for name, tuning, jiter in LAYOUTS:
        tune(**tuning)
        g = Engine(s, _integ().to_data(precision=precision))
        _check_static(g, ref, precision, tag="compact n=%d %s" % (n, name))
        lay = _layout(g, n, jiter, ar.exception_row_entries(s, s.alchemical_atoms))
        assert lay[2] > 0 and g.stats()["alchemical_kernel"] == 0
        g.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [8, 32, 64])
def test_static_parity_scattered_regions(Engine, oracle_mod, tol_box, tune, n, precision):
    """Waters from all over the box (extent > 1 nm): the alchemical tile's bounding box and its list are as large as the box allows."""
    s = _box_system(tol_box, "scattered", n)
    ref = _static(oracle_mod, ("scattered", n), s)
    counts = []
    for name, tuning, jiter in LAYOUTS:
        tune(**tuning)
        g = Engine(s, _integ().to_data(precision=precision))
        _check_static(g, ref, precision, tag="scattered n=%d %s" % (n, name))
        counts.append(_layout(g, n, jiter, 0)[2])
        g.close()
    if n > 8:
        assert min(counts) > 900, counts      # (most of the 975 - n environment atoms are in the list)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("jiter", [1, 8])
@pytest.mark.parametrize("n", [2, 33, 64])
def test_static_parity_with_pinned_j_groups(Engine, oracle_mod, tol_box, tune, n, jiter, precision):
    """BluesTuning.k2_jiter pinned to 1 and to 8: the host clamps it to PA (2 at n = 2), which the accessor shows."""
    s = _box_system(tol_box, "compact", n)
    ref = _static(oracle_mod, ("compact", n), s)
    for name, tuning, default in LAYOUTS:
        if jiter == default:      # (that layout's own choice: test_static_parity_compact_regions ran it)
            continue
        tune(k2_jiter=jiter, **tuning)
        g = Engine(s, _integ().to_data(precision=precision))
        _check_static(g, ref, precision, tag="compact n=%d %s jiter=%d" % (n, name, jiter))
        _layout(g, n, jiter)
        g.close()


# ---- b. fragment lists, reciprocal space, the exact PME treatment
@pytest.mark.parametrize("n", [33, 64])
def test_static_parity_fragment_lists(Engine, oracle_mod, tol_box, tune, n, precision=0):
    """(mixed precision: the fragment lists are a path of that mode only -- in double precision the engine keeps the tile kernel)"""
    s = _box_system(tol_box, "compact", n)
    ref = _static(oracle_mod, ("compact", n), s)
    tune(k1_mode=3, assume_batch=4)      # (tests/test_gpu_frag.py)
    g = Engine(s, _integ().to_data(precision=precision))
    assert g.stats()["nonbonded_kernel"] == 3, g.stats()
    _check_static(g, ref, precision, tag="fragment lists n=%d" % n)
    _layout(g, n)
    found, missing = g.audit_lists()
    assert found > 0 and missing == 0
    g.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [17, 64])
def test_static_parity_reciprocal_space(Engine, oracle_mod, tol_box, n, precision):
    s = _box_system(tol_box, "pme", n)
    ref = _static(oracle_mod, ("pme", n), s)
    g = Engine(s, _integ().to_data(precision=precision))
    _check_static(g, ref, precision, nterms=10, tag="reciprocal space n=%d" % n)
    assert ref[(1.0, 1.0)][2][8] != 0.0 and ref[(1.0, 1.0)][2][9] != 0.0
    _layout(g, n)
    g.close()


_EXACT = {}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [16, 64])
def test_exact_pme_treatment(Engine, tol_box, n, precision):
    """kernels_pme.h: PMEX_MAX_ALCH = 64 (run so far at 15 and 4 atoms).  Against tests/exact_pme_reference.py by its GROUPS, with the
    bars of tests/test_gpu_exact_pme.py; 975 mobile atoms: the general mesh path serves the alchemical class."""
    s = _box_system(tol_box, "exact", n)
    if n not in _EXACT:
        ref = xref.ExactPmeReference(s, openmp=True)
        _EXACT[n] = {lam: ref.evaluate(s.positions, *lam) for lam in LAMBDAS}
    tol = TOL[precision]
    g = Engine(s, _integ().to_data(precision=precision))
    for (ls, le) in LAMBDAS:
        eo, fo, to = _EXACT[n][(ls, le)]
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        tg = g.energy_terms()
        gg, go = xref.group_terms(tg), xref.group_terms(to)
        f = g.get_forces()
        print("ALCH-REGION exact n=%d precision=%d (%.2f, %.2f): groups %s forces %.3e" % (n, precision, ls, le, " ".join("%.2e" % d for d in gg - go), _rel(f, fo)))
        for k in range(len(go)):
            assert abs(gg[k] - go[k]) <= tol * max(abs(go[k]), 1.0), (ls, le, k, gg[k], go[k])
        assert abs(tg.sum() - eo) <= tol * abs(eo)
        assert _rel(f, fo) <= tol, (ls, le, _rel(f, fo))
    st = g.stats()
    assert st["exact_pme_general_launches"] > 0 and st["exact_pme_fast_launches"] == 0, st
    _layout(g, n)
    g.close()


# ---- c. work traces
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [2, 17, 33, 64])
def test_switch_work_trace(Engine, oracle_mod, tol_box, n, precision):
    """A 12-step switch from the fixture's velocities: the work at every step and the final positions (the step kernel's fused copy of
    fin_alch_self and the [9][64] table feed every kick)."""
    s, v = _box_system(tol_box, "compact", n), tol_box[1]
    ref = _trace(oracle_mod, ("compact", n), s, v)
    g = Engine(s, _integ().to_data(precision=precision))
    _check_trace(g, ref, precision, v, tag="compact n=%d" % n)
    _layout(g, n)
    assert g.get_global("step") == NSTEPS
    g.close()


@pytest.mark.parametrize("n", [33, 64])
def test_batch_member_equals_the_lone_chain_bitwise(Engine, oracle_mod, tol_box, tune, n):
    """The same switch as member 0 of a batch of 8 (k_alchemical + k_finalize over gridDim.y = 8) and alone, laid out the same way
    (tune(assume_batch=8)): bit for bit, as tests/test_gpu_general_constraints.py::test_batch_equals_lone_chain_bitwise."""
    from blues_amd.engine import NativeBatch
    s, v = _box_system(tol_box, "compact", n), tol_box[1]
    R = 8
    tune(assume_batch=R)

    def make(r):
        e = Engine(s, _integ(seed=40 + r).to_data(precision=0, replica=r))
        e.set_velocities(v * (1.0 + 0.01 * r))
        return e
    lone = make(0)
    wl = lone.run_switch(NSTEPS, trace=True)
    xl, vl = lone.get_positions(), lone.get_velocities()
    # the stepping path the two share (k_alchemical + k_finalize) against the oracle's chain of the same seed
    o = oracle_mod.Oracle(s, _integ(seed=40).to_data(precision=1, replica=0)); o.set_velocities(v)
    wo = []
    for _ in range(NSTEPS):
        o.step(1); wo.append(o.get_global("protocol_work"))
    print("ALCH-REGION batch8 layout n=%d trace: work %.3e of %.4g" % (n, np.abs(wl - wo).max() / np.abs(wo).max(), np.abs(wo).max()))
    assert np.abs(wl - wo).max() <= WTOL[0] * max(1.0, np.abs(wo).max()) and np.abs(xl - o.get_positions()).max() < PTOL[0]
    _layout(lone, n, 8)
    lone.close()
    engs = [make(r) for r in range(R)]
    batch = NativeBatch(engs)
    try:
        _, w = batch.step(NSTEPS, trace=True)
        assert np.array_equal(w[0], wl), (w[0], wl)
        assert np.array_equal(engs[0].get_positions(), xl) and np.array_equal(engs[0].get_velocities(), vl)
        assert np.all(np.isfinite(w)) and len({tuple(row) for row in w}) == R      # eight different chains
        st = batch.stats()
        assert st["fallback_steps"] == 0 and st["lockstep_steps"] > 0, st
    finally:
        batch.close()
        for e in engs:
            e.close()


@pytest.mark.parametrize("precision,tol,dt", ledger.CASES)
@pytest.mark.parametrize("n", [33, 64])
def test_heat_and_shadow_work_ledger(Engine, oracle_mod, tol_box, n, precision, tol, dt):
    """measure_shadow_work / measure_heat on (kernels_integrate.h: ledger_pe_body sums the alchemical partials with its own PA-strided
    staging): heat and shadow work after every one of 12 steps against the oracle, and the ledger's identity on the engine's own numbers,
    as tests/test_gpu_energy_ledger.py::test_heat_and_shadow_work_match_the_oracle with its bars."""
    s, v = _box_system(tol_box, "compact", n), tol_box[1]
    data = ledger._integ(dt).to_data(precision=precision)
    g, o = Engine(s, data), oracle_mod.Oracle(s, data)
    x, v = ledger._start(Engine, s, v)
    g.set_positions(x); o.set_positions(x); g.set_velocities(v); o.set_velocities(v)
    big_s, big_q = ledger._ledger_run(g, s, 12, tol, 0.0 if precision else 5e-7, o=o)
    assert big_q > 1e-3 and big_s > 1e-3
    _layout(g, n)
    g.close()


# ---- d. exception rows beyond 256: the second trip of the alchemical-by-alchemical block's row loop and its row clipping
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,entries", [("synthetic-150-0", 354), ("synthetic-101-0", 256), ("synthetic-101-1", 257)])
def test_exception_rows_beyond_256(Engine, oracle_mod, tol_box, tune, kind, entries, precision):
    """The 64-atom region with synthetic (toluene atom, alchemical-water atom) exceptions: 354 row entries (two trips of the 256-entry
    loop), exactly 256 (one full trip) and 257 (a second trip of one entry; the odd one is an alchemical-environment exception)."""
    s, v = _box_system(tol_box, kind, 64), tol_box[1]
    ref = _static(oracle_mod, (kind, 64), s)
    for name, tuning, jiter in LAYOUTS:
        tune(**tuning)
        g = Engine(s, _integ().to_data(precision=precision))
        _check_static(g, ref, precision, tag="%s %s" % (kind, name))
        _layout(g, 64, jiter, entries)
        if name == "lone":
            _check_trace(g, _trace(oracle_mod, (kind, 64), s, v), precision, v, tag=kind)
        g.close()


# ---- e. the 64 limit
def test_the_limit_is_64_atoms(Engine, tol_box):
    from blues_amd.engine import EngineError
    s = tol_box[0]
    g = Engine(ar.with_region(s, ar.compact(s, 64)), _integ().to_data())
    assert g.alchemical_layout()[0] == 64
    g.close()
    with pytest.raises(EngineError, match="more than 64 alchemical atoms"):
        Engine(ar.with_region(s, ar.compact(s, 65)), _integ().to_data())


def test_batch_refuses_members_with_different_regions(Engine, tol_box):
    """Two whole waters each, so the members agree in every size the batch compares first: the reason names the alchemical atoms."""
    from blues_amd.engine import EngineError, NativeBatch
    s = tol_box[0]
    a = Engine(ar.with_region(s, ar.waters_only(s, 2)), _integ().to_data(precision=0))
    b = Engine(ar.with_region(s, ar.waters_only(s, 2, skip=1)), _integ().to_data(precision=0, replica=1))
    batch = NativeBatch([a, b])
    try:
        for e in (a, b):
            e.set_velocities(tol_box[1])
        with pytest.raises(EngineError, match="alchemical atoms"):      # (the members are compared when they first share a launch)
            batch.step(1)
    finally:
        batch.close(); a.close(); b.close()


# ---- f. the dense forms (at most 16 atoms, no alchemical-environment exclusions, mixed precision, large batches)
DENSE_LONG_LIST = (27, 276, 384, 612, 681)      # oxygens of five mobile waters of S23k, extent 0.854 nm: alch_regions.longest_list_waters(s, 5, mobile, 0.86, 1.2) (tests/test_alch_regions_cpu.py)
LONG_LIST_SKIN = 0.5
DENSE_REGIONS = ["1", "2", "3", "4", "5", "toluene", "long_list"]


def _s23k():
    if "s23k" not in _SYSTEMS:
        _SYSTEMS["s23k"] = systems.s23k(mobile_atoms=275, frozen=True)
    return _SYSTEMS["s23k"]


def _dense_region(which):
    s, _ = _s23k()
    mob = np.nonzero(s.mass > 0)[0]
    if which == "toluene":
        return np.arange(15, dtype=np.int32)
    if which == "long_list":
        return np.sort(np.concatenate([np.arange(o, o + 3) for o in DENSE_LONG_LIST])).astype(np.int32)
    if which == "wide":
        return ar.waters_only(s, 5, among=mob, skip=6)
    return ar.waters_only(s, int(which), among=mob)


def _dense_precondition(s, region):
    return 0.5 * float(np.min(s.box)) > s.cutoff + ar.extent(s, region) + 0.3


def _three_forms(Engine, tune, s, which):
    """(fp32 dense body, lane layout, fp64 dense body): k2_dense = default, 0, 2"""
    extra = dict(skin=LONG_LIST_SKIN) if which == "long_list" else {}
    out = []
    for k2_dense in (-1, 0, 2):
        tune(assume_batch=512, k2_dense=k2_dense, **extra)
        out.append(Engine(s, _integ().to_data(precision=0)))
    return out


def _dense_case(which):
    s0, _ = _s23k()
    region = _dense_region(which)
    s = ar.with_region(s0, region)
    assert _dense_precondition(s, region) and (s.mass[region] > 0).all()
    return s, region


@pytest.mark.parametrize("which", DENSE_REGIONS)
def test_dense_forms_against_the_oracle(Engine, oracle_mod, tune, which):
    """k2_dense = default / 0 / 2 report alchemical_kernel 1 / 0 / 2 on regions of 1 to 5 mobile waters (3 to 15 atoms) and on toluene, and
    each form meets the oracle at 1e-5: the eight terms at 1e-5 max(|term|, 1), the total energy, the forces on the mobile atoms.  The
    fp32 dense body's pair energies are good to about 2^-22 of the sum of their magnitudes -- enough for the work of a step, which it
    forms from per-pair differences, not for a term that is the small remainder of large cancelling Coulomb energies: with two
    alchemical waters term [5] = -0.22237 kJ/mol came out 1.3e-5 kJ/mol off.  An energy evaluation of such an engine therefore runs the
    fp64 dense body over the same list (blues_engine.hip: launch_alchemical, `energy`); the force passes keep the fp32 form.

    "long_list": the five mobile waters with the longest list that the host's precondition half_min > cutoff + ext + 0.3 allows
    (tests/alch_regions.py: longest_list_waters, a seeded search over the 87 mobile waters) have 1,849 entries at the engine's own margin
    (cutoff + 0.2 nm) -- no five waters reach K2D_JC = 2560 there.  With BluesTuning.skin pinned to 0.5 nm their list holds 3,107 atoms
    by the CPU count: more than K2D_JC = 2560 and K2F_JC = 2432, so both dense bodies take a second staging round.  The accessor's
    count is asserted."""
    s, region = _dense_case(which)
    ref = _static(oracle_mod, ("s23k", which), s, openmp=True)
    forms = _three_forms(Engine, tune, s, which)
    mob = s.mass > 0
    try:
        assert [g.stats()["alchemical_kernel"] for g in forms] == [1, 0, 2]
        for g, name in zip(forms, ("dense32", "lanes", "dense64")):
            for (ls, le) in LAMBDAS:
                eo, fo, to = ref[(ls, le)]
                g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
                tg, fg = g.energy_terms(), g.get_forces()
                floor = 1.0
                worst = max(abs(tg[k] - to[k]) / max(abs(to[k]), floor) for k in range(8))
                print("ALCH-REGION s23k %s %s (%.2f, %.2f): terms %.3e total %.3e forces %.3e" % (which, name, ls, le, worst, abs(tg.sum() - eo) / abs(eo), _rel(fg[mob], fo[mob])))
                for k in range(8):
                    assert abs(tg[k] - to[k]) <= 1e-5 * max(abs(to[k]), floor), (which, name, ls, le, k, tg[k], to[k])
                assert abs(tg.sum() - eo) <= 1e-5 * abs(eo), (which, name, ls, le)
                assert _rel(fg[mob], fo[mob]) <= 1e-5, (which, name, ls, le, _rel(fg[mob], fo[mob]))
                assert np.all(fg[~mob] == 0.0)
            lay = _layout(g, len(region))
            print("ALCH-REGION s23k %s %s: list entries %d" % (which, name, lay[2]))
            if which == "long_list":
                assert lay[2] > 2560, lay
                assert ar.list_count(s, region, s.cutoff + LONG_LIST_SKIN) > 2560
    finally:
        for g in forms:
            g.close()


def _forms_at(forms, lam):
    for g in forms:
        g.set_global("lambda_sterics", lam[0]); g.set_global("lambda_electrostatics", lam[1])


@pytest.mark.parametrize("which", DENSE_REGIONS)
def test_dense_forms_against_each_other(Engine, tune, which):
    """At the tolerances of tests/test_gpu_batch.py::test_dense_alchemical_kernel_equals_the_lane_layout: total energies of the fp32
    dense body and the lane layout to 1e-9, of the fp64 dense body and the lane layout to 1e-11, forces of the fp32 dense body to 2e-6
    of the largest."""
    s, region = _dense_case(which)
    forms = _three_forms(Engine, tune, s, which)
    d, l, d64 = forms
    mob = s.mass > 0
    try:
        for lam in LAMBDAS:
            _forms_at(forms, lam)
            ed, el, e64 = d.potential_energy(), l.potential_energy(), d64.potential_energy()
            fd, fl = d.get_forces()[mob], l.get_forces()[mob]
            print("ALCH-REGION s23k %s forms (%.2f, %.2f): E32 %.3e E64 %.3e f32 %.3e" % (which, lam[0], lam[1], abs(ed - el) / abs(el), abs(e64 - el) / abs(el), np.abs(fd - fl).max() / np.abs(fl).max()))
            assert abs(ed - el) <= 1e-9 * abs(el), (lam, ed, el)
            assert abs(e64 - el) <= 1e-11 * abs(el), (lam, e64, el)
            assert np.abs(fd - fl).max() <= 2e-6 * np.abs(fl).max(), (lam, np.abs(fd - fl).max())
    finally:
        for g in forms:
            g.close()


@pytest.mark.parametrize("which", DENSE_REGIONS)
def test_fp64_dense_body_forces_equal_the_lane_layout(Engine, tune, which):
    """The same file's bound for the forces of the fp64 dense body against the lane layout: 1e-8 of the largest force + 2e-5 kJ/mol/nm.

    Both forms keep a pair force's components and their sums in fp64 (kernels_alch.h: alchemical_body, alchemical_dense_body) and differ
    by the dense body's 2^-20 fixed point and the summation order: at most 3.9e-6 kJ/mol/nm over these regions, bound 5.5e-5.  While
    both rounded the components to fp32 in mixed precision the water regions missed it -- 1.53e-4 (one water) to 3.83e-4 (two) at
    lambda = (1, 1), largest force 3541: one fp32 rounding of a hydrogen bond's 3.5e3 kJ/mol/nm is up to 1.2e-4 -- and toluene, whose
    alchemical pair forces are small beside the largest force in the box, passed with 2.6e-5."""
    s, region = _dense_case(which)
    forms = _three_forms(Engine, tune, s, which)
    d, l, d64 = forms
    mob = s.mass > 0
    try:
        for lam in LAMBDAS:
            _forms_at(forms, lam)
            f64, fl = d64.get_forces()[mob], l.get_forces()[mob]
            print("ALCH-REGION s23k %s dense64 - lanes (%.2f, %.2f): %.3e kJ/mol/nm, bound %.3e" % (which, lam[0], lam[1], np.abs(f64 - fl).max(), 1e-8 * np.abs(fl).max() + 2e-5))
            assert np.abs(f64 - fl).max() <= 1e-8 * np.abs(fl).max() + 2e-5, (lam, np.abs(f64 - fl).max())
    finally:
        for g in forms:
            g.close()


@pytest.mark.parametrize("which", ["wide", "compact16", "compact17"])
def test_regions_the_dense_forms_do_not_take(Engine, oracle_mod, tune, which):
    """An extent that breaks the host's precondition half_min > cutoff + ext + 0.3, and regions with a partial water (16 and 17 atoms:
    alchemical-environment exclusions): the lane layout runs (kernel 0) and meets the oracle."""
    s0, _ = _s23k()
    region = _dense_region("wide") if which == "wide" else ar.compact(s0, int(which[7:]))
    s = ar.with_region(s0, region)
    if which == "wide":
        assert not _dense_precondition(s, region) and len(region) == 15
    ref = _static(oracle_mod, ("s23k", which), s, openmp=True)
    tune(assume_batch=512)
    g = Engine(s, _integ().to_data(precision=0))
    assert g.stats()["alchemical_kernel"] == 0, g.stats()
    _check_static(g, ref, 0, mobile=s.mass > 0, tag="s23k %s" % which)
    _layout(g, len(region))
    g.close()


# ---- g. NoCutoff: vacDivaline, regions range(n); at 34 the environment is one atom, at 35 there is none
def _divaline(n, implicit_solvent=None):
    key = ("vacDivaline", n, implicit_solvent)
    if key not in _SYSTEMS:
        prm = amber.read_prmtop(os.path.join(GOLDEN, "vacDivaline.prmtop"))
        pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "vacDivaline.inpcrd"))
        kw = {"implicit_solvent": implicit_solvent} if implicit_solvent else {}
        _SYSTEMS[key] = amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=list(range(n)), nonbonded_method="NoCutoff", **kw)
    return _SYSTEMS[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [2, 8, 32, 33, 34, 35])
def test_nocutoff_regions(Engine, oracle_mod, n, precision):
    """The ten terms as tests/test_gpu_nocutoff.py::_check_parity, and a 12-step switch (positions to that file's 1e-8 / 1e-4 nm)."""
    s = _divaline(n)
    assert s.n_atoms == 35
    ref = _static(oracle_mod, ("vacDivaline", n), s)
    g = Engine(s, _integ(dt=0.002).to_data(precision=precision))
    _check_static(g, ref, precision, nterms=10, tag="vacDivaline n=%d" % n)
    for lam in LAMBDAS:
        assert ref[lam][2][8] == 0.0 and ref[lam][2][9] == 0.0
    lay = _layout(g, n, 4, ar.exception_row_entries(s, np.arange(n)))
    assert lay[2] == 35 - n, lay
    st = g.stats()
    assert st["nonbonded_kernel"] == 4 and st["list_builds"] == 0, st
    tr = _trace(oracle_mod, ("vacDivaline", n), s, None, dt=0.002)
    _check_trace(g, tr, precision, tr[2], tag="vacDivaline n=%d" % n, ptol=1e-8 if precision == 1 else 1e-4)
    g.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_nocutoff_33_atoms_with_implicit_solvent(Engine, oracle_mod, precision):
    """n = 33 with GB-OBC2 against the oracle + tests/gb_reference.py, as tests/test_gpu_implicit_solvent.py::_check_parity compares."""
    import dataclasses
    s = _divaline(33, "OBC2")
    tol = TOL[precision]
    ref = _static(oracle_mod, ("vacDivaline", 33), dataclasses.replace(s, implicit_solvent=None))
    coef = gbr.system_coefficients(s)
    g = Engine(s, _integ(dt=0.002).to_data(precision=precision))
    for ls, le in LAMBDAS:
        eo, fo, to = ref[(ls, le)]
        pol, sa, fgb = gbr.evaluate(coef, le)
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        tg = g.energy_terms()
        assert abs(tg[8] - pol) <= tol * max(abs(pol), 1.0), (ls, le, tg[8], pol)
        assert abs(tg[9] - sa) <= tol * max(abs(sa), 1.0), (ls, le, tg[9], sa)
        for k in range(8):
            assert abs(tg[k] - to[k]) <= tol * max(abs(to[k]), 1.0), (ls, le, k, tg[k], to[k])
        total = eo + pol + sa
        assert abs(tg.sum() - total) <= tol * max(abs(total), 1.0), (ls, le, tg.sum(), total)
        fg, fref = g.get_forces(), fo + fgb
        print("ALCH-REGION vacDivaline n=33 OBC2 precision=%d (%.2f, %.2f): forces %.3e" % (precision, ls, le, _rel(fg, fref)))
        assert _rel(fg, fref) <= tol, (ls, le, _rel(fg, fref))
    _layout(g, 33, 4)
    g.close()
