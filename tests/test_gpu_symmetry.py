"""GPU suite: exact symmetries of the potential on every force path of the HIP engine, with no reference at all.

A System with its atoms in another order, its term lists shuffled and turned round, its molecules boxes away from each other, its axes
exchanged or (in vacuum) rotated as a whole is the same physics (tests/symmetry.py; proved on the fp64 oracle by
tests/test_symmetry_cpu.py).  The engine maps caller order -> Hilbert-sorted image order -> i-slots -> group-list positions -> u16
per-atom entries and keeps `orig`, `sx_row`, `mlist`, GenAtom and FragRec tables beside them; the Hilbert sort, the bounding boxes and
spheres, the prefilter of the atoms'-list builder and the PME mesh treat x, y and z in separate code.  A slip in any of these that is
the identity for "ligand at atoms 0..14, molecules contiguous, lists ascending, coordinates in [0, box), cubic box" passes every parity
test; here it shows as two runs of the ENGINE disagreeing.  Nothing in this file asks the oracle for an expected value.

Tolerances are the project's contract between engine and oracle, applied between two runs of the engine: energies and forces 1e-10 in
double (1e-9 on the S23k row, tests/test_gpu_parity.py::test_s23k_parity_frozen_and_full), 1e-5 in mixed precision; work trace 1e-9 of
max|w| and positions 1e-9 nm in double (test_short_switch_work_trace), work 1e-5 in mixed; force = -dE/dx as
tests/test_oracle_golden.py::test_forces_are_energy_gradient (rel 2e-5, abs 2e-3).  Each case prints its residuals ("SYMMETRY ..."
lines, pytest -s); the table of a run is profiles/symmetry/README.md."""
import copy
import os

import numpy as np
import pytest

import ethylene as eth
import symmetry as sym
from blues_amd import amber, integrators, systems

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VAC_ALCHEMICAL = {"TOL-parm": list(range(15)), "vacDivaline": list(range(22, 32))}
STATIC_LAMBDAS = ((1.0, 1.0), (0.4, 0.2))
PERIODIC_ROWS = ("tile", "atom", "frag", "pme")
VAC_ROWS = ("vacDivaline", "TOL-parm", "ethylene")
PERIODIC_TRANSFORMS = ("molecule_order", "scatter+shuffle", "unwrap", "cycle_axes")
VAC_TRANSFORMS = ("scatter+shuffle", "rotate")
# the kernel a lone all-mobile 1,950-atom chain gets (stats()["nonbonded_kernel"], by precision): 31 i-tiles x 1 replica <= 32 keeps
# the fused one-launch force pass in both precisions, whose nonbonded part is the tile kernel (blues_engine.hip: sort_and_tile)
TILE_KERNEL = {1: 0, 0: 0}


@pytest.fixture(scope="module")
def Engine():
    from blues_amd import build
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


def _tol(row, precision):
    if precision == 0:
        return 1e-5
    return 1e-9 if row == "atom" else 1e-10


def _row_system(row, tol_box):
    """(System, velocities or None) of a row of the table in the module docstring of profiles/symmetry/README.md."""
    s, v = tol_box
    if row in ("tile", "frag", "pme"):
        big = systems.tile_system(s, (1, 1, 2))            # 1,950 atoms, 2.18 x 2.18 x 4.36 nm, everything mobile
        if row == "pme":
            big = systems.with_reciprocal_space(big)
            assert len(set(big.pme_grid)) > 1              # the mesh differs per axis
        return big, np.concatenate([v, v])
    if row == "atom":
        return systems.s23k(275, frozen=True)
    if row == "ethylene":
        return eth.load()[0], None
    prm = amber.read_prmtop(os.path.join(GOLDEN, row + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, row + ".inpcrd"))
    return amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=VAC_ALCHEMICAL[row], nonbonded_method="NoCutoff"), None


def _set_tuning(row, tune):
    if row == "atom":
        tune(assume_batch=1024)
    elif row == "frag":
        tune(k1_mode=3)


def _check_path(row, precision, g):
    """Each row runs the kernel it means to run."""
    st = g.stats()
    if row == "tile":
        assert st["nonbonded_kernel"] == TILE_KERNEL[precision], st
    elif row == "atom":
        if precision == 0:
            assert st["nonbonded_kernel"] == 2 and st["pruned_lists"] == 1 and st["alchemical_kernel"] == 1, st
    elif row == "frag":
        assert st["nonbonded_kernel"] == 3, st
    elif row == "pme":
        t = g.energy_terms()
        assert t[8] != 0.0 and t[9] != 0.0, t
    else:
        assert st["nonbonded_kernel"] == 4 and st["list_builds"] == 0, st


def _steps(transform):
    scatter = lambda s, v: sym.permute_atoms(s, v, sym.scatter_perm(s.n_atoms, 11))
    shuffle = lambda s, v: sym.shuffle_terms(s, np.random.RandomState(12), v)
    return {"molecule_order": [lambda s, v: sym.permute_atoms(s, v, sym.molecule_order_perm(s))],
            "scatter+shuffle": [scatter, shuffle],
            "unwrap": [lambda s, v: sym.unwrap_molecules(s, np.random.RandomState(13), 3, v)],
            "cycle_axes": [sym.cycle_axes],
            "rotate": [lambda s, v: sym.rotate(s, v, sym.rotation_matrix([0.3, -1.0, 0.5], 2.1), (0.7, -1.3, 0.4))]}[transform]


def _data(row, precision, nsteps=12, zero_rate=False):
    dt, T = (0.001, 200.0) if row == "ethylene" else ((0.002, 300.0) if row in VAC_ROWS else (0.004, 300.0))
    if zero_rate:
        integ = integrators.AlchemicalExternalLangevinIntegrator(integrators.DEFAULT_ALCHEMICAL_FUNCTIONS, splitting="H V R O R V H", temperature=T,
                                                                  collision_rate=0.0, timestep=dt, nsteps_neq=nsteps, seed=7)
    else:
        integ = integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=dt, temperature=T, seed=7)
    return integ.to_data(precision=precision)


def _static(g, lambdas=STATIC_LAMBDAS):
    out = []
    for ls, le in lambdas:
        g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        out.append((g.energy_terms(), g.potential_energy(), g.get_forces()))
    return out


@pytest.fixture(scope="module")
def originals(Engine, tol_box):
    """The untransformed engine of a (row, precision) and what it computes: made once, by the first test that asks (under the tuning
    that test has set), kept alive so that the transformed Systems meet blues_engine_create's content-hashed HostTopology sharing with
    the original still there, and left unchanged (positions, velocities and lambdas are set by nobody else)."""
    cache = {}

    def get(row, precision):
        key = (row, precision)
        if key not in cache:
            s, v = _row_system(row, tol_box)
            g = Engine(s, _data(row, precision))
            cache[key] = {"s": s, "v": v, "g": g, "static": _static(g), "audit": g.audit_lists() if row in ("atom", "frag") and precision == 0 else None}
        return cache[key]
    yield get
    for c in cache.values():
        c["g"].close()


def _report(kind, row, precision, transform, what, value, bound):
    print("SYMMETRY %-8s %-12s %-6s %-16s %-22s %.3e (bound %.1e)" % (kind, row, "double" if precision else "mixed", transform, what, value, bound))


STATIC_CASES = [(r, p, t) for r in PERIODIC_ROWS for p in ((0,) if r == "frag" else (1, 0)) for t in PERIODIC_TRANSFORMS] + \
               [(r, p, t) for r in VAC_ROWS for p in (1, 0) for t in VAC_TRANSFORMS]


@pytest.mark.parametrize("row,precision,transform", STATIC_CASES)
def test_static_symmetry(Engine, originals, tune, row, precision, transform):
    """energy_terms(), potential_energy() and get_forces() of the transformed System, mapped back, equal the original's."""
    _set_tuning(row, tune)
    o = originals(row, precision)
    s, tol = o["s"], _tol(row, precision)
    s2, _, m = sym.chain(s, o["v"], *_steps(transform))
    g2 = Engine(s2, _data(row, precision))
    got = _static(g2)
    mob, mob2 = s.mass > 0, s2.mass > 0
    worst_e = worst_f = 0.0
    fails = []
    for (ls, le), (t0, e0, f0), (t1, e1, f1) in zip(STATIC_LAMBDAS, o["static"], got):
        res = [abs(t1[k] - t0[k]) / max(abs(t0[k]), 1.0) for k in range(10)] + [abs(e1 - e0) / max(abs(e0), 1.0)]
        worst_e = max(worst_e, max(res))
        if max(res) > tol:
            fails.append(("energy", ls, le, int(np.argmax(res)), max(res)))
        fb = m.vectors(f1)
        rf = np.abs(fb[mob] - f0[mob]).max() / np.abs(f0[mob]).max()
        worst_f = max(worst_f, rf)
        if rf > tol:
            fails.append(("forces", ls, le, int(np.argmax(np.abs(fb - f0).max(1))), rf))
        assert np.all(f1[~mob2] == 0.0) and np.all(f0[~mob] == 0.0)          # frozen atoms receive exactly no force
        assert np.abs(f0[mob]).max() > 1.0
    _report("static", row, precision, transform, "energy terms", worst_e, tol)
    _report("static", row, precision, transform, "forces", worst_f, tol)
    if row in ("atom", "frag") and precision == 0:         # (blues_audit_lists walks the mixed-precision lists: there are no others)
        found2, missing2 = g2.audit_lists()
        found, missing = o["audit"]
        _report("static", row, precision, transform, "audit found %d vs %d" % (found2, found), float(missing2), 0.0)
        assert missing == 0 and missing2 == 0, (found, missing, found2, missing2)
        if transform in ("molecule_order", "scatter+shuffle", "cycle_axes"):
            # the same coordinates (cycle_axes: the same three numbers per atom, the same edge under each), so the same fixed-point
            # image and the same set of pairs in range
            assert found2 == found, (found, found2)
        else:
            # unwrap: the global shift is no multiple of the image's quantum (edge / 2^32, <= 2.1e-9 nm here), so every coordinate
            # rounds afresh and a pair distance moves by up to ~7e-9 nm; pairs within that of the cutoff may change sides.  With
            # `found` pairs in a sphere of radius r_c = 1 nm the count per nm of distance at r_c is 3 found / r_c: ~1e-3 pairs expected
            assert abs(found2 - found) <= 2, (found, found2)
    _check_path(row, precision, o["g"]); _check_path(row, precision, g2)
    g2.close()
    assert not fails, fails


DYNAMIC_CASES = [(r, 1, t) for r in ("tile", "atom") for t in PERIODIC_TRANSFORMS] + [("atom", 0, t) for t in PERIODIC_TRANSFORMS] + \
                [(r, 1, t) for r in VAC_ROWS for t in VAC_TRANSFORMS]


@pytest.mark.parametrize("row,precision,transform", DYNAMIC_CASES)
def test_noise_free_switch(Engine, tol_box, tune, row, precision, transform):
    """A 12-step switch without noise from transformed positions and velocities.  The Philox counter is keyed by the caller's atom
    index, so a permuted System would draw other numbers per physical atom; the program therefore carries none:
    AlchemicalExternalLangevinIntegrator(collision_rate=0) with the default splitting `H V R O R V H` IS WHAT RUNS (engine and oracle
    both take a zero rate: the O substep becomes v <- 1 v + 0 xi), so the fused step kernel of the default program is exercised, not
    the interpreter of an O-free splitting.  HBonds Systems only (general clusters sweep in atom-index order and legitimately differ
    at the solver tolerance).  Velocities without a fixture (vacuum rows) are drawn once by the engine itself."""
    _set_tuning(row, tune)
    n = 12
    s, v = _row_system(row, tol_box)
    data = _data(row, precision, n, zero_rate=True)
    g = Engine(s, data)
    if v is None:
        g.set_velocities_to_temperature(data.temperature, 11); v = g.get_velocities()
    g.set_velocities(v)
    s2, v2, m = sym.chain(s, v, *_steps(transform))
    g2 = Engine(s2, data); g2.set_velocities(v2)
    w, w2 = g.run_switch(n, trace=True), g2.run_switch(n, trace=True)
    wtol, xtol = (1e-9, 1e-9) if precision else (1e-5, None)
    scale = np.abs(w).max()
    assert scale > 1e-3 and np.all(np.isfinite(w2))                     # the protocol does work: the traces compare something
    rw = np.abs(w2 - w).max() / scale
    _report("dynamic", row, precision, transform, "work trace", rw, wtol)
    x, x2 = g.get_positions(), m.positions(g2.get_positions())
    d = x2 - x
    if row not in VAC_ROWS:
        box = np.asarray(s.box, dtype=np.float64)
        d -= box * np.rint(d / box)                                      # modulo each molecule's lattice shift (and the engine's own wrapping)
    mob = s.mass > 0
    assert np.abs(x - s.positions)[mob].max() > 1e-3                    # the atoms moved
    _report("dynamic", row, precision, transform, "positions [nm]", np.abs(d).max(), xtol or float("nan"))
    st, st2 = g.stats(), g2.stats()
    g.close(); g2.close()
    assert rw <= wtol, (rw, w[-1], w2[-1])
    if xtol is not None:
        assert np.abs(d).max() <= xtol, np.abs(d).max()
    if (~mob).any():
        assert np.abs(d[~mob]).max() <= 1e-12                           # frozen atoms stay where they were put (to the rounding of mapping them back)
    if row in VAC_ROWS:
        assert st["list_builds"] == 0 and st2["list_builds"] == 0
    else:
        assert st["list_builds"] >= 1 and st2["list_builds"] >= 1       # equal in kind; their number follows the sort, not the physics


@pytest.mark.parametrize("row", ("atom", "vacDivaline", "TOL-parm"))
@pytest.mark.parametrize("precision", (1, 0))
def test_alchemical_identities(Engine, originals, tune, row, precision):
    """(i) At lambda = (1, 1) energies and forces equal those of the same System with no alchemical atom at all: the softcore forms of
    the alchemical kernel against the plain forms of the nonbonded one.  (ii) At lambda = (0, 0) with the defaults (sterics decoupled,
    electrostatics annihilated) the environment does not feel where the ligand is.  Both hold for the oracle
    (tests/test_oracle_golden.py::test_invariances_and_lambda_one).  The ethylene System is left out: its pair form acts only between
    alchemical and other atoms (no plain System to compare with) and its q / r^2 is scaled by no lambda; (ii) needs a ligand that is a
    whole molecule, so vacDivaline takes part in (i) only."""
    _set_tuning(row, tune)
    o = originals(row, precision)
    s, tol = o["s"], _tol(row, precision)
    mob = s.mass > 0
    plain = copy.copy(s); plain.alchemical_atoms = np.zeros(0, np.int32)
    p = Engine(plain, _data(row, precision))
    (t0, e0, f0), (t1, e1, f1) = o["static"][0], _static(p, ((1.0, 1.0),))[0]
    p.close()
    re, rf = abs(e1 - e0) / max(abs(e0), 1.0), np.abs(f1[mob] - f0[mob]).max() / np.abs(f0[mob]).max()
    bonded = max(abs(t1[k] - t0[k]) / max(abs(t0[k]), 1.0) for k in (0, 1, 2, 7, 8, 9))
    _report("identity", row, precision, "lambda=1 vs plain", "energy", max(re, bonded), tol)
    _report("identity", row, precision, "lambda=1 vs plain", "forces", rf, tol)
    assert t1[5] == 0.0 and t1[6] == 0.0 and (t0[5] != 0.0 or t0[6] != 0.0)
    assert abs((t1[3] + t1[4]) - (t0[3] + t0[4] + t0[5] + t0[6])) <= tol * max(abs(t1[3] + t1[4]), 1.0)
    assert re <= tol and bonded <= tol and rf <= tol, (re, bonded, rf)
    # (ii) where the ligand is a molecule of its own (vacDivaline's side chain is bonded to its backbone: moving it alone is no symmetry);
    # an engine of its own: the shared original is left as it is
    label = sym.molecules(s)
    if not np.array_equal(np.nonzero(np.isin(label, label[np.asarray(s.alchemical_atoms, np.int64)]))[0], np.sort(s.alchemical_atoms)):
        assert row == "vacDivaline"
        return
    g = Engine(s, _data(row, precision))
    (_, ea, fa), = _static(g, ((0.0, 0.0),))
    lig = np.asarray(s.alchemical_atoms, np.int64)
    x = np.array(s.positions, dtype=np.float64); x[lig] += np.array([0.3, 0.2, -0.1])
    g.set_positions(x)
    (_, eb, fb), = _static(g, ((0.0, 0.0),))
    _check_path(row, precision, g)
    g.close()
    env = mob.copy(); env[lig] = False
    rf = np.abs(fb[env] - fa[env]).max() / np.abs(fa[env]).max()
    re = abs(eb - ea) / max(abs(ea), 1.0)
    _report("identity", row, precision, "decoupled ligand", "energy", re, tol)
    _report("identity", row, precision, "decoupled ligand", "environment forces", rf, tol)
    assert env.sum() > 10 and rf <= tol and re <= tol, (rf, re)
    assert np.abs(fb[lig] - fa[lig]).max() <= tol * np.abs(fa[mob]).max()      # what is left on the ligand is its own bonded terms


@pytest.mark.parametrize("row", ("tile", "atom", "pme") + VAC_ROWS)
def test_forces_are_the_energy_gradient(Engine, tol_box, tune, row):
    """Central differences (h = 1e-5 nm) of potential_energy() against get_forces() in double precision at lambda = (0.45, 0.2), on six
    (atom, component) picks of a seeded draw: three ligand atoms and three mobile environment atoms, one of them in a constraint
    cluster (the ethylene System has no mobile environment: its three ligand picks only).  The force forms and the energy forms of the
    nonbonded and alchemical kernels are separate instantiations; this ties them to each other without the oracle."""
    _set_tuning(row, tune)
    s, _ = _row_system(row, tol_box)
    g = Engine(s, _data(row, 1))
    g.set_global("lambda_sterics", 0.45); g.set_global("lambda_electrostatics", 0.2)
    rng = np.random.RandomState(5)
    lig = np.asarray(s.alchemical_atoms, np.int64)
    env = np.ones(s.n_atoms, bool); env[lig] = False; env &= s.mass > 0
    constrained = np.zeros(s.n_atoms, bool); constrained[np.asarray(s.constraint_atoms, np.int64).reshape(-1)] = True
    picks = list(rng.choice(lig[s.mass[lig] > 0], 3, replace=False))
    if env.any():
        picks += list(rng.choice(np.nonzero(env & constrained)[0], 1)) + list(rng.choice(np.nonzero(env)[0], 2, replace=False))
    x0 = np.array(s.positions, dtype=np.float64)
    f = g.get_forces()
    h = 1e-5
    worst = 0.0
    for i in picks:
        k = rng.randint(3)
        xp = x0.copy(); xp[i, k] += h; g.set_positions(xp); ep = g.potential_energy()
        xm = x0.copy(); xm[i, k] -= h; g.set_positions(xm); em = g.potential_energy()
        fd = -(ep - em) / (2 * h)
        worst = max(worst, abs(f[i, k] - fd) / max(abs(fd), 100.0))
        assert f[i, k] == pytest.approx(fd, rel=2e-5, abs=2e-3), (int(i), k, f[i, k], fd)
    _report("gradient", row, 1, "-", "|f + dE/dx| / max(|f|, 100)", worst, 2e-5)
    _check_path(row, 1, g)
    g.close()
