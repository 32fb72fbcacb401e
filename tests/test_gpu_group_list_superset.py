"""Kept supersets of the group lists' candidates (kernels_nb.h: build_lists_body) on a real MI355X.

A rebuild that scans all atoms also keeps, per list, every non-alchemical atom within the list's sphere + a slack D and every mobile
one; later rebuilds run the same tests over that superset while the list's sphere still lies inside it, so the lists must come out
IDENTICAL: same entries, same order, same counts, and with them every force and trajectory.  The shape is the smallest at which this
kernel runs in its benchmark form: one S23k chain with 275 mobile atoms, frozen, mixed precision, laid out as a member of a batch of
1024.  The switch is read when an engine is created, BLUES_GROUP_LIST_SUPERSET (blues_amd/engine.py): 0 = every rebuild scans all atoms,
unset = D of 300 pm, N = D of N pm (20 pm: a hot chain leaves the superset's reach within a few rebuilds, so one run takes the first
derivation, the served rebuild and the fallback).  The same launch also books the rebuild for the mobile atoms only (xbuild, fJ);
every comparison below covers that too.
Reference behaviour being reproduced: the NonbondedForce evaluation behind CustomIntegrator's `f`
(reference blues/integrators.py:159-231)."""
import numpy as np
import pytest

from blues_amd import build, integrators, systems

pytestmark = pytest.mark.gpu

SWITCH = "BLUES_GROUP_LIST_SUPERSET"
LIST_STATS = ("atom_list_entries", "atom_list_iterations", "pruned_list_entries", "pruned_list_iterations")   # stats [14], [15], [17], [18]


@pytest.fixture(scope="module")
def Engine():
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


@pytest.fixture(scope="module")
def s23k():
    return systems.s23k(mobile_atoms=275, frozen=True)


def _create(Engine, monkeypatch, switch, s, data, v):
    if switch is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, switch)
    g = Engine(s, data); g.set_velocities(v)
    monkeypatch.delenv(SWITCH, raising=False)
    return g


def _counts(g):
    return int(g.get_global("group_list_superset_served")), int(g.get_global("group_list_superset_fallback"))


def _hot(nsteps=200):
    return integrators.generateNCMCIntegrator(nstepsNC=nsteps, dt=0.004, temperature=450.0, seed=11).to_data(precision=0)


def test_same_lists_bit_for_bit(Engine, s23k, tune, monkeypatch):
    """Full scan, superset with D = 300 pm, and D = 20 pm: the same lists after the first build (longest group list, entries and
    64-entry iterations of the full and the pruned atoms' lists, forces bitwise) and the same trajectory, work trace and build count
    over 150 steps of the hot chain.  The counts say which path the rebuilds took."""
    s, v = s23k
    tune(assume_batch=1024)
    engs = [_create(Engine, monkeypatch, sw, s, _hot(), 1.5 * v) for sw in ("0", None, "20")]
    forces = [g.get_forces() for g in engs]          # (the first evaluation builds every list)
    stats = [g.stats() for g in engs]
    print("after the first build:", [[st[k] for k in ("max_jcount",) + LIST_STATS] for st in stats], [_counts(g) for g in engs])
    assert stats[0]["nonbonded_kernel"] == 2 and stats[0]["pruned_lists"] == 1 and stats[0]["tiles_per_list"] == 5
    assert stats[0]["atom_list_entries"] > 100000
    for f, st in zip(forces[1:], stats[1:]):
        for k in ("max_jcount",) + LIST_STATS:
            assert st[k] == stats[0][k], (k, st[k], stats[0][k])
        assert np.array_equal(f, forces[0])
    works = [g.run_switch(150, trace=True) for g in engs]
    x0, v0, b0 = engs[0].get_positions(), engs[0].get_velocities(), engs[0].stats()["list_builds"]
    counts = [_counts(g) for g in engs]
    print("list builds:", [g.stats()["list_builds"] for g in engs], "served / fell back:", counts)
    assert b0 >= 5
    for g, w in zip(engs[1:], works[1:]):
        assert np.array_equal(g.get_positions(), x0) and np.array_equal(g.get_velocities(), v0)
        assert np.array_equal(w, works[0])
        assert g.stats()["list_builds"] == b0
        for k in ("max_jcount",) + LIST_STATS:
            assert g.stats()[k] == engs[0].stats()[k], k
    assert counts[0] == (0, 0)                                   # switch off: nothing is counted
    assert counts[1][0] + counts[1][1] == b0 and counts[1][0] >= 1 and counts[1][1] >= 1         # 300 pm: derived by the first build, then served
    assert counts[2][0] + counts[2][1] == b0 and counts[2][0] >= 1 and counts[2][1] >= 2         # 20 pm: served, and left behind at least once
    for g in engs:
        g.close()


@pytest.mark.parametrize("switch", [None, "20"])
def test_audit_finds_no_missing_pair(Engine, s23k, tune, monkeypatch, switch):
    """blues_audit_lists: right after the first build and at every step of several list lives."""
    s, v = s23k
    tune(assume_batch=1024)
    g = _create(Engine, monkeypatch, switch, s, _hot(), 1.5 * v)
    g.get_forces()
    found, missing = g.audit_lists()
    assert found > 50000 and missing == 0, (found, missing)
    for step in range(60):
        g.step(1)
        found, missing = g.audit_lists()
        assert found > 50000 and missing == 0, (step, found, missing)
    served, fell = _counts(g)
    assert served + fell == g.stats()["list_builds"] >= 2, (g.stats(), served, fell)
    assert served >= 1 or switch == "20"          # (at 20 pm these 60 steps may leave the superset behind at every rebuild)
    g.close()


def test_replaced_positions_invalidate_the_superset(Engine, s23k, tune, monkeypatch):
    """A frozen water next to the mobile region is displaced by 0.3 nm through set_positions after some served rebuilds: the rebuild
    that follows trusts nothing kept (the fallback count rises by one, the served count stays) and the forces equal, bit for bit,
    those of an engine that scans all atoms at every rebuild and was given the same upload; so do the 40 steps after it.  That water
    sits deep inside the kept superset and the scan reads positions live, so for this upload the COUNT is what would notice a missing
    invalidation.  The second upload is the one whose forces would: a frozen water from far outside every superset (> 3.5 nm from the
    ligand) is put where the first one was -- a rebuild served from what was kept would leave it out of the lists."""
    s, v = s23k
    tune(assume_batch=1024)
    ga, gb = [_create(Engine, monkeypatch, sw, s, _hot(), 1.5 * v) for sw in (None, "0")]
    for g in (ga, gb):
        g.step(60)
    served, fell = _counts(ga)
    assert served >= 1 and fell >= 1, (served, fell)
    x = ga.get_positions()
    assert np.array_equal(x, gb.get_positions())
    lig = np.asarray(s.alchemical_atoms)
    d = systems.min_image(x - x[lig].mean(0), s.box)
    r2 = (d * d).sum(1)
    r2[s.mass != 0.0] = np.inf
    near = int(np.argmin(r2))                                     # the frozen atom closest to the ligand; its whole molecule moves
    mol = np.nonzero(s.residue_of_atom == s.residue_of_atom[near])[0]
    assert np.all(s.mass[mol] == 0.0) and r2[near] < 1.5 ** 2
    x[mol, 0] += 0.3
    fs = []
    for g in (ga, gb):
        g.set_positions(x)
        fs.append(g.get_forces())
    served1, fell1 = _counts(ga)
    assert fell1 == fell + 1 and served1 in (served, served + 1), (served1, fell1, served, fell)   # (+1: a rebuild that was due before the upload)
    assert np.array_equal(fs[0], fs[1])
    for g in (ga, gb):
        g.step(40)
    assert np.array_equal(ga.get_positions(), gb.get_positions()) and np.array_equal(ga.get_velocities(), gb.get_velocities())
    assert ga.stats()["list_builds"] == gb.stats()["list_builds"]
    served2, fell2 = _counts(ga)
    assert served2 > served1
    # ---- a frozen water from outside every superset into the place the first one left (rigid translation, same kind of molecule)
    x2 = ga.get_positions()
    far_mol = None
    for far in np.argsort(-np.where(np.isfinite(r2), r2, -1.0)):
        m2 = np.nonzero(s.residue_of_atom == s.residue_of_atom[int(far)])[0]
        if len(m2) == len(mol) and np.all(s.mass[m2] == 0.0):
            far_mol = m2
            break
    assert far_mol is not None and r2[far_mol].min() > 3.5 ** 2, r2[far_mol]
    x2[far_mol] += (x[mol[0]] - np.array([0.3, 0.0, 0.0])) - x2[far_mol[0]]
    fs = []
    for g in (ga, gb):
        g.set_positions(x2)
        fs.append(g.get_forces())
    served3, fell3 = _counts(ga)
    assert fell3 == fell2 + 1 and served3 in (served2, served2 + 1), (served3, fell3, served2, fell2)
    assert np.array_equal(fs[0], fs[1])
    found, missing = ga.audit_lists()
    assert found > 50000 and missing == 0, (found, missing)
    ga.close(); gb.close()


def test_a_new_layout_invalidates_the_superset(Engine, s23k, tune, monkeypatch):
    """A re-sort forced from Python: set_box with a minimally changed box (one part in 10^6) lays the chain out again at once -- new
    sorted indices, new image, zero-filled fJ and superset headers.  After some served rebuilds, on the default engine and on one
    that scans all atoms at every rebuild: the rebuild that follows falls back (the fallback count rises by one, the served count
    does not move), the forces are equal bit for bit, the lists are complete, and so are positions and velocities 40 steps on,
    with rebuilds served from the newly derived superset."""
    s, v = s23k
    tune(assume_batch=1024)
    ga, gb = [_create(Engine, monkeypatch, sw, s, _hot(), 1.5 * v) for sw in (None, "0")]
    for g in (ga, gb):
        g.step(60)
    served, fell = _counts(ga)
    assert served >= 1 and fell >= 1, (served, fell)
    box = np.diag(ga.get_box()) * (1.0 + 1e-6)
    fs = []
    for g in (ga, gb):
        g.set_box(box)
        fs.append(g.get_forces())
    assert _counts(ga) == (served, fell + 1), (_counts(ga), served, fell)
    assert np.array_equal(fs[0], fs[1])
    found, missing = ga.audit_lists()
    assert found > 50000 and missing == 0, (found, missing)
    for g in (ga, gb):
        g.step(40)
    assert np.array_equal(ga.get_positions(), gb.get_positions()) and np.array_equal(ga.get_velocities(), gb.get_velocities())
    assert ga.stats()["list_builds"] == gb.stats()["list_builds"]
    found, missing = ga.audit_lists()
    assert found > 50000 and missing == 0, (found, missing)
    assert _counts(ga)[0] > served
    ga.close(); gb.close()


def test_batch_member_equals_the_lone_chain(Engine, s23k, tune, monkeypatch):
    """A batch of 8 laid out as members of 1024 (the batched builder, k_build_lists_b, superset on): members 0 and 7 equal the same
    chains advanced alone, bit for bit, over 100 steps.  Seeds and velocities as in test_full_size_batch_of_eight."""
    from blues_amd.engine import NativeBatch
    s, v = s23k
    R, n = 8, 100
    tune(assume_batch=1024)

    def make(r):
        d = integrators.generateNCMCIntegrator(nstepsNC=n, dt=0.004, temperature=300.0, seed=100 + r).to_data(precision=0, replica=r)
        return _create(Engine, monkeypatch, None, s, d, v * (1.0 + 0.03 * r))
    solo = {r: make(r) for r in (0, R - 1)}
    ws = {r: g.run_switch(n, trace=True) for r, g in solo.items()}
    bat = [make(r) for r in range(R)]
    B = NativeBatch(bat)
    _, wb = B.step(n, trace=True)
    assert B.stats()["fallback_steps"] == 0
    for r, g in solo.items():
        assert np.array_equal(wb[r], ws[r]), (r, np.abs(wb[r] - ws[r]).max())
        assert np.array_equal(g.get_positions(), bat[r].get_positions()) and np.array_equal(g.get_velocities(), bat[r].get_velocities())
        assert g.stats()["list_builds"] == bat[r].stats()["list_builds"] >= 2
        assert _counts(bat[r]) == _counts(g) and _counts(g)[0] >= 1, (_counts(bat[r]), _counts(g))
    B.close()
    for g in list(solo.values()) + bat:
        g.close()


def test_tile_kernel_in_double_precision(Engine, tol_box, monkeypatch):
    """The other caller of the body: the 975-atom toluene box in double precision (tile kernel with exclusion masks, lone engine),
    60 steps, full scan against the default.  Every atom of this box is mobile, so every non-alchemical atom belongs to a superset
    unconditionally and it would hold more than half of the atoms: the design marks it "never valid", the list keeps the scan of all atoms for
    good, and the fallback count equals the build count."""
    s, v = tol_box
    data = integrators.generateNCMCIntegrator(nstepsNC=60, dt=0.004, temperature=300.0, seed=3).to_data(precision=1)
    ga, gb = [_create(Engine, monkeypatch, sw, s, data, v) for sw in ("0", None)]
    wa, wb = ga.run_switch(60, trace=True), gb.run_switch(60, trace=True)
    assert np.array_equal(wa, wb)
    assert np.array_equal(ga.get_positions(), gb.get_positions()) and np.array_equal(ga.get_velocities(), gb.get_velocities())
    builds = gb.stats()["list_builds"]
    assert builds == ga.stats()["list_builds"] >= 1
    assert _counts(gb) == (0, builds), (_counts(gb), builds)
    ga.close(); gb.close()
