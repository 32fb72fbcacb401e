"""Prefilter of the atoms'-list builder (kernels_nb.h: build_atom_lists_body) on a real MI355X.

A wave of the builder first keeps the candidates of its group's list that lie within list radius + reach of the sphere around
its atoms, and the unchanged walk takes that shorter list, in the same order -- so the atoms' lists must come out IDENTICAL to
the direct walk's: same entries, same order, same counts.  The smallest shape at which this kernel exists: one S23k chain with 275
mobile atoms, frozen, mixed precision, laid out as a member of a batch of 1024 (per-atom lists, one group of five tiles).
The switch is the environment variable read when an engine is created, BLUES_ATOM_LIST_PREFILTER (blues_amd/engine.py): 0 = every wave
walks the list directly, unset = the prefilter, N > 0 = waves with a reach above N picometres walk directly (100 pm: about half
of this system's waves, so one launch runs both paths).
Reference behaviour being reproduced: the NonbondedForce evaluation behind CustomIntegrator's `f`
(reference blues/integrators.py:159-231)."""
import numpy as np
import pytest

from blues_amd import build, integrators, systems

pytestmark = pytest.mark.gpu

SWITCH = "BLUES_ATOM_LIST_PREFILTER"
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


def test_same_lists_bit_for_bit(Engine, s23k, tune, monkeypatch):
    """Direct walk, prefilter, and a launch that mixes both: the same lists after a rebuild (entries and 64-entry iterations of
    the full and the pruned lists, forces bitwise), and the same trajectory over 150 steps of the hot chain of
    test_list_audit_no_pair_in_range_is_ever_missing (several rebuilds, many prunes)."""
    s, v = s23k
    tune(assume_batch=1024)
    data = integrators.generateNCMCIntegrator(nstepsNC=200, dt=0.004, temperature=450.0, seed=11).to_data(precision=0)
    engs = [_create(Engine, monkeypatch, sw, s, data, 1.5 * v) for sw in ("0", None, "100")]
    forces = [g.get_forces() for g in engs]          # (the first evaluation builds every list)
    stats = [g.stats() for g in engs]
    print("after the rebuild:", [[st[k] for k in LIST_STATS] for st in stats])
    assert stats[0]["nonbonded_kernel"] == 2 and stats[0]["pruned_lists"] == 1 and stats[0]["tiles_per_list"] == 5
    assert stats[0]["atom_list_entries"] > 100000 and stats[0]["pruned_list_entries"] > 0
    for g, f, st in zip(engs[1:], forces[1:], stats[1:]):
        for k in LIST_STATS:
            assert st[k] == stats[0][k], (k, st[k], stats[0][k])
        assert np.array_equal(f, forces[0])
    for g in engs:
        g.step(150)
    x0, v0, b0 = engs[0].get_positions(), engs[0].get_velocities(), engs[0].stats()["list_builds"]
    print("list builds:", [g.stats()["list_builds"] for g in engs])
    assert b0 >= 5
    for g in engs[1:]:
        assert np.array_equal(g.get_positions(), x0) and np.array_equal(g.get_velocities(), v0)
        assert g.stats()["list_builds"] == b0
        for k in LIST_STATS:
            assert g.stats()[k] == engs[0].stats()[k], k
    for g in engs:
        g.close()


def test_audit_finds_no_missing_pair(Engine, s23k, tune, monkeypatch):
    """blues_audit_lists on the prefiltered engine: right after a rebuild and at every step of several list lives."""
    s, v = s23k
    tune(assume_batch=1024)
    data = integrators.generateNCMCIntegrator(nstepsNC=200, dt=0.004, temperature=450.0, seed=11).to_data(precision=0)
    g = _create(Engine, monkeypatch, None, s, data, 1.5 * v)
    g.get_forces()
    found, missing = g.audit_lists()
    assert found > 50000 and missing == 0, (found, missing)
    for step in range(60):
        g.step(1)
        found, missing = g.audit_lists()
        assert found > 50000 and missing == 0, (step, found, missing)
    assert g.stats()["list_builds"] >= 2 and g.stats()["atom_prunes"] > 0, g.stats()
    g.close()


def test_batch_member_equals_the_lone_chain(Engine, s23k, tune, monkeypatch):
    """A batch of 8 laid out as members of 1024 (the batched builder, k_build_atom_lists_b, prefilter on): members 0 and 7 equal
    the same chains advanced alone, bit for bit, over 100 steps.  Seeds and velocities as in test_full_size_batch_of_eight."""
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
    B.close()
    for g in list(solo.values()) + bat:
        g.close()
