"""Coulomb-only walk of the benchmark's nonbonded kernel (kernels_nb.h: nonbonded_atom_body) on a real MI355X.

An i-atom without epsilon (a water's hydrogen: 174 of the 261 i-slots here) has a 12-6 term of exactly +-0 with every entry of its
list.  Its wave takes a walk without the Lennard-Jones chain -- and, where it does not prune, without the read of the entry's
{sigma/2, 2 sqrt(eps)} record -- and must store THE SAME BITS: fma(q_i q_j, g, +-0) rounds to the plain product whenever that is
not zero, and a zero of either sign adds the same to a partial sum that starts at +0.  The smallest set-up in which an engine runs
this kernel with pruned lists: one S23k chain with 275 mobile atoms, frozen, mixed precision, laid out as a member of a batch of 512.
The switch is the environment variable read when an engine is created, BLUES_NB_COULOMB_WALK (blues_amd/engine.py): 0 = every atom
takes the full walk (the kernel as it was), unset or 1 = atoms without epsilon take the Coulomb-only walk.
Reference behaviour being reproduced: the NonbondedForce evaluation behind CustomIntegrator's `f`
(reference blues/integrators.py:159-231)."""
import copy

import numpy as np
import pytest

from blues_amd import build, integrators, systems

pytestmark = pytest.mark.gpu

SWITCH = "BLUES_NB_COULOMB_WALK"


@pytest.fixture(scope="module")
def Engine():
    build.build_engine()
    from blues_amd.engine import NativeEngine
    return NativeEngine


@pytest.fixture(scope="module")
def s23k():
    return systems.s23k(mobile_atoms=275, frozen=True)


def _create(Engine, monkeypatch, switch, s, data, v):
    monkeypatch.setenv(SWITCH, switch)
    g = Engine(s, data); g.set_velocities(v)
    monkeypatch.delenv(SWITCH, raising=False)
    st = g.stats()
    assert st["nonbonded_kernel"] == 2 and st["pruned_lists"] == 1, st
    return g


def _hot(n=200):
    """the hot chain of test_list_audit_no_pair_in_range_is_ever_missing: 450 K, to be started with 1.5 x the velocities"""
    return integrators.generateNCMCIntegrator(nstepsNC=n, dt=0.004, temperature=450.0, seed=11).to_data(precision=0)


def _waters(s):
    """(hydrogens, oxygens) of the System's waters: the atoms without epsilon outside the ligand, and their residues' other atom"""
    alch = np.zeros(s.n_atoms, bool); alch[np.asarray(s.alchemical_atoms)] = True
    hyd = np.nonzero((np.asarray(s.epsilon) == 0.0) & ~alch)[0]
    res = np.asarray(s.residue_of_atom)
    oxy = np.nonzero(np.isin(res, res[hyd]) & (np.asarray(s.epsilon) != 0.0) & ~alch)[0]
    assert len(hyd) == 2 * len(oxy) > 0
    return hyd, oxy


def test_same_bits_at_rest_and_in_motion(Engine, s23k, tune, monkeypatch):
    """Switch on against switch off: forces at two lambda states, then positions, velocities and protocol work at steps 1, 37 and 80 of
    the hot chain -- prunes in most passes, more than one rebuild, so both kinds of walk ran pruning and not pruning."""
    s, v = s23k
    tune(assume_batch=512)
    on, off = (_create(Engine, monkeypatch, sw, s, _hot(), 1.5 * v) for sw in ("1", "0"))
    assert int(on.get_global("nb_coulomb_walk_atoms")) == 174 and int(off.get_global("nb_coulomb_walk_atoms")) == 0
    for ls, le in ((1.0, 1.0), (0.4, 0.2)):
        for g in (on, off):
            g.set_global("lambda_sterics", ls); g.set_global("lambda_electrostatics", le)
        f_on, f_off = on.get_forces(), off.get_forces()
        assert np.isfinite(f_on).all() and np.abs(f_on).max() > 0.0
        assert np.array_equal(f_on, f_off), (ls, le, np.abs(f_on - f_off).max())
    done = 0
    for upto in (1, 37, 80):
        for g in (on, off):
            g.step(upto - done)
        done = upto
        assert np.array_equal(on.get_positions(), off.get_positions()), upto
        assert np.array_equal(on.get_velocities(), off.get_velocities()), upto
        assert on.get_global("protocol_work") == off.get_global("protocol_work"), upto
    st_on, st_off = on.stats(), off.stats()
    print("atom_prunes", st_on["atom_prunes"], st_off["atom_prunes"], "list_builds", st_on["list_builds"], st_off["list_builds"])
    assert st_on["atom_prunes"] == st_off["atom_prunes"] > 0
    assert st_on["list_builds"] == st_off["list_builds"] > 1
    on.close(); off.close()


def _variants(s):
    hyd, oxy = _waters(s)
    a = copy.copy(s); a.epsilon = np.array(s.epsilon, dtype=np.float64, copy=True); a.epsilon[hyd] = 1e-3      # kJ/mol, at the hydrogens' sigma of 0.1 nm
    b = copy.copy(s); b.epsilon = np.array(s.epsilon, dtype=np.float64, copy=True); b.epsilon[oxy] = 0.0
    mobile_oxy = [int(o) for o in oxy if s.mass[o] > 0.0]
    res = np.asarray(s.residue_of_atom)
    dead = np.nonzero(res == res[mobile_oxy[4]])[0]
    assert len(dead) == 3
    c = copy.copy(s); c.epsilon = np.array(s.epsilon, dtype=np.float64, copy=True); c.charge = np.array(s.charge, dtype=np.float64, copy=True)
    c.epsilon[dead] = 0.0; c.charge[dead] = 0.0
    return {"hydrogens_with_epsilon": (a, 0, None), "oxygens_without_epsilon": (b, 261, None), "one_water_without_charge_or_epsilon": (c, 175, dead)}


@pytest.mark.parametrize("which", ["hydrogens_with_epsilon", "oxygens_without_epsilon", "one_water_without_charge_or_epsilon"])
def test_the_branch_follows_epsilon_not_the_element(Engine, oracle_mod, s23k, tune, monkeypatch, which):
    """The decision is the i-atom's own 2 sqrt(eps) == 0, whatever the atom is: hydrogens that have an epsilon take the full walk, oxygens
    without one the Coulomb-only walk, and a water with neither charge nor epsilon feels exactly nothing on either.  Forces on / off
    bitwise, and within the standing 1e-5 of the largest oracle force."""
    s0, v = s23k
    s, n_walk, dead = _variants(s0)[which]
    tune(assume_batch=512)
    data = integrators.generateNCMCIntegrator(nstepsNC=20, dt=0.004, temperature=300.0, seed=7).to_data(precision=0)
    on, off = (_create(Engine, monkeypatch, sw, s, data, v) for sw in ("1", "0"))
    assert int(on.get_global("nb_coulomb_walk_atoms")) == n_walk and int(off.get_global("nb_coulomb_walk_atoms")) == 0
    f_on, f_off = on.get_forces(), off.get_forces()
    assert np.isfinite(f_on).all() and np.isfinite(f_off).all()
    assert np.array_equal(f_on, f_off), np.abs(f_on - f_off).max()
    fo = oracle_mod.Oracle(s, data).energy_forces(1.0, 1.0)[1]
    mob = np.nonzero(np.asarray(s.mass) > 0)[0]
    err = np.abs(f_on[mob] - fo[mob]).max() / np.abs(fo[mob]).max()
    print(which, "force error / largest oracle force: %.3g" % err)
    assert err <= 1e-5, err
    if dead is not None:   # (a rigid water: no bonded term, so its whole force is the nonbonded one)
        assert np.all(f_on[dead] == 0.0) and np.all(f_off[dead] == 0.0), (f_on[dead], f_off[dead])
    on.close(); off.close()


def test_list_audit_still_finds_nothing_missing(Engine, s23k, tune, monkeypatch):
    """The pruning Coulomb-only walk writes the pruned lists of two atoms in three: blues_audit_lists at every step of the hot chain."""
    s, v = s23k
    tune(assume_batch=512)
    g = _create(Engine, monkeypatch, "1", s, _hot(), 1.5 * v)
    assert int(g.get_global("nb_coulomb_walk_atoms")) == 174
    for step in range(40):
        g.step(1)
        found, missing = g.audit_lists()
        assert found > 50000 and missing == 0, (step, found, missing)
    assert g.stats()["atom_prunes"] > 0, g.stats()
    g.close()


def test_batch_members_equal_their_lone_chains(Engine, s23k, tune, monkeypatch):
    """Four members advanced 40 steps through NativeBatch (k_nonbonded_atom_b) equal four lone engines (k_nonbonded_atom) bit for bit,
    switch on.  The construction of test_full_size_batch_of_eight, smaller."""
    from blues_amd.engine import NativeBatch
    s, v = s23k
    R, n = 4, 40
    tune(assume_batch=512)

    def make():
        return [_create(Engine, monkeypatch, "1", s, integrators.generateNCMCIntegrator(nstepsNC=n, dt=0.004, temperature=300.0, seed=100 + r).to_data(precision=0, replica=r),
                        v * (1.0 + 0.03 * r)) for r in range(R)]
    solo = make()
    ws = [g.run_switch(n, trace=True) for g in solo]
    bat = make()
    B = NativeBatch(bat)
    _, wb = B.step(n, trace=True)
    assert B.stats()["fallback_steps"] == 0
    for r in range(R):
        assert int(bat[r].get_global("nb_coulomb_walk_atoms")) == 174
        assert np.array_equal(wb[r], ws[r]), (r, np.abs(wb[r] - ws[r]).max())
        assert np.array_equal(solo[r].get_positions(), bat[r].get_positions()) and np.array_equal(solo[r].get_velocities(), bat[r].get_velocities())
        assert solo[r].stats()["atom_prunes"] == bat[r].stats()["atom_prunes"] > 0
    assert len({w[-1] for w in ws}) == R
    B.close()
    for g in solo + bat:
        g.close()
