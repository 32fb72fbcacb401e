"""CPU suite: the inputs and the reference of tests/test_gpu_alch_regions.py at the shapes it uses -- the regions of tests/alch_regions.py
(sizes, order, the padded sizes they reach), the System with synthetic exceptions (every exception an exclusion, more than 256 row
entries, and what the added pairs contribute, by a plain numpy sum), and the oracle at those regions: E(1, 1) does not depend on the region,
and the forces of the 64-atom region are the gradient of its energy."""
import numpy as np
import pytest
from scipy.special import erfc

import alch_regions as ar
from blues_amd import integrators

ONE_4PI_EPS0 = 138.935456


def _data():
    return integrators.generateNCMCIntegrator(nstepsNC=10, dt=0.002, temperature=300.0).to_data()


def test_regions_sizes_order_and_padded_sizes(tol_box):
    s, _ = tol_box
    lig = ar.ligand(s)
    assert len(lig) == 15 and len(ar.waters(s)) == 320
    for make in (ar.compact, ar.scattered):
        for n in ar.SIZES:
            r = make(s, n)
            assert len(r) == n and np.all(np.diff(r) > 0) and r.min() >= 0 and r.max() < s.n_atoms
    assert {ar.padded(n) for n in ar.SIZES} == {1, 2, 4, 8, 16, 32, 64}
    for n in ar.SIZES:
        r = ar.compact(s, n)
        assert np.array_equal(r[:min(n, 15)], lig[:min(n, 15)])      # the ligand first ...
        res = np.asarray(s.residue_of_atom)[r[15:]]
        assert sum((res == q).sum() != 3 for q in np.unique(res)) <= 1      # ... then whole waters, only the last taken may be cut
    # 16, 17 and 64 end inside a water (a partially alchemical rigid molecule), 33 and 63 do not
    for n, cut in ((16, True), (17, True), (64, True), (33, False), (63, False)):
        res = np.asarray(s.residue_of_atom)[ar.compact(s, n)[15:]]
        assert any((res == q).sum() != 3 for q in np.unique(res)) == cut
    assert not np.isin(ar.scattered(s, 64), lig).any() and ar.extent(s, ar.scattered(s, 64)) > 1.0 > ar.extent(s, ar.compact(s, 64))
    w = ar.waters_only(s, 5)
    assert len(w) == 15 and not np.isin(w, lig).any() and len(np.unique(np.asarray(s.residue_of_atom)[w])) == 5
    assert np.array_equal(ar.compact(s, 30)[15:], w)


def test_synthetic_exceptions_are_exclusions_and_cross_256_entries(tol_box):
    s, _ = tol_box
    r = ar.compact(s, 64)
    assert ar.exception_row_entries(s, r) == 54      # toluene's 27 exceptions, both atoms in the region
    for n_pairs, n_env, want in ((150, 0, 354), (101, 0, 256), (101, 1, 257)):
        s2, count, pairs = ar.with_synthetic_exceptions(s, r, n_pairs, 1, n_env)
        assert count == want and len(pairs) == n_pairs + n_env and len(np.unique(pairs, axis=0)) == len(pairs)
        excl = set((int(min(a, b)), int(max(a, b))) for a, b in np.asarray(s2.exclusions).reshape(-1, 2))
        exc = [(int(min(a, b)), int(max(a, b))) for a, b in np.asarray(s2.exception_atoms).reshape(-1, 2)]
        assert len(set(exc)) == len(exc) == 27 + len(pairs) and set(exc) <= excl
        assert len(s2.exception_params) == len(s2.exception_atoms) and np.array_equal(np.asarray(s2.alchemical_atoms), r)
        inside = np.isin(pairs, r)
        assert inside[:n_pairs].all() and (inside[n_pairs:].sum(1) == 1).all()
    assert len(s.exception_atoms) == 27      # the fixture's System was not touched
    # another seed: another draw
    assert not np.array_equal(ar.with_synthetic_exceptions(s, r, 150, 2)[2], ar.with_synthetic_exceptions(s, r, 150, 1)[2])


@pytest.mark.parametrize("n_env", [0, 1])
def test_oracle_takes_the_synthetic_exceptions_as_a_numpy_sum_says(oracle_mod, tol_box, n_env):
    """At lambda = (1, 1) an added pair contributes its exception (unscaled Lennard-Jones + bare Coulomb, no cutoff) and loses its regular
    direct-space term (inside the cutoff): E_synthetic - E_plain against that sum over the added pairs, to 1e-9 of the sum of |terms|."""
    s, _ = tol_box
    r = ar.compact(s, 64)
    s2, _, pairs = ar.with_synthetic_exceptions(s, r, 150, 1, n_env)
    e_plain = oracle_mod.Oracle(ar.with_region(s, r), _data()).energy_forces(1.0, 1.0, forces=False)[0]
    e_syn = oracle_mod.Oracle(s2, _data()).energy_forces(1.0, 1.0, forces=False)[0]
    x, q, sg, ep = s.positions, s.charge, s.sigma, s.epsilon
    d = x[pairs[:, 0]] - x[pairs[:, 1]]
    d -= s.box * np.round(d / s.box)
    rr = np.sqrt((d * d).sum(1))
    par = np.asarray(s2.exception_params)[27:]
    lj = lambda sig, eps: 4.0 * eps * ((sig / rr) ** 12 - (sig / rr) ** 6)
    added = lj(par[:, 1], par[:, 2]) + ONE_4PI_EPS0 * par[:, 0] / rr
    sig, eps, qq = 0.5 * (sg[pairs[:, 0]] + sg[pairs[:, 1]]), np.sqrt(ep[pairs[:, 0]] * ep[pairs[:, 1]]), q[pairs[:, 0]] * q[pairs[:, 1]]
    regular = np.where(rr < s.cutoff, lj(sig, eps) + ONE_4PI_EPS0 * qq * erfc(s.ewald_alpha * rr) / rr, 0.0)
    assert (rr < s.cutoff).sum() > 100 and rr.min() > 0.2      # (no clash geometry)
    want = (added - regular).sum()
    scale = np.abs(added).sum() + np.abs(regular).sum()
    print("synthetic exceptions: oracle %.10f, numpy %.10f, sum |terms| %.4f" % (e_syn - e_plain, want, scale))
    assert abs(want) > 1.0 and abs((e_syn - e_plain) - want) <= 1e-9 * scale


def test_oracle_energy_at_lambda_one_does_not_depend_on_the_region(oracle_mod, tol_box):
    s, _ = tol_box
    e0 = oracle_mod.Oracle(s, _data()).energy_forces(1.0, 1.0, forces=False)[0]
    for make in (ar.compact, ar.scattered):
        for n in ar.SIZES:
            o = oracle_mod.Oracle(ar.with_region(s, make(s, n)), _data())
            e1 = o.energy_forces(1.0, 1.0, forces=False)[0]
            assert abs(e1 - e0) <= 1e-12 * abs(e0), (make.__name__, n, e1, e0)
            assert abs(o.energy_forces(0.5, 0.3, forces=False)[0] - e0) > 0.1      # (and the region does something away from (1, 1))


def test_oracle_forces_are_the_gradient_at_the_64_atom_region(oracle_mod, tol_box):
    """Central differences (h = 1e-5 nm) at lambda = (0.45, 0.2): three (atom, component) picks inside the region and three outside,
    seeded.  Bar as tests/test_oracle_golden.py::test_forces_are_energy_gradient and tests/test_gpu_symmetry.py::
    test_forces_are_the_energy_gradient, which do the same for the existing regions: rel 2e-5, abs 2e-3."""
    s, _ = tol_box
    r = ar.compact(s, 64)
    o = oracle_mod.Oracle(ar.with_region(s, r), _data())
    ls, le = 0.45, 0.2
    x0 = np.array(s.positions, dtype=np.float64)
    f = o.energy_forces(ls, le)[1]
    rng = np.random.RandomState(5)
    outside = np.setdiff1d(np.arange(s.n_atoms), r)
    h = 1e-5
    for i in list(rng.choice(r, 3, replace=False)) + list(rng.choice(outside, 3, replace=False)):
        k = rng.randint(3)
        xp = x0.copy(); xp[i, k] += h; o.set_positions(xp); ep = o.energy_forces(ls, le, forces=False)[0]
        xm = x0.copy(); xm[i, k] -= h; o.set_positions(xm); em = o.energy_forces(ls, le, forces=False)[0]
        assert f[i, k] == pytest.approx(-(ep - em) / (2 * h), rel=2e-5, abs=2e-3), (int(i), k)


def test_the_long_list_region_of_the_dense_forms():
    """tests/test_gpu_alch_regions.py: DENSE_LONG_LIST is what longest_list_waters finds on S23k (five mobile waters, extent < 0.86 nm, list
    at cutoff + 0.2 nm; the full search of 60,000 draws takes a minute and is not repeated here: a short one must not beat it), with the
    counts the GPU test's docstring states."""
    from blues_amd import systems
    from test_gpu_alch_regions import DENSE_LONG_LIST, LONG_LIST_SKIN
    s, _ = systems.s23k(mobile_atoms=275, frozen=True)
    region = np.sort(np.concatenate([np.arange(o, o + 3) for o in DENSE_LONG_LIST]))
    mob = np.nonzero(s.mass > 0)[0]
    assert np.isin(region, mob).all() and np.isin(region, ar.waters(s)).all()
    assert abs(ar.extent(s, region) - 0.8543) < 1e-4 and 0.5 * s.box.min() > s.cutoff + ar.extent(s, region) + 0.3
    assert ar.list_count(s, region, s.cutoff + 0.2) == 1849 and ar.list_count(s, region, s.cutoff + LONG_LIST_SKIN) == 3107
    oxygens, count = ar.longest_list_waters(s, 5, mob, 0.86, s.cutoff + 0.2, seed=0, draws=2000)
    assert oxygens is not None and count <= 1849
