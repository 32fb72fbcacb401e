"""CPU suite for the mesh-shape cases of tests/pme_cases.py: the oracle's mesh on anisotropic, odd and mixed-parity meshes against the
exact Ewald sum, the host-side model of the mesh kernel's path on every row of the table, and the oracle's forces as the gradient of its
energy on every row (the GPU suite, tests/test_gpu_pme_shapes.py, compares the engine with this oracle)."""
import numpy as np
import pytest

import pme_cases as pc
from blues_amd import integrators, systems


def _integ():
    return integrators.generateNCMCIntegrator(nstepsNC=10).to_data()


def test_mesh_converges_to_the_exact_ewald_sum_on_anisotropic_meshes(oracle_mod):
    """The toluene box tiled (1, 1, 2): 2.18 x 2.18 x 4.36 nm, 1,950 atoms.  Odd and mixed-parity meshes of three resolutions against
    ewald_reciprocal_exact(14), an answer the mesh code did not produce.  Bounds: order-5 splines converge as h^5 until rounding of the
    exact sum's own truncation shows (measured 7.5e-3, 1.25e-5, 1.6e-6)."""
    s, _ = systems.toluene_box()
    t = systems.tile_system(s, (1, 1, 2))
    assert t.n_atoms == 1950 and np.allclose(t.box, [2.1786, 2.1786, 4.3572], atol=1e-3)
    exact, errs = None, []
    for mesh in ((9, 11, 19), (18, 21, 37), (36, 43, 75)):
        r = systems.with_reciprocal_space(t); r.pme_grid = mesh
        o = oracle_mod.Oracle(r, _integ(), openmp=True)
        if exact is None:
            exact = o.ewald_reciprocal_exact(14)
        errs.append(abs(pc.mesh_energy_of(r, o) - exact) / abs(exact))
    print("relative errors of the mesh energy:", errs)
    assert errs[0] < 2e-2 and errs[1] < 1e-4 and errs[2] < 1e-5, errs
    assert errs[0] > errs[1] > errs[2], errs


def test_expected_path_on_the_rows_of_the_table():
    """The model must give the path and the kind of block each row was chosen for: this keeps the GPU suite from drifting onto one path."""
    fast_partial, kinds, wrapped = 0, set(), np.zeros(3, bool)
    one_full = {0: np.zeros(3, bool), 1: np.zeros(3, bool), 2: np.zeros(3, bool)}      # full axis -> axes a fast block of that class wraps on
    for c in pc.CASES:
        s = pc.build(c)
        path, L = pc.expected_path(s)
        assert int((s.mass != 0.0).sum()) == c.mobile, (c.id, int((s.mass != 0.0).sum()))
        assert path == c.kind, (c.id, path, L)
        if c.block is not None:
            assert pc.block_class(s, L) == c.block, (c.id, L)
        kinds.add(path)
        if path == "fast" and pc.block_class(s, L) == "partial":
            fast_partial += 1
            wrapped |= np.array(pc.wraps(s))
        if path == "fast" and pc.block_class(s, L) == "one-full":
            d = [L[k] >= s.pme_grid[k] for k in range(3)].index(True)
            assert pc.expected_block(s)[1][d] == 0
            one_full[d] |= np.array(pc.wraps(s))
    assert fast_partial >= 8
    # a block on the pruned pipeline that is the whole mesh along ONE axis only, for each axis, with both other axes wrapping somewhere
    for d in range(3):
        assert [bool(w) for w in one_full[d]] == [k != d for k in range(3)], (d, one_full[d])
    assert wrapped.all()                                  # a fast partial block runs through the periodic edge on each axis somewhere
    assert {"fast", "general:host", "general:atoms", "general:block"} <= kinds
    # shifts that should wrap exactly one axis do
    for mesh in ("20x18x27", "18x20x32", "27x20x18", "24x24x30"):
        assert pc.wraps(pc.build(pc.BY_ID[mesh + "-45-corner"])) == (True, True, True)
        assert pc.wraps(pc.build(pc.BY_ID[mesh + "-45-xface"])) == (True, False, False)
        assert pc.wraps(pc.build(pc.BY_ID[mesh + "-45-yface"])) == (False, True, False)
        assert pc.wraps(pc.build(pc.BY_ID[mesh + "-45-zface"])) == (False, False, True)
        assert pc.wraps(pc.build(pc.BY_ID[mesh + "-45-centre"])) == (False, False, False)
    # the long-axis rows: full on two axes, partial on the long one only
    assert pc.expected_path(pc.build(pc.BY_ID["6x7x64-150"]))[1][:2] == (6, 7) and pc.expected_path(pc.build(pc.BY_ID["6x7x64-150"]))[1][2] < 64
    assert pc.expected_path(pc.build(pc.BY_ID["64x7x6-150"]))[1][1:] == (7, 6) and pc.expected_path(pc.build(pc.BY_ID["64x7x6-150"]))[1][0] < 64


def test_model_of_the_special_cases():
    """The cases the GPU suite builds beside the table land where it needs them."""
    s = pc.build(pc.BY_ID["20x18x27-45"])
    lig_only = pc.mobile_nearest(s, 15)
    assert pc.expected_path(lig_only) == ("fast", (1, 1, 1))                       # no charged mobile atom: the empty block
    path, L = pc.expected_path(lig_only, full_charges=True)                        # the qn_full launch of the same engine: a real block
    assert path == "fast" and min(L) > 5 and pc.block_class(lig_only, L) == "partial"
    u = pc.uncharged_frozen(s)
    assert np.all(u.charge[u.mass == 0.0] == 0.0) and np.array_equal(u.charge[u.mass != 0.0], s.charge[s.mass != 0.0])
    assert pc.expected_path(u) == pc.expected_path(s)
    b = pc.build(pc.BY_ID["24x24x30-45"])
    x = pc.scattered(b)
    assert pc.expected_path(b, x)[0] == "general:block" and pc.expected_path(b)[0] == "fast"
    assert np.allclose(np.sort(x, axis=0), np.sort(b.positions, axis=0), atol=0)   # the same sites, other molecules on them
    for name in ("20x18x27-45-corner", "18x20x32-45-corner"):
        s = pc.build(pc.BY_ID[name])
        K, L = s.pme_grid, np.asarray(s.box).reshape(-1)[:3]
        for ulps in (0, 1, -1):
            r, planted = pc.on_planes(s, ulps)
            assert len({a for a, _, _ in planted}) == len(pc.PLANE_TARGETS)
            assert np.abs(r.positions - s.positions - L * np.round((r.positions - s.positions) / L)).max() < 0.55 * (L / np.asarray(K)).max()
            assert pc.expected_path(r)[0] == "fast"
            for (a, ax, t), name_t in zip(planted, pc.PLANE_TARGETS):
                assert r.positions[a, ax] == t
                u_ = pc.mesh_index(r.positions[a], s.box, K)[1][ax]
                if ulps == 0 and name_t.startswith("plane"):
                    assert u_ == np.floor(u_)
                if ulps == 0 and name_t == "minus_tiny":
                    assert u_ == K[ax]      # (frac(-1e-17 / L) rounds to 1: pme_locate's ti == K branch)
                if ulps == 0 and name_t == "box_edge":
                    assert u_ == 0.0


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_oracle_forces_are_the_gradient_on_every_mesh_and_placement(oracle_mod, case):
    """-dE/dx by central differences for three mobile atoms of the row (a ligand atom, a water's oxygen, a water's hydrogen), at the
    tolerances of tests/test_oracle_pme.py::test_reciprocal_forces_are_the_gradient_and_spare_alchemical_atoms."""
    s = pc.build(case)
    o = oracle_mod.Oracle(s, _integ(), openmp=True)
    e, f, T = o.energy_forces(0.7, 0.4)
    assert abs(T[8]) > 10.0
    mob = np.nonzero(s.mass != 0.0)[0]
    x = np.array(s.positions, dtype=np.float64); h = 1e-5
    for i in (int(mob[3]), int(mob[15]), int(mob[-1])):
        for k in range(3):
            xp = x.copy(); xp[i, k] += h; o.set_positions(xp); ep = o.energy_forces(0.7, 0.4, forces=False)[0]
            xm = x.copy(); xm[i, k] -= h; o.set_positions(xm); em = o.energy_forces(0.7, 0.4, forces=False)[0]
            assert f[i, k] == pytest.approx(-(ep - em) / (2 * h), rel=2e-6, abs=2e-5), (i, k)
