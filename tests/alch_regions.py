"""Alchemical regions of 1 to 64 atoms for the parity tests (tests/test_alch_regions_cpu.py, tests/test_gpu_alch_regions.py).

The engine takes up to 64 alchemical atoms, and the shape of its alchemical kernels follows the region's size padded to a power of two
(PA: lanes per j-slot, widths of the segmented reductions, strides of the partial sums).  The helpers here make regions of any size out
of the Systems the suite already has -- the ligand's atoms first, then whole waters -- so every PA from 1 to 64 and both sides of each
power of two can run.  A region may end inside a rigid water: that is legal (alchemical-environment exclusions and constraints, the path
of test_gpu_parity.py::test_alchemical_subset_of_a_molecule).

Everything is deterministic: index order, stable sorts, and seeded numpy.random.RandomState where something is drawn.
"""
import copy

import numpy as np

SIZES = (1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64)      # every PA from 1 to 64, both sides of each power of two, the dense forms' limit


def padded(n):
    """PA: n padded to a power of two (blues_engine.hip: `PA = 1; while (PA < n_alch) PA <<= 1`)."""
    pa = 1
    while pa < n:
        pa <<= 1
    return pa


def _min_image(d, box):
    box = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    return d - box * np.round(d / box)


def ligand(system):
    return np.sort(np.asarray(system.alchemical_atoms, dtype=np.int64).reshape(-1))


def waters(system):
    """(w, 3) atom indices of the three-atom residues outside the ligand, oxygen first, in index order."""
    res = np.asarray(system.residue_of_atom)
    order = np.argsort(res, kind="stable")
    _, first, count = np.unique(res[order], return_index=True, return_counts=True)
    w = np.stack([order[first[count == 3] + k] for k in range(3)], axis=1).astype(np.int64)
    w = w[~np.isin(w, ligand(system)).any(1)]
    q = np.asarray(system.charge, dtype=np.float64)[w]
    w = np.take_along_axis(w, np.argsort(q, axis=1, kind="stable"), axis=1)      # (the oxygen carries the negative charge)
    return w[np.argsort(w.min(1), kind="stable")]


def _waters_by_distance(system, among=None):
    """Whole waters in order of the oxygen's minimum-image distance to the ligand's centroid (stable; ties in index order)."""
    w = waters(system)
    if among is not None:
        ok = np.zeros(system.n_atoms, bool); ok[np.asarray(among, dtype=np.int64)] = True
        w = w[ok[w].all(1)]
    x = np.asarray(system.positions, dtype=np.float64)
    c = x[ligand(system)].mean(0)
    d = _min_image(x[w[:, 0]] - c, system.box)
    return w[np.argsort((d * d).sum(1), kind="stable")]


def with_region(system, region):
    s = copy.copy(system)
    s.alchemical_atoms = np.asarray(region, dtype=np.int32)
    return s


def compact(system, n):
    """The ligand's atoms in index order for n up to its size; beyond that, whole waters (O, H, H) nearest the ligand's centroid are
    added, the list is cut at n and sorted.  Sizes that are not ligand + 3 k end inside a water."""
    lig = ligand(system)
    atoms = list(lig[:n])
    if n > len(lig):
        for w in _waters_by_distance(system):
            atoms.extend(int(a) for a in w)
            if len(atoms) >= n:
                break
    atoms = np.sort(np.array(atoms[:n], dtype=np.int64))
    assert len(atoms) == n and len(np.unique(atoms)) == n
    return atoms.astype(np.int32)


def scattered(system, n):
    """Waters taken at a fixed stride through the index range, cut at n atoms and sorted: a region spread over the whole box."""
    w = waters(system)
    k = (n + 2) // 3
    stride = max(1, len(w) // k)
    atoms = np.sort(w[::stride][:k].reshape(-1)[:n])
    assert len(atoms) == n
    return atoms.astype(np.int32)


def waters_only(system, k, among=None, skip=0):
    """k whole waters and no ligand: those nearest the ligand's centroid among the atoms `among` (default: all), after `skip` of them."""
    w = _waters_by_distance(system, among)[skip:skip + k]
    assert len(w) == k
    return np.sort(w.reshape(-1)).astype(np.int32)


def exception_row_entries(system, region):
    """Entries of the engine's alchemical exception rows: 2 for an exception with both atoms in the region, 1 for one with one atom in it
    (unless its chargeProd and epsilon are both 0: such a pair has no row entry)."""
    inside = np.zeros(system.n_atoms, bool); inside[np.asarray(region, dtype=np.int64)] = True
    ea = np.asarray(system.exception_atoms, dtype=np.int64).reshape(-1, 2)
    ep = np.asarray(system.exception_params, dtype=np.float64).reshape(-1, 3)
    k = inside[ea[:, 0]].astype(int) + inside[ea[:, 1]].astype(int)
    live = (ep[:, 0] != 0.0) | (ep[:, 2] != 0.0)
    return int(2 * (k == 2).sum() + ((k == 1) & live).sum())


def _exception_of(system, i, j):
    q, sg, ep = np.asarray(system.charge), np.asarray(system.sigma), np.asarray(system.epsilon)
    return (q[i] * q[j] / 1.2, 0.5 * (sg[i] + sg[j]), 0.5 * np.sqrt(ep[i] * ep[j]))


def with_synthetic_exceptions(system, region, n_pairs=150, seed=1, n_env_pairs=0):
    """The System with `region` alchemical and n_pairs more exceptions, each between a ligand atom of the region and an atom of one of the
    region's waters, drawn without repeats from RandomState(seed); every new pair becomes an exclusion and an exception with
    (q_i q_j / 1.2, (sigma_i + sigma_j) / 2, 0.5 sqrt(eps_i eps_j)).  n_env_pairs more pairs join a ligand atom of the region with the
    oxygen of the nearest waters OUTSIDE the region (one row entry each).  Returns (System, exception-row entries, the added pairs)."""
    region = np.asarray(region, dtype=np.int64)
    lig = ligand(system)
    tol = region[np.isin(region, lig)]
    wat = region[~np.isin(region, lig)]
    assert len(tol) and len(wat) and n_pairs <= len(tol) * len(wat)
    rng = np.random.RandomState(seed)
    pick = np.sort(rng.choice(len(tol) * len(wat), n_pairs, replace=False))
    pairs = [(int(tol[p // len(wat)]), int(wat[p % len(wat)])) for p in pick]
    if n_env_pairs:
        outside = np.ones(system.n_atoms, bool); outside[region] = False; outside[lig] = False
        near = _waters_by_distance(system, among=np.nonzero(outside)[0])[:n_env_pairs]
        pairs += [(int(tol[(3 * k) % len(tol)]), int(w[0])) for k, w in enumerate(near)]
    pairs = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    have = set((int(min(a, b)), int(max(a, b))) for a, b in np.asarray(system.exclusions, dtype=np.int64).reshape(-1, 2))
    assert not any((min(a, b), max(a, b)) in have for a, b in pairs)
    s = with_region(system, region)
    s.exclusions = np.concatenate([np.asarray(system.exclusions).reshape(-1, 2), pairs]).astype(np.int32)
    s.exception_atoms = np.concatenate([np.asarray(system.exception_atoms).reshape(-1, 2), pairs]).astype(np.int32)
    s.exception_params = np.concatenate([np.asarray(system.exception_params, dtype=np.float64).reshape(-1, 3),
                                         np.array([_exception_of(system, a, b) for a, b in pairs], dtype=np.float64).reshape(-1, 3)])
    return s, exception_row_entries(s, region), pairs


def list_count(system, region, radius):
    """Atoms outside the region within `radius` (cutoff + skin) of any of its atoms, by the minimum image: the alchemical atoms' j-list as
    the engine builds it, counted on the CPU."""
    x = np.asarray(system.positions, dtype=np.float64)
    region = np.asarray(region, dtype=np.int64)
    near = np.zeros(system.n_atoms, bool)
    for a in region:
        d = _min_image(x - x[a], system.box)
        near |= (d * d).sum(1) <= radius * radius
    near[region] = False
    return int(near.sum())


def longest_list_waters(system, k, among, max_extent, radius, seed=0, draws=60000):
    """The oxygens of the k whole waters among the atoms `among` whose region has the longest list (list_count at `radius`) with an extent
    below max_extent: the best of `draws` seeded draws of k waters (about a minute for 60,000).  Returns (oxygens, list count)."""
    x = np.asarray(system.positions, dtype=np.float64)
    w = _waters_by_distance(system, among)
    near = np.zeros((len(w), system.n_atoms), bool)
    for q, ww in enumerate(w):
        for a in ww:
            d = _min_image(x - x[a], system.box)
            near[q] |= (d * d).sum(1) <= radius * radius
    rng = np.random.RandomState(seed)
    best = (-1, None)
    for _ in range(draws):
        pick = np.sort(rng.choice(len(w), k, replace=False))
        region = np.sort(w[pick].reshape(-1))
        if extent(system, region) < max_extent:
            m = near[pick].any(0); m[region] = False
            if int(m.sum()) > best[0]:
                best = (int(m.sum()), tuple(int(o) for o in np.sort(w[pick][:, 0])))
    return best[1], best[0]


def extent(system, region):
    """Largest minimum-image distance of a region's atom from its first (the `ext` of the host's dense-form precondition)."""
    x = np.asarray(system.positions, dtype=np.float64)
    region = np.asarray(region, dtype=np.int64)
    d = _min_image(x[region] - x[region[0]], system.box)
    return float(np.sqrt((d * d).sum(1)).max())
