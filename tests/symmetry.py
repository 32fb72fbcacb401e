"""Exact symmetries of the potential as transformations of a SystemData (tests/test_symmetry_cpu.py proves them on the CPU oracle,
tests/test_gpu_symmetry.py holds the HIP engine to them).  Plain numpy; nothing here knows the engine or the oracle.

A transformed System describes the same physics: atoms in another order, term lists in another order and orientation, molecules
moved by lattice vectors of their own, axes exchanged, or (without periodicity) the whole System rotated.  Energies must come out the
same and forces, positions and velocities the same once mapped back.  Every function returns

    (new SystemData, transformed velocities or None, Map)

and the Map takes per-atom vectors and positions of the new System back to the original's order, axes and place.  Maps compose
(`first.then(second)`), so a chain of transformations has one Map.
"""
import dataclasses

import numpy as np

from blues_amd import _abi, systems

_PER_ATOM = ("mass", "charge", "sigma", "epsilon", "positions", "residue_of_atom")
_INDEX_LISTS = ("exclusions", "exception_atoms", "bond_atoms", "angle_atoms", "torsion_atoms", "constraint_atoms", "alchemical_atoms",
                "restraint_atoms")
# (index array, its parameter rows, how a row may be turned round without changing the term)
_TERM_LISTS = (("exclusions", None, "flip"), ("exception_atoms", "exception_params", "flip"), ("bond_atoms", "bond_params", "flip"),
               ("angle_atoms", "angle_params", "reverse"), ("torsion_atoms", "torsion_params", "reverse"),
               ("constraint_atoms", "constraint_dist", "flip"), ("restraint_atoms", "restraint_x0", None), ("alchemical_atoms", None, None))


class Map:
    """x_new = x_old[perm] @ M.T + shift (shift in the new order and frame); vectors (forces, velocities) transform without the shift.
    `box` is the NEW System's box where positions are to be compared modulo lattice vectors, else None."""

    def __init__(self, n, perm=None, M=None, shift=None, box=None):
        self.perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
        self.M = np.eye(3) if M is None else np.asarray(M, dtype=np.float64)
        self.shift = np.zeros((n, 3)) if shift is None else np.asarray(shift, dtype=np.float64)
        self.box = box

    def then(self, other):
        """The Map of `self`'s transformation followed by `other`'s."""
        return Map(len(self.perm), self.perm[other.perm], other.M @ self.M, self.shift[other.perm] @ other.M.T + other.shift,
                   other.box if other.box is not None else (None if self.box is None else np.abs(other.M) @ self.box))

    def forward_vectors(self, v_old):
        return None if v_old is None else np.asarray(v_old)[self.perm] @ self.M.T

    def vectors(self, f_new):
        """Forces or velocities of the new System in the original's order and axes."""
        out = np.empty_like(np.asarray(f_new, dtype=np.float64))
        out[self.perm] = np.asarray(f_new, dtype=np.float64) @ self.M
        return out

    def positions(self, x_new):
        """Positions of the new System where the original has them (every molecule's own shift taken off)."""
        out = np.empty_like(np.asarray(x_new, dtype=np.float64))
        out[self.perm] = (np.asarray(x_new, dtype=np.float64) - self.shift) @ self.M
        return out

    def per_atom(self, a_new):
        out = np.empty_like(np.asarray(a_new))
        out[self.perm] = np.asarray(a_new)
        return out


def _replace(s, **kw):
    return dataclasses.replace(s, **kw)


def _box3(s):
    return np.asarray(s.box, dtype=np.float64).reshape(-1)[:3] if np.size(s.box) == 3 else np.diag(np.asarray(s.box, dtype=np.float64).reshape(3, 3))


# ---------------------------------------------------------------------------------------------------------------- atom order
def permute_atoms(s, v, perm):
    """The same System with atom `perm[i]` of the original at place i: per-atom arrays re-ordered, every index array re-numbered
    (rows and their order stay: alchemical_atoms and the term lists come out in the original's row order, so in general unsorted)."""
    perm = np.asarray(perm, dtype=np.int64)
    n = s.n_atoms
    assert np.array_equal(np.sort(perm), np.arange(n)), "perm is not a permutation of the atoms"
    new_of_old = np.empty(n, np.int64); new_of_old[perm] = np.arange(n)
    kw = {}
    for name in _PER_ATOM:
        a = getattr(s, name)
        if a is not None:
            kw[name] = np.asarray(a)[perm].copy()
    if s.names is not None:
        kw["names"] = [s.names[i] for i in perm]
    for name in _INDEX_LISTS:
        a = np.asarray(getattr(s, name))
        kw[name] = new_of_old[a.astype(np.int64)].astype(np.int32).reshape(a.shape)
    kw["centroid_bonds"] = tuple(([int(new_of_old[i]) for i in b[0]], list(b[1]), [int(new_of_old[i]) for i in b[2]], list(b[3]), b[4])
                                 for b in (s.centroid_bonds or ()))
    return _replace(s, **kw), (None if v is None else np.asarray(v)[perm].copy()), Map(n, perm=perm)


def molecules(s):
    """label[i]: the molecule of atom i -- connected components over bonds and constraints, numbered by their first atom."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = s.n_atoms
    pairs = np.concatenate([np.asarray(s.bond_atoms, np.int64).reshape(-1, 2), np.asarray(s.constraint_atoms, np.int64).reshape(-1, 2)])
    g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, label = connected_components(g, directed=False)
    first = np.full(label.max() + 1, n, np.int64)
    np.minimum.at(first, label, np.arange(n))
    return np.argsort(np.argsort(first))[label]


def molecule_order_perm(s):
    """Whole molecules re-ordered: every molecule without an alchemical atom in REVERSED order, the ligand's molecule(s) last; the
    order inside a molecule stays."""
    label = molecules(s)
    lig = np.unique(label[np.asarray(s.alchemical_atoms, np.int64)])
    is_lig = np.isin(label, lig)
    key = np.where(is_lig, label.max() + 1 + label, label.max() - label)
    return np.argsort(key, kind="stable")


def scatter_perm(n, seed):
    """A seeded random permutation of all atoms: no molecule stays contiguous."""
    return np.random.RandomState(seed).permutation(n)


# ---------------------------------------------------------------------------------------------------------------- term order
def shuffle_terms(s, rng, v=None):
    """Rows of every term list in random order with their parameter rows; pair rows flipped at random, angles and torsions reversed
    at random (phi(a,b,c,d) = phi(d,c,b,a)); alchemical_atoms shuffled and left unsorted; centroid bonds in random order, their two
    groups swapped and each group's atoms shuffled with their weights.  Map.terms records what was done (unshuffle_terms)."""
    kw, rec = {}, {}
    for name, par, turn in _TERM_LISTS:
        a = np.asarray(getattr(s, name))
        order = rng.permutation(len(a))
        b = a[order].copy()
        flipped = np.zeros(len(a), bool)
        if turn is not None and len(a):
            flipped = rng.randint(0, 2, len(a)).astype(bool)
            b[flipped] = b[flipped][:, ::-1]
        kw[name] = b
        if par is not None:
            kw[par] = np.asarray(getattr(s, par))[order].copy()
        rec[name] = (order, flipped)
    bonds = list(s.centroid_bonds or ())
    border = rng.permutation(len(bonds))
    new_bonds, brec = [], []
    for q in border:
        i1, w1, i2, w2, k = bonds[q]
        swap = bool(rng.randint(0, 2))
        o1, o2 = rng.permutation(len(i1)), rng.permutation(len(i2))
        g1 = ([i1[j] for j in o1], [w1[j] for j in o1]); g2 = ([i2[j] for j in o2], [w2[j] for j in o2])
        if swap:
            g1, g2 = g2, g1
        new_bonds.append((g1[0], g1[1], g2[0], g2[1], k)); brec.append((int(q), swap, o1, o2))
    kw["centroid_bonds"] = tuple(new_bonds)
    m = Map(s.n_atoms)
    m.terms = (rec, brec)
    return _replace(s, **kw), (None if v is None else np.array(v, copy=True)), m


def unshuffle_terms(s, m):
    """Inverse of shuffle_terms, from the record its Map carries."""
    rec, brec = m.terms
    kw = {}
    for name, par, turn in _TERM_LISTS:
        order, flipped = rec[name]
        b = np.asarray(getattr(s, name)).copy()
        if turn is not None and len(b):
            b[flipped] = b[flipped][:, ::-1]
        a = np.empty_like(b); a[order] = b
        kw[name] = a
        if par is not None:
            p = np.asarray(getattr(s, par)); q = np.empty_like(p); q[order] = p
            kw[par] = q
    bonds = [None] * len(brec)
    for (q, swap, o1, o2), (j1, x1, j2, x2, k) in zip(brec, s.centroid_bonds or ()):
        if swap:
            j1, x1, j2, x2 = j2, x2, j1, x1
        i1, w1, i2, w2 = [None] * len(j1), [None] * len(j1), [None] * len(j2), [None] * len(j2)
        for pos, j in enumerate(o1):
            i1[j], w1[j] = j1[pos], x1[pos]
        for pos, j in enumerate(o2):
            i2[j], w2[j] = j2[pos], x2[pos]
        bonds[q] = (i1, w1, i2, w2, k)
    kw["centroid_bonds"] = tuple(bonds)
    return _replace(s, **kw)


def sort_alchemical(s):
    """The same System with alchemical_atoms ascending (the form a caller that builds the list from a selection hands over)."""
    return _replace(s, alchemical_atoms=np.sort(np.asarray(s.alchemical_atoms, np.int32)))


# ---------------------------------------------------------------------------------------------------------------- place in space
def unwrap_molecules(s, rng, kmax=3, v=None):
    """What a long trajectory hands over: every molecule (molecules(): whole, never split) moved by its own integer multiples of the
    box edges in [-kmax, kmax] per axis, negative coordinates included, plus one shift of everything that is no lattice vector.
    Direct space is invariant under any such shift.  The reciprocal-space MESH is invariant only under whole mesh cells (B-spline
    interpolation error depends on where an atom sits in its cell), so under NB_PME the global shift is a random whole number of
    mesh cells per axis -- still no lattice vector, and a symmetry to rounding."""
    if int(s.nonbonded_method) == _abi.NB_NOCUTOFF:
        raise ValueError("unwrap_molecules: a NoCutoff System has no lattice")
    box = _box3(s)
    label = molecules(s)
    k = rng.randint(-kmax, kmax + 1, size=(label.max() + 1, 3))
    if int(s.nonbonded_method) == _abi.NB_PME:
        K = np.asarray(s.pme_grid, dtype=np.float64)
        g = rng.randint(1, 4, size=3) * rng.choice([-1, 1], size=3) * box / K
    else:
        g = rng.uniform(-1.0, 1.0, size=3) * box
    shift = k[label] * box + g
    kw = {"positions": np.asarray(s.positions, dtype=np.float64) + shift}
    if len(np.asarray(s.restraint_atoms).reshape(-1)):
        kw["restraint_x0"] = np.asarray(s.restraint_x0, dtype=np.float64).reshape(-1, 3) + shift[np.asarray(s.restraint_atoms, np.int64)]
    return _replace(s, **kw), (None if v is None else np.array(v, copy=True)), Map(s.n_atoms, shift=shift, box=box.copy())


def cycle_axes(s, v, times=1):
    """(x, y, z) -> (y, z, x), `times` times over (3 is the identity, 2 the inverse of 1): positions, box, restraint_x0 and velocities;
    the PME mesh is derived again from the new box, as a caller would."""
    ax = np.roll(np.arange(3), -int(times) % 3)          # new column c = old column ax[c]
    assert np.size(s.box) == 3
    kw = {"positions": np.asarray(s.positions)[:, ax].copy(), "box": np.asarray(s.box, dtype=np.float64)[ax].copy()}
    if len(np.asarray(s.restraint_atoms).reshape(-1)):
        kw["restraint_x0"] = np.asarray(s.restraint_x0, dtype=np.float64).reshape(-1, 3)[:, ax].copy()
    if int(s.nonbonded_method) == _abi.NB_PME:
        kw["pme_grid"] = systems.pme_grid_for(kw["box"], s.ewald_alpha, s.cutoff)
    M = np.eye(3)[ax]                                      # x_new = x_old @ M.T picks column ax[c] into c
    return _replace(s, **kw), (None if v is None else np.asarray(v)[:, ax].copy()), Map(s.n_atoms, M=M)


def rotation_matrix(axis, angle):
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rotate(s, v, R, translation=(0.0, 0.0, 0.0)):
    """A proper rotation about the centroid plus a translation.  NoCutoff Systems only: a box is not invariant."""
    if int(s.nonbonded_method) != _abi.NB_NOCUTOFF:
        raise ValueError("rotate: only a NoCutoff System is invariant under rotations")
    R = np.asarray(R, dtype=np.float64)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0, "R is not a proper rotation"
    x = np.asarray(s.positions, dtype=np.float64)
    c = x.mean(0)
    t = c - c @ R.T + np.asarray(translation, dtype=np.float64)       # x' = x R^T + t
    kw = {"positions": x @ R.T + t}
    if len(np.asarray(s.restraint_atoms).reshape(-1)):
        kw["restraint_x0"] = np.asarray(s.restraint_x0, dtype=np.float64).reshape(-1, 3) @ R.T + t
    return _replace(s, **kw), (None if v is None else np.asarray(v) @ R.T), Map(s.n_atoms, M=R, shift=np.tile(t, (s.n_atoms, 1)))


def chain(s, v, *steps):
    """Apply steps (callables (s, v) -> (s, v, Map)) one after the other; returns (s, v, the composed Map)."""
    m = Map(s.n_atoms)
    for step in steps:
        s, v, m2 = step(s, v)
        m = m.then(m2)
    return s, v, m
