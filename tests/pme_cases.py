"""Mesh shapes, mobile sets and placements shared by tests/test_pme_shapes_cpu.py and tests/test_gpu_pme_shapes.py (no test of its own),
and a host-side model of the path the mixed-precision mesh kernel takes (blues_amd/csrc/kernels_pme.h: pme_fast_body,
blues_engine.hip: launch_pme_t).  The model steers the choice of cases and makes failures readable; what the GPU tests assert is the
counter the kernel keeps (stats()["pme_fast_launches"] / ["pme_general_launches"])."""
import collections
import copy

import numpy as np

from blues_amd import systems

ORDER = 5
LDS_X, LDS_Y, LDS_ATOMS = 7424, 9280, 768      # kernels_pme.h: PME_LDS_X, PME_LDS_Y, PME_LDS_ATOMS
SHIFTS = (None, "corner", "xface", "yface", "zface", "centre")
N_LIG = 15


# ---- the model
def mesh_index(x, box, K):
    """pme_locate: (t, u) per atom and axis, t = mesh index in [0, K), u = fractional mesh coordinate in [0, K]"""
    inv = 1.0 / np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    fr = np.asarray(x, dtype=np.float64) * inv
    fr = fr - np.floor(fr)
    u = fr * np.asarray(K, dtype=np.float64)
    t = u.astype(np.int64)
    return np.where(t >= np.asarray(K), t - np.asarray(K), t), u


def mesh_charges(system, full_charges=False):
    """qn of the launch: every atom's charge with the alchemical atoms at 0 ('direct-space' treatment), or all of them (qn_full)"""
    q = np.array(system.charge, dtype=np.float64, copy=True)
    if not full_charges:
        q[np.asarray(system.alchemical_atoms, dtype=np.int64)] = 0.0
    return q


def expected_block(system, positions=None, full_charges=False):
    """(L, s): extents and start of the block of the mesh that holds the stencils of the charged mobile atoms, relative to the first of them
    in index order, through the periodic wrap -- (1, 1, 1) at 0 when there is none."""
    K = tuple(int(k) for k in system.pme_grid)
    x = system.positions if positions is None else positions
    sel = np.nonzero(np.asarray(system.mass) != 0.0)[0]
    q = mesh_charges(system, full_charges)[sel].astype(np.float32)
    t = mesh_index(np.asarray(x)[sel], system.box, K)[0][q != 0.0]
    if len(t) == 0:
        return (1, 1, 1), (0, 0, 0)
    L, s = [], []
    for d in range(3):
        de = t[:, d] - t[0, d]
        de = np.where(2 * de >= K[d], de - K[d], np.where(2 * de < -K[d], de + K[d], de))
        Ld, sd = int(de.max() - de.min()) + ORDER, int((t[0, d] + de.min()) % K[d])
        if Ld >= K[d]:
            Ld, sd = K[d], 0
        L.append(Ld); s.append(sd)
    return tuple(L), tuple(s)


def expected_path(system, positions=None, full_charges=False):
    """("fast" | "general:host" | "general:atoms" | "general:block", (Lx, Ly, Lz)) of a mixed-precision mobile launch"""
    K0, K1, K2 = (int(k) for k in system.pme_grid)
    Hz = K2 // 2 + 1
    n_sel = int((np.asarray(system.mass) != 0.0).sum())
    (Lx, Ly, Lz), _ = expected_block(system, positions, full_charges)
    if K0 * K1 * Hz > LDS_Y:
        return "general:host", (Lx, Ly, Lz)
    if n_sel > LDS_ATOMS:
        return "general:atoms", (Lx, Ly, Lz)
    fits = (Lx * Ly * Lz <= LDS_X and Lx * K1 * Hz <= LDS_X and Lx * Ly * Hz <= LDS_Y and n_sel * 16 <= LDS_X
            and (Lx * Ly * Lz + 4 + n_sel * 48 + 1) // 2 <= LDS_Y)
    return ("fast" if fits else "general:block"), (Lx, Ly, Lz)


def block_class(system, L):
    """"whole" (the block is the mesh), "partial" (shorter than the mesh on all three axes), "one-full" (the whole mesh along exactly one
    axis, start 0 there, beside two partial axes) or "two-full" (partial on one axis only)"""
    full = sum(L[d] >= system.pme_grid[d] for d in range(3))
    return ("partial", "one-full", "two-full", "whole")[full]


def wraps(system, positions=None):
    """per axis: the block runs through the periodic edge of the mesh (start + extent > K, extent < K)"""
    L, s = expected_block(system, positions)
    return tuple(L[d] < system.pme_grid[d] and s[d] + L[d] > system.pme_grid[d] for d in range(3))


# ---- builders on the 975-atom toluene box
_base = []


def base():
    if not _base:
        s, v = systems.toluene_box()
        _base.append((systems.with_reciprocal_space(s), v))
    return _base[0]


def _waters(s):
    """first atoms of the water molecules (three atoms each, behind the ligand)"""
    return np.arange(N_LIG, s.n_atoms, 3)


def mobile_nearest(s, n_atoms):
    """the ligand and the nearest whole waters, n_atoms in all (n_atoms = 15: the ligand alone)"""
    lig = np.arange(N_LIG)
    if n_atoms <= N_LIG:
        return systems.freeze_except(s, lig)
    near = systems.nearest_molecules(s, lig, n_atoms - N_LIG, exclude_idx=lig)
    return systems.freeze_except(s, np.concatenate([lig, near]))


def spread(s, step):
    """the ligand and every step-th water mobile: a mobile set across the whole box"""
    first = _waters(s)[::step]
    return systems.freeze_except(s, np.concatenate([np.arange(N_LIG)] + [first + k for k in range(3)]))


def shift(s, name):
    """all positions moved so that the ligand's centroid sits on a box corner, on the middle of the x / y / z face only, or at the centre"""
    if name is None:
        return s
    L = np.asarray(s.box, dtype=np.float64).reshape(-1)[:3]
    target = {"corner": (0.0, 0.0, 0.0), "xface": (0.0, 0.5, 0.5), "yface": (0.5, 0.0, 0.5), "zface": (0.5, 0.5, 0.0), "centre": (0.5, 0.5, 0.5)}[name] * L
    r = copy.copy(s)
    r.positions = np.asarray(s.positions, dtype=np.float64) - np.asarray(s.positions)[:N_LIG].mean(0) + target
    return r


def uncharged_frozen(s):
    """every frozen atom's charge at 0: no static launch, have_static == 0"""
    r = copy.copy(s)
    r.charge = np.array(s.charge, dtype=np.float64, copy=True)
    r.charge[np.asarray(s.mass) == 0.0] = 0.0
    frozen = np.asarray(s.mass) == 0.0
    ea = np.asarray(s.exception_atoms, dtype=np.int64).reshape(-1, 2)
    if len(ea):      # (an exception that holds an uncharged atom carries no charge product)
        r.exception_params = np.array(s.exception_params, dtype=np.float64, copy=True).reshape(-1, 3)
        r.exception_params[frozen[ea[:, 0]] | frozen[ea[:, 1]], 0] = 0.0
    return r


def scattered(s, want="general:block"):
    """Positions in which mobile waters are translated apart, molecule by molecule, each onto the site of a frozen water that takes its
    place in turn (identical molecules: no contact changes), farthest sites first, until the model gives `want`."""
    x = np.array(s.positions, dtype=np.float64, copy=True)
    L = np.asarray(s.box, dtype=np.float64).reshape(-1)[:3]
    mob = np.asarray(s.mass) != 0.0
    first = _waters(s)
    c = x[:N_LIG].mean(0)
    d = x[first] - c; d -= L * np.round(d / L)
    far = [f for f in first[np.argsort(-np.abs(d).max(1), kind="stable")] if not mob[f]]
    near = [f for f in first if mob[f]]
    for a, b in zip(near, far):
        for k in range(3):
            x[[a + k, b + k]] = x[[b + k, a + k]]
        if expected_path(s, x)[0] == want:
            return x
    raise AssertionError("no arrangement of the mobile waters gives %s" % want)


def exact_plane(x, axis, box, K):
    """the coordinate nearest x whose fractional mesh coordinate along `axis`, as pme_locate forms it, is an exact integer"""
    L, Kd = float(np.asarray(box).reshape(-1)[axis]), int(K[axis])
    inv = 1.0 / L
    m = np.round(x * Kd / L)
    t0 = m * L / Kd
    cands = [t0]
    for _ in range(8):
        cands = [np.nextafter(cands[0], -np.inf)] + cands + [np.nextafter(cands[-1], np.inf)]
    for t in sorted(cands, key=lambda t: abs(t - t0)):
        fr = t * inv; fr -= np.floor(fr); u = fr * Kd
        if u == np.floor(u):
            return float(t)
    raise AssertionError("no exact mesh plane within 8 ulps of %r" % t0)


PLANE_TARGETS = ("minus_tiny", "box_edge", "two_boxes", "plane0", "plane1", "plane2")      # (the box edge first: it has the fewest waters near it)


def on_planes(s, ulps=0):
    """Mobile waters moved rigidly (whole molecules, by less than a mesh cell) so that one atom of each has, in turn: coordinate -1e-17 (axis 0);
    coordinate exactly L (axis 1); coordinate 2 L + 1e-12 (axis 2); x K / L an exact integer on axis 0 / 1 / 2.  ulps = +-1: the
    same coordinates one unit in the last place to either side.  Returns (System, [(atom, axis, coordinate)])."""
    r = copy.copy(s)
    x = np.array(s.positions, dtype=np.float64, copy=True)
    L = np.asarray(s.box, dtype=np.float64).reshape(-1)[:3]
    K = tuple(int(k) for k in s.pme_grid)
    free = [f for f in _waters(s) if s.mass[f] != 0.0]
    planted = []
    for name in PLANE_TARGETS:
        cand = [(f, f + k) for f in free for k in range(3)]      # (molecule, the atom of it that is planted)
        if name.startswith("plane"):
            ax = int(name[-1])
            dist = [abs(x[a, ax] * K[ax] / L[ax] - np.round(x[a, ax] * K[ax] / L[ax])) for _, a in cand]
            f, a = cand[int(np.argmin(dist))]
            t = exact_plane(x[a, ax], ax, L, K)
        else:
            ax = PLANE_TARGETS.index(name)
            dist = [abs(x[a, ax] - L[ax] * np.round(x[a, ax] / L[ax])) for _, a in cand]
            f, a = cand[int(np.argmin(dist))]
            t = {"minus_tiny": -1e-17, "box_edge": float(L[ax]), "two_boxes": 2.0 * float(L[ax]) + 1e-12}[name]
        free.remove(f)
        # (the nearest periodic image of the molecule to the planted coordinate, then the rigid move)
        x[f:f + 3, ax] += L[ax] * np.round((t - x[a, ax]) / L[ax])
        x[f:f + 3, ax] += t - x[a, ax]
        if ulps:
            t = float(np.nextafter(t, np.inf if ulps > 0 else -np.inf))
        x[a, ax] = t
        planted.append((int(a), ax, float(t)))
    r.positions = x
    return r, planted


def scaled_box(s, scale):
    """(box, positions) of the box scaled per axis with every molecule moved rigidly by its centroid, as the barostat scales"""
    scale = np.asarray(scale, dtype=np.float64)
    x = np.array(s.positions, dtype=np.float64, copy=True)
    res = np.asarray(s.residue_of_atom)
    for m in np.unique(res):
        idx = np.nonzero(res == m)[0]
        c = x[idx].mean(0)
        x[idx] += c * scale - c
    return np.asarray(s.box, dtype=np.float64).reshape(-1)[:3] * scale, x


# ---- the table
Case = collections.namedtuple("Case", "id mesh mobile spread shift kind block")


def _rows():
    rows = []

    def add(mesh, mobile, kind, block, spread_step=None, shifts=(None,)):
        for sh in shifts:
            name = "%dx%dx%d-%s%s" % (mesh + (("spread%d" % spread_step) if spread_step else str(mobile), "-" + sh if sh else ""))
            rows.append(Case(name, mesh, mobile, spread_step, sh, kind, block))
    add((9, 9, 9), 150, "fast", "whole")
    add((5, 5, 5), 150, "fast", "whole")                      # K == order: every stencil covers every axis
    add((20, 18, 27), 45, "fast", "partial", shifts=SHIFTS)   # odd K2 in the half spectrum
    add((18, 20, 32), 45, "fast", "partial", shifts=SHIFTS)   # even K2: the Nyquist plane
    add((27, 20, 18), 45, "fast", "partial", shifts=SHIFTS)   # odd K0
    add((24, 24, 30), 45, "fast", "partial", shifts=SHIFTS)   # half spectrum 9,216 <= 9,280
    add((24, 24, 32), 45, "general:host", "partial")          # 9,792 > 9,280
    add((24, 24, 30), 150, "general:block", None)
    add((8, 20, 27), 45, "fast", "one-full", shifts=SHIFTS)   # L == K on x only (start 0 there), y and z partial and wrapping with the shifts
    add((20, 8, 27), 45, "fast", "one-full", shifts=SHIFTS)   # ... on y only
    add((20, 18, 8), 45, "fast", "one-full", shifts=SHIFTS)   # ... on z only: the whole half spectrum beside two pruned axes
    add((6, 7, 64), 150, "fast", "two-full")                  # full on two axes, partial on the long one
    add((64, 7, 6), 150, "fast", "two-full")
    add((6, 7, 64), 300, "fast", "whole")
    add((64, 7, 6), 300, "fast", "whole")
    add((24, 24, 30), 255, "general:block", None, spread_step=4)
    add((9, 9, 9), 255, "fast", "whole", spread_step=4)
    add((9, 9, 9), 345, "fast", "whole")
    add((9, 9, 9), 360, "fast", "whole")
    add((9, 9, 9), 390, "general:block", "whole")             # the weights no longer fit beside the block
    add((10, 12, 15), 345, "fast", "whole")
    add((10, 12, 15), 360, "general:block", "whole")
    add((9, 9, 9), 975, "general:atoms", "whole")
    return rows


CASES = _rows()
BY_ID = {c.id: c for c in CASES}
_built = {}


def build(case):
    """the System of a row (made once, shared, not to be changed)"""
    if case.id not in _built:
        s = copy.copy(base()[0])
        s.pme_grid = tuple(case.mesh)
        if case.spread:
            s = spread(s, case.spread)
        elif case.mobile < s.n_atoms:
            s = mobile_nearest(s, case.mobile)
        _built[case.id] = shift(s, case.shift)
    return _built[case.id]


def mesh_energy_of(system, oracle, terms=None):
    """1/2 sum eterm |Q^|^2 from the oracle's term [8]: the self term, the neutralising background and the erf corrections of the excluded
    pairs taken off again (tests/test_oracle_pme.py::_mesh_energy)."""
    from math import erf
    KE = 138.935456
    T = oracle.energy_forces(1.0, 1.0)[2] if terms is None else terms
    q = mesh_charges(system)
    box = np.asarray(system.box, dtype=np.float64).reshape(-1)[:3]
    al = system.ewald_alpha
    e = T[8] + KE * al / np.sqrt(np.pi) * (q ** 2).sum() + np.pi * KE * q.sum() ** 2 / (2 * np.prod(box) * al ** 2)
    x = oracle.get_positions()
    for a, b in np.asarray(system.exclusions):
        if q[a] * q[b] != 0.0:
            d = x[a] - x[b]; d -= box * np.round(d / box); r = np.linalg.norm(d)
            e += KE * q[a] * q[b] * erf(al * r) / r
    return e
