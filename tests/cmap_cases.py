"""Systems and maps shared by tests/test_cmap_cpu.py and tests/test_gpu_cmap.py (no test of its own)."""
import copy
import os

import numpy as np

from blues_amd import _abi, amber

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TWO_PI = 2.0 * np.pi


def surface(phi, psi):
    """the analytic surface of the issue: smooth, periodic, not symmetric under phi <-> psi"""
    return 4.0 * np.cos(phi) + 2.0 * np.sin(2.0 * psi) + 3.0 * np.cos(phi - psi + 0.4)


def surface_map(n):
    g = np.arange(n) * TWO_PI / n
    return surface(g[:, None], g[None, :])


def random_map(n, seed=5):
    return np.random.default_rng(seed).normal(size=(n, n)) * 6.0


def backbone_atoms(names):
    """C-N-CA-C-N of the backbone by atom name: the first C, then the next N, CA, C after it and the N that follows -- or, where the
    chain ends there (a dipeptide has no third residue), the terminal OXT in the place the next residue's N would take."""
    names = list(names)
    c0 = names.index("C")
    n1 = names.index("N", c0); ca = names.index("CA", n1); c1 = names.index("C", ca)
    last = names.index("N", c1) if "N" in names[c1:] else names.index("OXT", c1)
    return [c0, n1, ca, c1, last]


_cache = {}


def divaline(maps=None, five=None):
    """vacDivaline (35 atoms, NoCutoff, HBonds), optionally with one CMAP torsion in Amber's five-atom form on its backbone"""
    if "val" not in _cache:
        prm = amber.read_prmtop(os.path.join(GOLDEN, "vacDivaline.prmtop"))
        pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "vacDivaline.inpcrd"))
        _cache["val"] = amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=list(range(22, 32)), nonbonded_method="NoCutoff")
    s = copy.deepcopy(_cache["val"])
    if maps is not None:
        a = backbone_atoms(s.names) if five is None else list(five)
        s.cmap_maps = tuple(maps)
        s.cmap_torsions = np.array([[0, a[0], a[1], a[2], a[3], a[1], a[2], a[3], a[4]]], np.int32)
    return s


def chain(x, maps, torsions, box=None, bonds=True):
    """atoms with harmonic bonds along the chain, no charges, no Lennard-Jones, one plain torsion over the first four: a System whose
    only forces that matter are bonded"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    pairs = np.array([(i, i + 1) for i in range(n - 1)], np.int32)
    r0 = np.linalg.norm(x[pairs[:, 0]] - x[pairs[:, 1]], axis=1)
    excl = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
    return _abi.SystemData(
        box=np.zeros(3) if box is None else np.asarray(box, dtype=np.float64), mass=np.full(n, 12.0), charge=np.zeros(n), sigma=np.full(n, 0.3), epsilon=np.zeros(n),
        exclusions=excl, bond_atoms=pairs if bonds else np.zeros((0, 2), np.int32),
        bond_params=np.stack([r0, np.full(n - 1, 2.0e5)], axis=1) if bonds else np.zeros((0, 2)),
        torsion_atoms=np.array([[0, 1, 2, 3]], np.int32), torsion_params=np.array([[2.0, 0.3, 5.0]]),
        nonbonded_method=_abi.NB_NOCUTOFF, positions=x, cmap_maps=tuple(maps), cmap_torsions=np.asarray(torsions, np.int32).reshape(-1, 9))


def five_atoms(phi, psi, b=0.15, theta=1.9):
    """five positions whose dihedrals (0,1,2,3) and (1,2,3,4) are exactly phi and psi in the convention of cmap_reference.dihedral
    (up to rounding): built atom by atom from bond length, bond angle and dihedral"""
    def place(a, bb, c, ang):
        bc = (c - bb) / np.linalg.norm(c - bb)
        nrm = np.cross(bb - a, bc); nrm /= np.linalg.norm(nrm)
        m = np.cross(nrm, bc)
        d = np.array([-b * np.cos(theta), b * np.sin(theta) * np.cos(ang), b * np.sin(theta) * np.sin(ang)])
        return c + d[0] * bc + d[1] * m + d[2] * nrm
    x = [b * np.array([np.cos(theta), np.sin(theta), 0.0]), np.zeros(3), np.array([b, 0.0, 0.0])]
    x.append(place(x[0], x[1], x[2], phi))
    x.append(place(x[1], x[2], x[3], psi))
    return np.array(x) + np.array([0.31, -0.12, 0.07])
