"""A chamber-style topology written from tests/golden/vacDivaline.prmtop, and the Systems that tests/test_charmm_cpu.py and
tests/test_gpu_charmm.py share (no test of its own).

The written file has what chamber writes and an Amber file does not: %FLAG CTITLE with %FORMAT(a80), FORCE_FIELD_TYPE with
%FORMAT(i2,a78), %COMMENT lines inside sections, SCEE / SCNB of 1.0, a Urey-Bradley term on every angle that has a hydrogen,
impropers on three planar centres (central atom first) and two tetrahedral ones, and a 1-4 Lennard-Jones table that is the main one
with every entry scaled by a factor of its own type pair -- a reader that ignores the table is caught."""
import copy
import dataclasses
import os
import tempfile

import numpy as np

from blues_amd import _abi, amber

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KCAL = 4.184

# 0-based quadruples: C, N and the carboxylate C with their three neighbours (planar), CA and CB of the first residue (tetrahedral)
IMPROPERS = [(16, 4, 18, 17), (18, 16, 20, 19), (32, 20, 34, 33), (4, 0, 6, 16), (6, 4, 8, 12)]
IMPROPER_TYPE = [1, 1, 1, 2, 3]                       # 1-based, as the file holds them
IMPROPER_K = [120.0, 45.5, 38.25]                     # kcal/mol/rad^2
IMPROPER_PHASE = [0.0, -35.26439, -30.0]              # degrees: the tetrahedral centres sit near -0.6 rad
UB_K = [30.0, 5.4, 22.53, 48.7]                       # kcal/mol/A^2
UB_S0 = [2.179, 1.802, 2.14731, 2.101]                # A


def _written(values, form):
    """the numbers a reader gets back from the text"""
    return [float(form % v) for v in values]


def plain_prmtop():
    return os.path.join(GOLDEN, "vacDivaline.prmtop")


def _sections(text):
    """[(name, [lines after the %FLAG line])] in file order, and the lines before the first flag"""
    head, out = [], []
    for line in text.split("\n"):
        if line.startswith("%FLAG"):
            out.append((line.split()[1], []))
        elif out:
            out[-1][1].append(line)
        else:
            head.append(line)
    return head, out


def _body(fmt, values, per_line, form, comment=None):
    lines = ["%COMMENT  " + comment] if comment else []
    lines.append("%%FORMAT(%s)" % fmt)
    values = list(values)
    for k in range(0, len(values), per_line):
        lines.append("".join(form % v for v in values[k:k + per_line]))
    if not values:
        lines.append("")
    return lines


def lj14_factors(n):
    """what entry k of the 1-4 table is of entry k of the main one: (A factor, B factor), different for every k mod 35"""
    k = np.arange(n)
    return 0.5 + 0.03 * (k % 7), 0.6 + 0.02 * (k % 5)


def write_chamber(dirpath, name="chamber.prmtop", edit=None):
    """Writes the file; returns (path, expected) with `expected` the numbers the file holds, as a reader gets them back.
    `edit(sections)` may change the dict {name: lines} of the sections this function adds or replaces before the file is written."""
    plain = amber.read_prmtop(plain_prmtop())
    head, secs = _sections(open(plain_prmtop()).read().rstrip("\n"))
    ang = np.asarray(plain["ANGLES_INC_HYDROGEN"]).reshape(-1, 4)
    ub_pairs = [(int(a[0]) // 3, int(a[2]) // 3) for a in ang]
    ub_type = [1 + k % len(UB_K) for k in range(len(ub_pairs))]
    ntab = len(plain["LENNARD_JONES_ACOEF"])
    fa, fb = lj14_factors(ntab)
    a14, b14 = np.asarray(plain["LENNARD_JONES_ACOEF"]) * fa, np.asarray(plain["LENNARD_JONES_BCOEF"]) * fb
    nd = len(plain["DIHEDRAL_FORCE_CONSTANT"])
    E, I = "%16.8E", "%8d"
    new = {
        "CTITLE": ["%FORMAT(a80)", "chamber-style topology of the valine dipeptide, written for the tests"],
        "FORCE_FIELD_TYPE": ["%FORMAT(i2,a78)", " 1 CHARMM  36       *>>>> CHARMM36 All-Hydrogen Topology File for Proteins <<<<<<"],
        "SCEE_SCALE_FACTOR": _body("5E16.8", [1.0] * nd, 5, E, "CHARMM scales no 1-4 electrostatics"),
        "SCNB_SCALE_FACTOR": _body("5E16.8", [1.0] * nd, 5, E, "the 1-4 table below says everything"),
        "CHARMM_UREY_BRADLEY_COUNT": _body("2I8", [len(ub_pairs), len(UB_K)], 2, I, "V(S) = K_UB(S - S0)^2"),
        "CHARMM_UREY_BRADLEY": _body("10I8", [v for (i, j), t in zip(ub_pairs, ub_type) for v in (i + 1, j + 1, t)], 10, I, "List of the two atoms and its parameter index"),
        "CHARMM_UREY_BRADLEY_FORCE_CONSTANT": _body("5E16.8", UB_K, 5, E, "K_UB: kcal/mol/A**2"),
        "CHARMM_UREY_BRADLEY_EQUIL_VALUE": _body("5E16.8", UB_S0, 5, E, "r_UB: A"),
        "CHARMM_NUM_IMPROPERS": _body("10I8", [len(IMPROPERS)], 10, I, "Number of terms contributing to the quadratic four atom improper energy term"),
        "CHARMM_IMPROPERS": _body("10I8", [v for q, t in zip(IMPROPERS, IMPROPER_TYPE) for v in [a + 1 for a in q] + [t]], 10, I, "List of the four atoms in each improper term"),
        "CHARMM_NUM_IMPR_TYPES": _body("1I8", [len(IMPROPER_K)], 1, I, "Number of unique parameters"),
        "CHARMM_IMPROPER_FORCE_CONSTANT": _body("5E16.8", IMPROPER_K, 5, E, "K_psi: kcal/mole/rad**2"),
        "CHARMM_IMPROPER_PHASE": _body("5E16.8", IMPROPER_PHASE, 5, E, "psi: degrees"),
        "LENNARD_JONES_14_ACOEF": _body("5E16.8", a14, 5, E),
        "LENNARD_JONES_14_BCOEF": _body("5E16.8", b14, 5, E),
    }
    if edit is not None:
        edit(new)
    lines = list(head)
    used = set()
    for sec, body in secs:
        if sec == "TITLE":      # chamber's title section, then the force-field line
            for k in ("CTITLE", "FORCE_FIELD_TYPE"):
                lines += ["%%FLAG %s" % k] + new[k]; used.add(k)
            continue
        lines.append("%%FLAG %s" % sec)
        if sec in new:
            lines += new[sec]; used.add(sec)
        else:
            lines += body
    for k, body in new.items():
        if k not in used:
            lines += ["%%FLAG %s" % k] + body
    path = os.path.join(str(dirpath), name)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    ty = np.array(ub_type) - 1
    ity = np.array(IMPROPER_TYPE) - 1
    expected = {
        "ub_atoms": np.array(ub_pairs, np.int32), "ub_k": np.array(_written(UB_K, E))[ty], "ub_s0": np.array(_written(UB_S0, E))[ty],
        "improper_atoms": np.array(IMPROPERS, np.int32), "improper_k": np.array(_written(IMPROPER_K, E))[ity],
        "improper_phase": np.array(_written(IMPROPER_PHASE, E))[ity],
        "a14": np.array(_written(a14, E)), "b14": np.array(_written(b14, E)),
    }
    return path, expected


def positions():
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "vacDivaline.inpcrd"))
    return pos, box


_cache = {}


def _from(path, constraints="HBonds"):
    pos, box = positions()
    return amber.system_from_amber(amber.read_prmtop(path), pos, box, constraints=constraints, alchemical_atoms=list(range(22, 32)), nonbonded_method="NoCutoff")


def chamber_divaline(constraints="HBonds"):
    """vacDivaline read from the written chamber file (35 atoms, NoCutoff, HBonds; the second valine's side chain alchemical)"""
    if ("chamber", constraints) not in _cache:
        with tempfile.TemporaryDirectory() as d:
            _cache[("chamber", constraints)] = _from(write_chamber(d)[0], constraints)
    return copy.deepcopy(_cache[("chamber", constraints)])


def amber_divaline():
    if "amber" not in _cache:
        _cache["amber"] = _from(plain_prmtop())
    return copy.deepcopy(_cache["amber"])


EMPTY = dict(urey_bradley_atoms=np.zeros((0, 2), np.int32), urey_bradley_params=np.zeros((0, 2)),
             improper_atoms=np.zeros((0, 4), np.int32), improper_params=np.zeros((0, 2)))


def without(s):
    """the same System without its Urey-Bradley terms and impropers"""
    return dataclasses.replace(s, **{k: v.copy() for k, v in EMPTY.items()})


def bare(x, ub=None, impr=None, mass=12.0):
    """atoms at x with no charges, no Lennard-Jones (epsilon 0), every pair excluded and no other term: NoCutoff, only the CHARMM
    terms pull.  ub = (atoms, params), impr = (atoms, params)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    excl = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
    kw = {k: v.copy() for k, v in EMPTY.items()}
    if ub is not None:
        kw["urey_bradley_atoms"], kw["urey_bradley_params"] = np.asarray(ub[0], np.int32).reshape(-1, 2), np.asarray(ub[1], np.float64).reshape(-1, 2)
    if impr is not None:
        kw["improper_atoms"], kw["improper_params"] = np.asarray(impr[0], np.int32).reshape(-1, 4), np.asarray(impr[1], np.float64).reshape(-1, 2)
    return _abi.SystemData(box=np.zeros(3), mass=np.full(n, float(mass)), charge=np.zeros(n), sigma=np.full(n, 0.3), epsilon=np.zeros(n),
                           exclusions=excl, nonbonded_method=_abi.NB_NOCUTOFF, positions=x, **kw)


def ring_path(s, start=0, length=6):
    """`length` atoms bonded in a row through harmonic bonds (heavy atoms), from the first atom at or after `start` that has one"""
    nb = {}
    for a, b in np.asarray(s.bond_atoms):
        nb.setdefault(int(a), []).append(int(b)); nb.setdefault(int(b), []).append(int(a))

    def walk(path):
        if len(path) == length:
            return path
        for q in nb.get(path[-1], []):
            if q not in path:
                out = walk(path + [q])
                if out:
                    return out
        return None
    for first in range(start, start + 15):
        p = walk([first])
        if p:
            return p
    raise AssertionError("no bonded path")


def with_ring_terms(s):
    """Urey-Bradley terms over the 1-3 pairs and impropers over three quadruples of a six-atom bonded path on the toluene (the box's
    ligand, atoms 0..14; within the molecule no image is needed in the stored positions); every psi0 lies 0.05 to 0.2 rad from the
    stored geometry's angle, wherever on the circle that is.  Returns (System, path)."""
    import charmm_reference as ref
    a = ring_path(s, 0)
    x = np.asarray(s.positions)
    ub = [(a[k], a[k + 2]) for k in range(4)]
    r0 = [0.97 * np.linalg.norm(x[i] - x[j]) for i, j in ub]
    imp = [(a[0], a[1], a[2], a[3]), (a[2], a[1], a[3], a[4]), (a[2], a[3], a[4], a[5])]
    psi0 = [ref.wrap(p + d) for p, d in zip(ref.improper_angles(imp, x), (0.05, 0.2, -0.1))]
    return dataclasses.replace(s, urey_bradley_atoms=np.array(ub, np.int32), urey_bradley_params=np.stack([r0, [2.5e4, 1.8e4, 3.1e4, 2.2e4]], axis=1),
                               improper_atoms=np.array(imp, np.int32), improper_params=np.stack([psi0, [400.0, 150.0, 260.0]], axis=1)), a


def _bad(s):
    r = dataclasses.replace
    def ua(row, col, v):
        a = s.urey_bradley_atoms.copy(); a[row, col] = v
        return a
    def up(row, col, v):
        a = s.urey_bradley_params.copy(); a[row, col] = v
        return a
    def ia(row, col, v):
        a = s.improper_atoms.copy(); a[row, col] = v
        return a
    def ip(row, col, v):
        a = s.improper_params.copy(); a[row, col] = v
        return a
    return {"ub atom": ("Urey-Bradley term 1: atom index out of range", r(s, urey_bradley_atoms=ua(1, 0, 35))),
            "ub negative atom": ("Urey-Bradley term 0: atom index out of range", r(s, urey_bradley_atoms=ua(0, 1, -1))),
            "ub equal": ("Urey-Bradley term 2: two equal atoms within one term", r(s, urey_bradley_atoms=ua(2, 0, int(s.urey_bradley_atoms[2, 1])))),
            "ub k negative": ("Urey-Bradley term 0: force constant -1 is negative or not finite", r(s, urey_bradley_params=up(0, 1, -1.0))),
            "ub k nan": ("Urey-Bradley term 3: force constant nan is negative or not finite", r(s, urey_bradley_params=up(3, 1, np.nan))),
            "ub r0": ("Urey-Bradley term 0: r0 0 is not a positive length", r(s, urey_bradley_params=up(0, 0, 0.0))),
            "improper atom": ("improper 4: atom index out of range", r(s, improper_atoms=ia(4, 3, 35))),
            "improper equal": ("improper 0: two equal atoms within one term", r(s, improper_atoms=ia(0, 2, int(s.improper_atoms[0, 0])))),
            "improper k inf": ("improper 1: force constant inf is negative or not finite", r(s, improper_params=ip(1, 1, np.inf))),
            "improper k negative": ("improper 1: force constant -2 is negative or not finite", r(s, improper_params=ip(1, 1, -2.0))),
            "improper psi0": (r"improper 2: psi0 3.2 lies outside \[-pi, pi\]", r(s, improper_params=ip(2, 0, 3.2)))}


def bad_systems():
    """{case: (the reason SystemData.check_charmm and the library give, the System)}"""
    return _bad(chamber_divaline())
