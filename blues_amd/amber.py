"""Minimal Amber prmtop / inpcrd readers and the Amber -> OpenMM-unit conversions.

BLUES loads its inputs with ParmEd (reference blues/settings.py:60-90,
`parmed.load_file(prmtop, xyz=inpcrd)`) and turns them into an OpenMM System
with `structure.createSystem(**kwargs)` (reference blues/simulation.py:219).
Neither ParmEd nor OpenMM exists on the MI355X box, so this module restates the
small part of that conversion the switching path needs: per-atom charge / LJ /
mass, bonded terms, exclusions and 1-4 exceptions, HBonds + rigid-water
constraints and hydrogen-mass repartitioning, all in OpenMM units
(nm, kJ/mol, amu, e).  Conversions: SURVEY.md Appendix B.
"""
import re

import numpy as np

from ._abi import NB_NOCUTOFF, NB_PME, NB_PME_DIRECT, SystemData

AMBER_CHARGE = 18.2223
KCAL = 4.184
WATER_NAMES = ("WAT", "HOH", "TIP3", "TP3", "SPC")


def _parse_format(fmt):
    """Fortran format of a prmtop section -> (repeat count, kind, field width).  Besides the counted descriptors of an Amber file
    ((10I8), (5E16.8), (20a4)) chamber writes one without a count -- (a80), under CTITLE: count 1 -- and a mixed one -- (i2,a78), under
    FORCE_FIELD_TYPE: kind "line", width 0, the section's lines are kept as they stand."""
    m = re.match(r"\(?(\d+)([aAiIeEfF])(\d+)(?:\.(\d+))?\)?", fmt.strip())
    if m:
        return int(m.group(1)), m.group(2).lower(), int(m.group(3))
    one = r"\d*[aAiIeEfF]\d+(?:\.\d+)?"
    m = re.fullmatch(r"\(([aAiIeEfF])(\d+)(?:\.(\d+))?\)", fmt.strip())
    if m:
        return 1, m.group(1).lower(), int(m.group(2))
    if re.fullmatch(r"\(%s(?:,%s)+\)" % (one, one), fmt.strip().replace(" ", "")):
        return 1, "line", 0
    raise ValueError("unsupported prmtop format %r" % fmt)


def read_prmtop(path):
    """Returns {FLAG: list or ndarray}."""
    flags = {}
    name, fmt, buf = None, None, []

    def flush():
        if name is None:
            return
        _, kind, width = fmt
        if kind == "line":   # (a mixed descriptor: the lines as strings)
            flags[name] = [line.rstrip("\n") for line in buf]
            return
        items = []
        for line in buf:
            line = line.rstrip("\n")
            for k in range(0, len(line), width):
                tok = line[k:k + width]
                if tok.strip() == "" and kind != "a":
                    continue
                items.append(tok)
        if kind == "i":
            flags[name] = np.array([int(t) for t in items], dtype=np.int64)
        elif kind in "ef":
            flags[name] = np.array([float(t) for t in items], dtype=np.float64)
        else:
            flags[name] = [t.strip() for t in items if t != ""]

    with open(path) as fh:
        for line in fh:
            if line.startswith("%VERSION") or line.startswith("%COMMENT"):
                continue
            if line.startswith("%FLAG"):
                flush()
                name, fmt, buf = line.split()[1], None, []
            elif line.startswith("%FORMAT"):
                fmt = _parse_format(line[len("%FORMAT"):])
            else:
                buf.append(line)
        flush()
    return flags


def read_inpcrd(path):
    """Returns (positions nm (n,3), velocities or None, box nm (3,) or None)."""
    with open(path) as fh:
        lines = fh.read().split("\n")
    natom = int(lines[1].split()[0])
    vals = []
    for line in lines[2:]:
        for k in range(0, len(line.rstrip()), 12):
            tok = line[k:k + 12].strip()
            if tok:
                vals.append(float(tok))
    vals = np.array(vals)
    pos = vals[:3 * natom].reshape(natom, 3) * 0.1
    rest = vals[3 * natom:]
    vel, box = None, None
    if len(rest) >= 3 * natom:
        vel = rest[:3 * natom].reshape(natom, 3) * 0.1 * 20.455  # Amber time unit -> nm/ps
        rest = rest[3 * natom:]
    if len(rest) >= 3:
        box = rest[:3] * 0.1
    return pos, vel, box


def read_rst7(path):
    """Amber restart (.rst7 / .rst) in either form parmed.amber.Rst7 accepts (reference blues/settings.py:76-85): the NetCDF
    "AMBERRESTART" file the reference's own RestartReporter writes (blues/reporters.py:217-225, netcdf=True), recognised by its
    magic bytes, or the ASCII inpcrd layout with a velocity block.  Returns (positions nm, velocities nm/ps or None, box nm or None)."""
    from .formats import AmberNetCDFRestart
    if AmberNetCDFRestart.is_netcdf(path):
        pos, vel, box, _ = AmberNetCDFRestart.read(path)
        return pos, vel, box
    return read_inpcrd(path)


def write_rst7(path, positions_nm, velocities_nm_ps=None, box_nm=None, title="written by blues_amd", time_ps=0.0, netcdf=False):
    """Amber restart: NetCDF (netcdf=True, the reference's choice) or ASCII in the fixed 6F12.7 layout (angstrom; velocities in
    angstrom per 1/20.455 ps)."""
    if netcdf:
        from .formats import AmberNetCDFRestart
        return AmberNetCDFRestart.write(path, positions_nm, velocities_nm_ps, box_nm, time_ps=time_ps, title=title)
    x = np.asarray(positions_nm, dtype=np.float64).reshape(-1, 3) * 10.0
    blocks = [x.reshape(-1)]
    if velocities_nm_ps is not None:
        blocks.append(np.asarray(velocities_nm_ps, dtype=np.float64).reshape(-1) * 10.0 / 20.455)
    with open(path, "w") as fh:
        fh.write(title[:80] + "\n")
        fh.write("%5d%15.7e\n" % (len(x), time_ps) if velocities_nm_ps is not None else "%5d\n" % len(x))
        for b in blocks:
            for k in range(0, len(b), 6):
                fh.write("".join("%12.7f" % v for v in b[k:k + 6]) + "\n")
        if box_nm is not None:
            fh.write("".join("%12.7f" % v for v in list(np.asarray(box_nm, dtype=np.float64).reshape(-1)[:3] * 10.0) + [90.0, 90.0, 90.0]) + "\n")


def ewald_alpha(cutoff, tolerance):
    """OpenMM: alpha = sqrt(-ln(2 tol)) / cutoff (2.145966 for 0.005 at 1 nm)."""
    return float(np.sqrt(-np.log(2.0 * tolerance)) / cutoff)


def cmap_from_prmtop(prm, natom=None):
    """The CMAP sections of a prmtop -> (maps, torsions) as SystemData.cmap_maps / .cmap_torsions hold them; ((), empty) without them.

    Sections CMAP_COUNT, CMAP_RESOLUTION, CMAP_PARAMETER_NN, CMAP_INDEX (Amber ff19SB) or the same names prefixed CHARMM_ (chamber).
    The layout is recalled from ParmEd, not source-pinned: CMAP_COUNT = (terms, types); CMAP_INDEX holds six integers
    per term, five 1-based atom numbers and a 1-based type; a parameter section holds res^2 values in kcal/mol, phi the slow index,
    both angles starting at -180 degrees.  OpenMM's maps start at 0: E[i, j] = 4.184 G[(i + res/2) mod res][(j + res/2) mod res].
    The five atoms a1..a5 become the torsion (a1, a2, a3, a4, a2, a3, a4, a5).  ValueError, with the reason, for an odd resolution,
    counts that do not match the sections and a type or atom out of range."""
    empty = ((), np.zeros((0, 9), np.int32))
    prefix = None
    for cand in ("", "CHARMM_"):
        if cand + "CMAP_COUNT" in prm:
            prefix = cand
            break
    if prefix is None:
        return empty
    count = np.asarray(prm[prefix + "CMAP_COUNT"]).reshape(-1)
    if len(count) != 2:
        raise ValueError("%sCMAP_COUNT holds %d values, not (terms, types)" % (prefix, len(count)))
    nterm, ntype = int(count[0]), int(count[1])
    res = np.asarray(prm.get(prefix + "CMAP_RESOLUTION", ())).reshape(-1)
    if len(res) != ntype:
        raise ValueError("%sCMAP_COUNT names %d types but %sCMAP_RESOLUTION holds %d" % (prefix, ntype, prefix, len(res)))
    maps = []
    for k in range(ntype):
        n = int(res[k])
        if n % 2:
            raise ValueError("CMAP type %d: odd resolution %d (a map that starts at -180 degrees cannot be shifted to start at 0)" % (k + 1, n))
        name = "%sCMAP_PARAMETER_%02d" % (prefix, k + 1)
        g = np.asarray(prm.get(name, ()), dtype=np.float64).reshape(-1)
        if len(g) != n * n:
            raise ValueError("%s holds %d values, resolution %d needs %d" % (name, len(g), n, n * n))
        shift = (np.arange(n) + n // 2) % n
        maps.append(KCAL * g.reshape(n, n)[np.ix_(shift, shift)])
    index = np.asarray(prm.get(prefix + "CMAP_INDEX", ()), dtype=np.int64).reshape(-1)
    if len(index) != 6 * nterm:
        raise ValueError("%sCMAP_COUNT names %d terms but %sCMAP_INDEX holds %d integers (six per term)" % (prefix, nterm, prefix, len(index)))
    index = index.reshape(-1, 6)
    tors = np.zeros((nterm, 9), np.int32)
    for t, row in enumerate(index):
        if row[5] < 1 or row[5] > ntype:
            raise ValueError("CMAP term %d: type %d of %d" % (t + 1, row[5], ntype))
        a = row[:5] - 1
        if np.any(a < 0) or (natom is not None and np.any(a >= natom)):
            raise ValueError("CMAP term %d: atom out of range" % (t + 1))
        tors[t] = (row[5] - 1, a[0], a[1], a[2], a[3], a[1], a[2], a[3], a[4])
    return tuple(maps), tors


def is_chamber(prm):
    """A topology written by chamber (CHARMM force field in prmtop form): it carries FORCE_FIELD_TYPE, CTITLE or a CHARMM_* section."""
    return "FORCE_FIELD_TYPE" in prm or "CTITLE" in prm or any(str(k).startswith("CHARMM_") for k in prm)


def charmm_from_prmtop(prm, natom=None):
    """The Urey-Bradley and improper sections of a chamber prmtop -> (urey_bradley_atoms, urey_bradley_params, improper_atoms,
    improper_params) as SystemData holds them; four empty arrays without them.

    The layout is recalled from ParmEd, not source-pinned: CHARMM_UREY_BRADLEY_COUNT = (terms, types);
    CHARMM_UREY_BRADLEY holds three integers per term, two 1-based ATOM NUMBERS (not the coordinate offsets of BONDS_*) and a 1-based
    type; CHARMM_UREY_BRADLEY_FORCE_CONSTANT in kcal/mol/A^2 and _EQUIL_VALUE in A.  CHARMM writes K (S - S0)^2, stored here as OpenMM's
    0.5 k (r - r0)^2: r0 = 0.1 S0, k = 2 K 4.184 100.  CHARMM_NUM_IMPROPERS, CHARMM_NUM_IMPR_TYPES; CHARMM_IMPROPERS holds five integers
    per term, four 1-based atom numbers and a 1-based type; CHARMM_IMPROPER_FORCE_CONSTANT in kcal/mol/rad^2 and _PHASE in degrees:
    E = k (psi - psi0)^2 with k = 4.184 K, psi0 in radians.  ValueError, with the reason, for counts that do not match the sections,
    a type or atom out of range and two equal atoms within one term."""
    def ints(name):
        return np.asarray(prm.get(name, ()), dtype=np.int64).reshape(-1)

    def floats(name):
        return np.asarray(prm.get(name, ()), dtype=np.float64).reshape(-1)

    def section(label, index_name, width, nterm, ntype, const_names):
        consts = [floats(c) for c in const_names]
        for c, name in zip(consts, const_names):
            if len(c) != ntype:
                raise ValueError("%s: %d types are announced but %s holds %d values" % (label, ntype, name, len(c)))
        index = ints(index_name)
        if len(index) != (width + 1) * nterm:
            raise ValueError("%s: %d terms are announced but %s holds %d integers (%d per term)" % (label, nterm, index_name, len(index), width + 1))
        index = index.reshape(-1, width + 1)
        for t, row in enumerate(index):
            if row[width] < 1 or row[width] > ntype:
                raise ValueError("%s %d: type %d of %d" % (label, t + 1, row[width], ntype))
            a = row[:width] - 1
            if np.any(a < 0) or (natom is not None and np.any(a >= natom)):
                raise ValueError("%s %d: atom out of range" % (label, t + 1))
            if len(set(int(v) for v in a)) != width:
                raise ValueError("%s %d: two equal atoms within one term" % (label, t + 1))
        return (index[:, :width] - 1).astype(np.int32), index[:, width] - 1, consts

    ub_atoms, ub_params = np.zeros((0, 2), np.int32), np.zeros((0, 2))
    if "CHARMM_UREY_BRADLEY_COUNT" in prm or "CHARMM_UREY_BRADLEY" in prm:
        count = ints("CHARMM_UREY_BRADLEY_COUNT")
        if len(count) != 2:
            raise ValueError("CHARMM_UREY_BRADLEY_COUNT holds %d values, not (terms, types)" % len(count))
        ub_atoms, ty, (kk, s0) = section("Urey-Bradley term", "CHARMM_UREY_BRADLEY", 2, int(count[0]), int(count[1]),
                                         ("CHARMM_UREY_BRADLEY_FORCE_CONSTANT", "CHARMM_UREY_BRADLEY_EQUIL_VALUE"))
        ub_params = np.stack([0.1 * s0[ty], 2.0 * kk[ty] * KCAL * 100.0], axis=1).reshape(-1, 2)
    im_atoms, im_params = np.zeros((0, 4), np.int32), np.zeros((0, 2))
    if "CHARMM_NUM_IMPROPERS" in prm or "CHARMM_IMPROPERS" in prm:
        nterm, ntype = ints("CHARMM_NUM_IMPROPERS"), ints("CHARMM_NUM_IMPR_TYPES")
        if len(nterm) != 1 or len(ntype) != 1:
            raise ValueError("CHARMM_NUM_IMPROPERS / CHARMM_NUM_IMPR_TYPES hold %d and %d values, not one each" % (len(nterm), len(ntype)))
        im_atoms, ty, (kk, ph) = section("improper", "CHARMM_IMPROPERS", 4, int(nterm[0]), int(ntype[0]),
                                         ("CHARMM_IMPROPER_FORCE_CONSTANT", "CHARMM_IMPROPER_PHASE"))
        im_params = np.stack([np.deg2rad(ph[ty]), KCAL * kk[ty]], axis=1).reshape(-1, 2)
    return ub_atoms.reshape(-1, 2), ub_params, im_atoms.reshape(-1, 4), im_params


def _refuse_nbfix(prm, ntypes):
    """ValueError naming the type pair whose off-diagonal entry of the main Lennard-Jones table is not the Lorentz-Berthelot combination
    of the diagonal ones (Rmin arithmetic mean, eps geometric mean) to 1e-6 relative: a CHARMM NBFIX, which per-atom sigma / epsilon
    cannot represent.  (The table is written with eight significant digits.)"""
    nbidx, acoef, bcoef = prm["NONBONDED_PARM_INDEX"], prm["LENNARD_JONES_ACOEF"], prm["LENNARD_JONES_BCOEF"]
    rmin, eps = np.zeros(ntypes), np.zeros(ntypes)
    for t in range(ntypes):
        k = int(nbidx[ntypes * t + t]) - 1
        if k >= 0 and acoef[k] != 0.0 and bcoef[k] != 0.0:
            rmin[t], eps[t] = (2.0 * acoef[k] / bcoef[k]) ** (1.0 / 6.0), bcoef[k] ** 2 / (4.0 * acoef[k])
    names = {}
    for i, t in enumerate(np.asarray(prm.get("ATOM_TYPE_INDEX", ()))):
        if "AMBER_ATOM_TYPE" in prm and int(t) - 1 not in names:
            names[int(t) - 1] = prm["AMBER_ATOM_TYPE"][i]
    for a in range(ntypes):
        for b in range(a + 1, ntypes):
            k = int(nbidx[ntypes * a + b]) - 1
            if k < 0:
                continue
            e, r6 = np.sqrt(eps[a] * eps[b]), (0.5 * (rmin[a] + rmin[b])) ** 6
            for got, want, which in ((acoef[k], e * r6 * r6, "ACOEF"), (bcoef[k], 2.0 * e * r6, "BCOEF")):
                if abs(got - want) > 1e-6 * max(abs(got), abs(want)):
                    raise ValueError("NBFIX: LENNARD_JONES_%s of the type pair (%d, %d)%s is %.8e, the Lorentz-Berthelot combination of the "
                                     "types' own entries gives %.8e; per-atom sigma / epsilon cannot represent a pair-specific entry"
                                     % (which, a + 1, b + 1, " [%s, %s]" % (names[a], names[b]) if a in names and b in names else "", got, want))


def system_from_amber(prm, positions, box, cutoff=1.0, ewald_error_tolerance=0.005, constraints="HBonds",
                      rigid_water=True, hydrogen_mass=None, remove_cm_motion=True, alchemical_atoms=(),
                      tip3p_for_untyped_water=True, reciprocal_space=True, dispersion_correction=True, nonbonded_method="PME",
                      implicit_solvent=None, solute_dielectric=1.0, solvent_dielectric=78.5, implicit_solvent_kappa=None,
                      implicit_solvent_salt_conc=None, alchemical_pme_treatment="direct-space", switch_distance=None):
    """Amber topology -> SystemData, following structure.createSystem's kwargs
    (reference examples/rotmove_cuda.yml:19-27: PME, 10 A cutoff, HBonds,
    rigidWater, removeCMMotion, hydrogenMass 3.024, ewaldErrorTolerance 0.005).
    Constrained bonds and rigid-water angles are left out of the harmonic terms
    (they contribute zero at the constrained geometry).
    reciprocal_space=True is nonbondedMethod=PME in full (mesh of OpenMM's Reference platform for the tolerance, self term,
    excluded-pair corrections, dispersion correction); False keeps the direct-space sum only and says so in the log --
    forces on the water then differ from the reference's, only the protocol work (lambda-dependent pairs) does not.
    nonbonded_method="NoCutoff" (vacuum, reference blues/tests/test_sidechain.py:42): every pair counts, no cutoff, no periodicity,
    no mesh and no dispersion correction; `box` may be None (the box is then stored as zeros and has no effect).
    implicit_solvent="OBC1" | "OBC2" (createSystem(implicitSolvent=app.OBC1 / app.OBC2, soluteDielectric, solventDielectric), reference
    blues/simulation.py:139-219): GB-OBC with the ACE surface term on a NoCutoff System, radii from %FLAG RADII and scale factors
    from %FLAG SCREEN.  HCT, GBn, GBn2 and salt screening (kappa, a salt concentration) are not implemented and raise.
    alchemical_pme_treatment="direct-space" | "exact" (SystemFactory.generateAlchSystem(..., alchemical_pme_treatment=...), reference
    blues/simulation.py:236, 274-284): how full PME treats the alchemical charges; "exact" needs reciprocal space.  'coulomb' raises.
    switch_distance (nm; createSystem(switchDistance=...), reference blues/simulation.py:157-161, blues/settings.py:155): the Lennard-Jones
    switching function between it and the cutoff.  None, 0 or a value >= the cutoff: no switch; on a NoCutoff System it is stored and
    has no effect.  Negative or not finite raises."""
    from ._abi import alchemical_pme_treatment_code
    alchemical_pme_treatment_code(alchemical_pme_treatment)
    if nonbonded_method not in ("PME", "NoCutoff"):
        raise ValueError("nonbonded_method must be 'PME' or 'NoCutoff', got %r" % (nonbonded_method,))
    no_cutoff = nonbonded_method == "NoCutoff"
    gb = None
    if implicit_solvent is not None:
        from ._abi import GB_MODELS, ImplicitSolventData
        name = getattr(implicit_solvent, "name", implicit_solvent)
        if name not in GB_MODELS:
            raise ValueError("implicit_solvent %r is not supported: the engine implements 'OBC1' and 'OBC2' (not HCT, GBn or GBn2)" % (implicit_solvent,))
        if implicit_solvent_kappa is not None or implicit_solvent_salt_conc is not None:
            raise ValueError("salt screening (implicit_solvent_kappa, implicit_solvent_salt_conc) is not supported: the engine implements "
                             "'OBC1' and 'OBC2' without it")
        if not no_cutoff:
            raise ValueError("implicit_solvent needs nonbonded_method='NoCutoff': GB has no periodic or cutoff form here")
        if "RADII" not in prm or "SCREEN" not in prm:
            raise ValueError("implicit_solvent needs the %FLAG RADII and %FLAG SCREEN sections of the prmtop")
        gb = ImplicitSolventData(GB_MODELS[name], np.asarray(prm["RADII"], dtype=np.float64) * 0.1, np.asarray(prm["SCREEN"], dtype=np.float64).copy(),
                                 float(solute_dielectric), float(solvent_dielectric))
    elif implicit_solvent_kappa is not None or implicit_solvent_salt_conc is not None:
        raise ValueError("implicit_solvent_kappa / implicit_solvent_salt_conc without implicit_solvent (and salt screening is not supported: "
                         "the engine implements 'OBC1' and 'OBC2' without it)")
    if box is None:
        if not no_cutoff:
            raise ValueError("a periodic System (nonbonded_method='PME') needs a box")
        box = np.zeros(3)
    p = prm["POINTERS"]
    natom, ntypes = int(p[0]), int(p[1])
    charge = prm["CHARGE"] / AMBER_CHARGE
    mass = prm["MASS"].copy()
    atnum = prm.get("ATOMIC_NUMBER")
    if atnum is None:
        atnum = np.where(mass < 1.5, 1, 6)
    tidx = prm["ATOM_TYPE_INDEX"]
    nbidx = prm["NONBONDED_PARM_INDEX"]
    acoef, bcoef = prm["LENNARD_JONES_ACOEF"], prm["LENNARD_JONES_BCOEF"]
    chamber = is_chamber(prm)
    if chamber:   # (1-4 pairs from the topology's own table; a non-chamber prmtop takes the path it always took)
        _refuse_nbfix(prm, ntypes)
    table14 = chamber and "LENNARD_JONES_14_ACOEF" in prm and "LENNARD_JONES_14_BCOEF" in prm   # (without the table: the diagonal entries, as for Amber)
    if table14:
        acoef14, bcoef14 = prm["LENNARD_JONES_14_ACOEF"], prm["LENNARD_JONES_14_BCOEF"]
        if len(acoef14) != len(acoef) or len(bcoef14) != len(bcoef):
            raise ValueError("LENNARD_JONES_14_ACOEF / _BCOEF hold %d and %d values, the main table %d" % (len(acoef14), len(bcoef14), len(acoef)))
    res_ptr = list(prm["RESIDUE_POINTER"] - 1) + [natom]
    res_lab = prm["RESIDUE_LABEL"]
    residue_of_atom = np.zeros(natom, dtype=np.int32)
    for r in range(len(res_lab)):
        residue_of_atom[res_ptr[r]:res_ptr[r + 1]] = r
    is_water_res = np.array([lab in WATER_NAMES for lab in res_lab])
    is_water = is_water_res[residue_of_atom]

    if gb is not None and tip3p_for_untyped_water:
        # water written without types carries no GB parameters either (RADII = SCREEN = 0): it gets what tleap's mbondi set gives a
        # water molecule [recalled: O 1.5 A, H bonded to O 0.8 A; screen 0.85 for both], as it gets TIP3P's Lennard-Jones below
        blank = is_water & (gb.radius == 0.0) & (gb.scale == 0.0)
        gb.radius[blank] = np.where(atnum[blank] == 8, 0.15, 0.08)
        gb.scale[blank] = 0.85
    sigma = np.zeros(natom)
    eps = np.zeros(natom)
    for i in range(natom):
        t = int(tidx[i])
        if t <= 0:
            if not (tip3p_for_untyped_water and is_water[i]):
                raise ValueError("atom %d has no LJ type" % i)
            if atnum[i] == 8:  # TIP3P oxygen
                sigma[i], eps[i] = 0.315075, 0.635968
            else:
                sigma[i], eps[i] = 0.1, 0.0
            continue
        k = int(nbidx[ntypes * (t - 1) + (t - 1)]) - 1
        a, b = acoef[k], bcoef[k]
        if a == 0.0 or b == 0.0:
            sigma[i], eps[i] = 0.1, 0.0
        else:
            sigma[i] = (a / b) ** (1.0 / 6.0) * 0.1
            eps[i] = b * b / (4.0 * a) * KCAL

    def triples(name, width):
        arr = prm.get(name)
        if arr is None or len(arr) == 0:
            return np.zeros((0, width), dtype=np.int64)
        return np.asarray(arr).reshape(-1, width)

    bonds = np.vstack([triples("BONDS_INC_HYDROGEN", 3), triples("BONDS_WITHOUT_HYDROGEN", 3)])
    angles = np.vstack([triples("ANGLES_INC_HYDROGEN", 4), triples("ANGLES_WITHOUT_HYDROGEN", 4)])
    dihs = np.vstack([triples("DIHEDRALS_INC_HYDROGEN", 5), triples("DIHEDRALS_WITHOUT_HYDROGEN", 5)])
    bk, br = prm["BOND_FORCE_CONSTANT"], prm["BOND_EQUIL_VALUE"]
    ak, at = prm["ANGLE_FORCE_CONSTANT"], prm["ANGLE_EQUIL_VALUE"]
    dk, dn, dp = prm["DIHEDRAL_FORCE_CONSTANT"], prm["DIHEDRAL_PERIODICITY"], prm["DIHEDRAL_PHASE"]
    scee = prm.get("SCEE_SCALE_FACTOR", np.full(len(dk), 1.0 if table14 else 1.2))
    scnb = prm.get("SCNB_SCALE_FACTOR", np.full(len(dk), 1.0 if table14 else 2.0))

    # hydrogen mass repartitioning (createSystem(hydrogenMass=...))
    if hydrogen_mass is not None:
        for b in bonds:
            i, j = int(b[0]) // 3, int(b[1]) // 3
            if atnum[i] == 1:
                i, j = j, i
            if atnum[j] == 1 and atnum[i] != 1:
                transfer = hydrogen_mass - mass[j]
                mass[j] = hydrogen_mass
                mass[i] -= transfer

    cons_atoms, cons_dist = [], []
    bond_atoms, bond_params = [], []
    constrained_pair = set()
    for b in bonds:
        i, j, t = int(b[0]) // 3, int(b[1]) // 3, int(b[2]) - 1
        r0, k = br[t] * 0.1, 2.0 * bk[t] * KCAL * 100.0
        has_h = atnum[i] == 1 or atnum[j] == 1
        water = is_water[i] and is_water[j]
        if (constraints in ("HBonds", "AllBonds", "HAngles") and has_h) or constraints in ("AllBonds", "HAngles") or (rigid_water and water):
            cons_atoms.append((i, j)); cons_dist.append(r0)
            constrained_pair.add((min(i, j), max(i, j)))
        else:
            bond_atoms.append((i, j)); bond_params.append((r0, k))
    angle_atoms, angle_params = [], []
    bond_dist = {frozenset(p_): d for p_, d in zip(cons_atoms, cons_dist)}   # (the constrained bonds; the 1-3 constraints below are not bonds)

    def constrain_13(i, j, k_, th0):
        """the 1-3 distance that the constrained bonds i-j, k-j and the equilibrium angle fix, once per pair"""
        pair = (min(i, k_), max(i, k_))
        if pair not in constrained_pair:
            d_ij, d_kj = bond_dist[frozenset((i, j))], bond_dist[frozenset((k_, j))]
            cons_atoms.append((i, k_)); cons_dist.append(float(np.sqrt(d_ij ** 2 + d_kj ** 2 - 2 * d_ij * d_kj * np.cos(th0))))
            constrained_pair.add(pair)

    for a in angles:
        i, j, k_, t = int(a[0]) // 3, int(a[1]) // 3, int(a[2]) // 3, int(a[3]) - 1
        th0, kk = at[t], 2.0 * ak[t] * KCAL
        if rigid_water and is_water[i] and is_water[j] and is_water[k_]:
            constrain_13(i, j, k_, th0)  # H-H distance from the two O-H bonds and the angle
            continue
        # HAngles (OpenMM): on top of AllBonds, every angle H-X-H and every angle H-O-X becomes the 1-3 distance that the two bond
        # lengths and the equilibrium angle fix, and leaves the harmonic terms; hydrogens by atomic number (repartitioned masses hide them)
        if constraints == "HAngles" and ((atnum[i] == 1 and atnum[k_] == 1) or (atnum[j] == 8 and (atnum[i] == 1 or atnum[k_] == 1))):
            constrain_13(i, j, k_, th0)
            continue
        angle_atoms.append((i, j, k_)); angle_params.append((th0, kk))
    tors_atoms, tors_params = [], []
    exc = {}
    for d in dihs:
        i, j, k_, l, t = int(d[0]) // 3, int(d[1]) // 3, abs(int(d[2])) // 3, abs(int(d[3])) // 3, int(d[4]) - 1
        if dk[t] != 0.0:
            tors_atoms.append((i, j, k_, l)); tors_params.append((round(abs(dn[t])), dp[t], dk[t] * KCAL))
        if int(d[2]) >= 0 and int(d[3]) >= 0:  # carries a 1-4 interaction
            pair = (min(i, l), max(i, l))
            if pair not in exc and table14:   # CHARMM's own 1-4 table, indexed like the main one
                ti, tl = int(tidx[i]), int(tidx[l])
                if ti <= 0 or tl <= 0:
                    raise ValueError("1-4 pair (%d, %d): an atom without a Lennard-Jones type" % (i, l))
                k14 = int(nbidx[ntypes * (ti - 1) + (tl - 1)]) - 1
                a14, b14 = (acoef14[k14], bcoef14[k14]) if k14 >= 0 else (0.0, 0.0)
                qq = charge[i] * charge[l] / (scee[t] if scee[t] != 0 else 1.0)
                if a14 == 0.0 or b14 == 0.0:
                    exc[pair] = (qq, 0.1, 0.0)
                else:
                    exc[pair] = (qq, 0.1 * (a14 / b14) ** (1.0 / 6.0), KCAL * b14 * b14 / (4.0 * a14) / (scnb[t] if scnb[t] != 0 else 1.0))
            elif pair not in exc:
                qq = charge[i] * charge[l] / (scee[t] if scee[t] != 0 else 1.2)
                e14 = np.sqrt(eps[i] * eps[l]) / (scnb[t] if scnb[t] != 0 else 2.0)
                exc[pair] = (qq, 0.5 * (sigma[i] + sigma[l]), e14)

    excl = set()
    nex, exl = prm["NUMBER_EXCLUDED_ATOMS"], prm["EXCLUDED_ATOMS_LIST"]
    pos_ = 0
    for i in range(natom):
        for q in range(int(nex[i])):
            j = int(exl[pos_ + q]) - 1
            if j >= 0:
                excl.add((min(i, j), max(i, j)))
        pos_ += int(nex[i])
    excl |= set(exc.keys()) | constrained_pair
    excl = np.array(sorted(excl), dtype=np.int32).reshape(-1, 2)
    exc_pairs = sorted(exc.keys())

    alpha = ewald_alpha(cutoff, ewald_error_tolerance)
    if no_cutoff:
        method, grid, alpha, dispersion_correction = NB_NOCUTOFF, (0, 0, 0), 0.0, False
    elif reciprocal_space:
        from .systems import pme_grid_for
        method, grid = NB_PME, pme_grid_for(box, alpha, cutoff, ewald_error_tolerance)
    else:
        import logging
        logging.getLogger(__name__).warning("system_from_amber: PME lowered to its direct-space part (reciprocal_space=False): no mesh, self or "
                                            "dispersion terms; energies and environment forces are not those of nonbondedMethod=PME")
        method, grid = NB_PME_DIRECT, (0, 0, 0)
    system = SystemData(
        pme_grid=grid, pme_order=5, dispersion_correction=bool(dispersion_correction),
        box=np.asarray(box, dtype=np.float64), mass=mass, charge=charge, sigma=sigma, epsilon=eps,
        exclusions=excl,
        exception_atoms=np.array(exc_pairs, dtype=np.int32).reshape(-1, 2),
        exception_params=np.array([exc[p_] for p_ in exc_pairs], dtype=np.float64).reshape(-1, 3),
        bond_atoms=np.array(bond_atoms, dtype=np.int32).reshape(-1, 2), bond_params=np.array(bond_params).reshape(-1, 2),
        angle_atoms=np.array(angle_atoms, dtype=np.int32).reshape(-1, 3), angle_params=np.array(angle_params).reshape(-1, 2),
        torsion_atoms=np.array(tors_atoms, dtype=np.int32).reshape(-1, 4), torsion_params=np.array(tors_params, dtype=np.float64).reshape(-1, 3),
        constraint_atoms=np.array(cons_atoms, dtype=np.int32).reshape(-1, 2), constraint_dist=np.array(cons_dist, dtype=np.float64),
        alchemical_atoms=np.array(sorted(alchemical_atoms), dtype=np.int32),
        nonbonded_method=method, cutoff=cutoff, ewald_alpha=alpha,
        remove_cm_motion=remove_cm_motion, positions=np.asarray(positions, dtype=np.float64),
        residue_of_atom=residue_of_atom, names=list(prm.get("ATOM_NAME", [])),
        implicit_solvent=gb, alchemical_pme_treatment=alchemical_pme_treatment,
        switch_distance=0.0 if switch_distance is None else float(switch_distance),
    )
    system.check_switch_distance()
    system.cmap_maps, system.cmap_torsions = cmap_from_prmtop(prm, natom)   # (CMAPTorsionForce of ff19SB / chamber topologies)
    system.check_cmap()
    if chamber:   # (HarmonicBondForce of the Urey-Bradley terms, CustomTorsionForce of the impropers)
        system.urey_bradley_atoms, system.urey_bradley_params, system.improper_atoms, system.improper_params = charmm_from_prmtop(prm, natom)
    system.check_charmm()
    system.check_implicit_solvent()
    system.check_alchemical_pme_treatment()
    return system
