"""ctypes mirror of include/blues_engine.h (the C-ABI structs and prototypes).

Both the product library (libblues_hip.so) and the test-only CPU oracle
(oracle/_build/libblues_oracle.so) consume the same two descriptor structs, so
this module only describes the ABI; it never loads the oracle.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

ABI_VERSION = 9
SWITCH_NONE, SWITCH_VV, SWITCH_GHMC = 0, 1, 2
NB_NOCUTOFF = 0
NB_PME_DIRECT = 1
NB_PME = 2
PAIR_STANDARD, PAIR_ETHYLENE = 0, 1      # BluesSystemDesc.custom_pair_mode
MAX_CENTROID_BONDS, MAX_CENTROID_GROUP = 4, 8
GB_NONE, GB_OBC1, GB_OBC2 = 0, 1, 2        # BluesImplicitSolventDesc.model
GB_MODELS = {"OBC1": GB_OBC1, "OBC2": GB_OBC2}
GB_RADIUS_OFFSET = 0.009                   # nm (OpenMM's GBSAOBCForce dielectric offset)
GB_SURFACE_AREA_ENERGY = 2.25936           # kJ/mol/nm^2 (OpenMM's default)
N_ENERGY_TERMS = 10
N_STATS = 22
N_BATCH_COUNTERS = 15
ENERGY_TERM_NAMES = ("bonds", "angles", "torsions", "nonbonded", "exceptions", "alch_sterics",
                     "alch_electrostatics", "restraint", "reciprocal", "dispersion_correction")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class BluesSystemDesc(C.Structure):
    _fields_ = [
        ("n_atoms", C.c_int32),
        ("box", C.c_double * 9),
        ("mass", _dp), ("charge", _dp), ("sigma", _dp), ("epsilon", _dp),
        ("n_exclusions", C.c_int32), ("exclusions", _ip),
        ("n_exceptions", C.c_int32), ("exception_atoms", _ip), ("exception_params", _dp),
        ("n_bonds", C.c_int32), ("bond_atoms", _ip), ("bond_params", _dp),
        ("n_angles", C.c_int32), ("angle_atoms", _ip), ("angle_params", _dp),
        ("n_torsions", C.c_int32), ("torsion_atoms", _ip), ("torsion_params", _dp),
        ("n_constraints", C.c_int32), ("constraint_atoms", _ip), ("constraint_dist", _dp),
        ("n_alchemical", C.c_int32), ("alchemical_atoms", _ip),
        ("n_restraints", C.c_int32), ("restraint_atoms", _ip), ("restraint_x0", _dp), ("restraint_k", C.c_double),
        ("nonbonded_method", C.c_int32),
        ("cutoff", C.c_double), ("ewald_alpha", C.c_double), ("softcore_alpha", C.c_double),
        ("annihilate_electrostatics", C.c_int32), ("annihilate_sterics", C.c_int32),
        ("remove_cm_motion", C.c_int32),
        ("pme_grid", C.c_int32 * 3), ("pme_order", C.c_int32), ("dispersion_correction", C.c_int32),
        ("custom_pair_mode", C.c_int32), ("n_centroid_bonds", C.c_int32),
        ("centroid_group_start", _ip), ("centroid_atoms", _ip), ("centroid_weights", _dp), ("centroid_k", _dp),
    ]


class BluesIntegratorDesc(C.Structure):
    _fields_ = [
        ("timestep", C.c_double), ("temperature", C.c_double), ("collision_rate", C.c_double),
        ("nsteps_neq", C.c_int32), ("nprop", C.c_int32),
        ("prop_lambda_min", C.c_double), ("prop_lambda_max", C.c_double),
        ("splitting", C.c_char_p),
        ("n_lambda_steps", C.c_int32),
        ("lambda_sterics", _dp), ("lambda_electrostatics", _dp),
        ("constraint_tolerance", C.c_double),
        ("seed", C.c_uint64), ("replica", C.c_int32), ("precision", C.c_int32),
        ("switching_mode", C.c_int32), ("steps_per_propagation", C.c_int32),
        ("measure_shadow_work", C.c_int32), ("measure_heat", C.c_int32),
    ]


class BluesImplicitSolventDesc(C.Structure):
    _fields_ = [
        ("model", C.c_int32),
        ("solute_dielectric", C.c_double), ("solvent_dielectric", C.c_double),
        ("surface_area_energy", C.c_double),
        ("radius", _dp), ("scale", _dp),
    ]


class BluesSystemExt(C.Structure):
    """include/blues_engine.h: BluesSystemExt (additive System options; blues_engine_create_ext)."""
    _fields_ = [("struct_size", C.c_int32), ("alchemical_pme_treatment", C.c_int32),
                ("n_cmap_maps", C.c_int32), ("cmap_size", _ip), ("cmap_energy", _dp),
                ("n_cmap_torsions", C.c_int32), ("cmap_torsion_map", _ip), ("cmap_torsion_atoms", _ip)]


class BluesSystemExtV3(C.Structure):
    """include/blues_engine.h: BluesSystemExtV3 (BluesSystemExt grown at its end by the CHARMM terms; passed to blues_engine_create_ext
    in BluesSystemExt's place with struct_size = its own size)."""
    _fields_ = BluesSystemExt._fields_ + [("n_urey_bradley", C.c_int32), ("urey_bradley_atoms", _ip), ("urey_bradley_params", _dp),
                                          ("n_impropers", C.c_int32), ("improper_atoms", _ip), ("improper_params", _dp)]


class BluesSystemExtV4(C.Structure):
    """include/blues_engine.h: BluesSystemExtV4 (BluesSystemExtV3 grown at its end by the Lennard-Jones switch distance; passed in
    BluesSystemExt's place with struct_size = its own size)."""
    _fields_ = BluesSystemExtV3._fields_ + [("lj_switch_distance", C.c_double), ("lj_switch_reserved", C.c_double)]


SYSTEM_EXT_SIZE_V1 = 8                     # a caller from before the CMAP fields: struct_size, alchemical_pme_treatment
SYSTEM_EXT_SIZE_V2 = C.sizeof(BluesSystemExt)   # BLUES_SYSTEM_EXT_SIZE_V2: a caller with maps but no Urey-Bradley terms or impropers
CMAP_MIN_SIZE, CMAP_MAX_SIZE = 4, 64       # BLUES_CMAP_MIN_SIZE / BLUES_CMAP_MAX_SIZE


# SystemData.alchemical_pme_treatment -> BluesSystemExt.alchemical_pme_treatment (BLUES_ALCH_PME_*)
ALCHEMICAL_PME_TREATMENTS = {"direct-space": 0, "exact": 1}


def alchemical_pme_treatment_code(name):
    """BLUES_ALCH_PME_* of openmmtools' alchemical_pme_treatment name; ValueError for anything but the two supported values."""
    if not isinstance(name, str) or name not in ALCHEMICAL_PME_TREATMENTS:
        raise ValueError("alchemical_pme_treatment %r is not supported: the engine implements 'direct-space' and 'exact'" % (name,))
    return ALCHEMICAL_PME_TREATMENTS[name]


class BluesMinimizeDesc(C.Structure):
    """include/blues_engine.h: BluesMinimizeDesc (the constants of the device-resident FIRE minimiser)."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("dt0", C.c_double), ("dt_max", C.c_double), ("f_inc", C.c_double), ("f_dec", C.c_double),
        ("alpha0", C.c_double), ("f_alpha", C.c_double), ("max_step", C.c_double),
        ("n_min", C.c_int32),
    ]


class BluesMinimizeResult(C.Structure):
    _fields_ = [
        ("converged", C.c_int32), ("iterations", C.c_int32), ("n_pos", C.c_int32), ("pad", C.c_int32),
        ("fmax", C.c_double), ("dt", C.c_double), ("alpha", C.c_double), ("e_initial", C.c_double), ("e_final", C.c_double),
    ]

    def as_dict(self):
        return {"converged": int(self.converged), "iterations": int(self.iterations), "n_pos": int(self.n_pos), "fmax": float(self.fmax),
                "dt": float(self.dt), "alpha": float(self.alpha), "e_initial": float(self.e_initial), "e_final": float(self.e_final)}


MINIMIZE_FIELDS = ("dt0", "dt_max", "f_inc", "f_dec", "alpha0", "f_alpha", "max_step", "n_min")
# additive entry points (BLUES_ABI_VERSION unchanged): a library built before them loads, and the wrappers that need them say so
MINIMIZE_SYMBOLS = ("blues_minimize_default", "blues_minimize", "blues_batch_minimize")
OPTIONAL_SYMBOLS = MINIMIZE_SYMBOLS + ("blues_engine_create_ext", "blues_get_exact_pme_path", "blues_get_pme_path", "blues_get_alchemical_layout", "blues_get_cmap_angles", "blues_get_lj_switch")


class BluesTuning(C.Structure):
    """include/blues_engine.h: BluesTuning (launch-policy overrides; the library reads no environment variables)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("plain_skin", C.c_int32),
        ("skin", C.c_double), ("prune_margin", C.c_double), ("jcap_scale", C.c_double), ("acap_scale", C.c_double),
        ("k1_mode", C.c_int32), ("list_group", C.c_int32), ("sub_iw", C.c_int32), ("sub_chunks", C.c_int32),
        ("seg_len", C.c_int32), ("waves_per_block", C.c_int32), ("k2_jiter", C.c_int32),
        ("fuse_forces", C.c_int32), ("fast_step", C.c_int32), ("fork", C.c_int32),
        ("batch_sync_lists", C.c_int32), ("force_lists", C.c_int32), ("no_sphere", C.c_int32),
        ("pme_general", C.c_int32), ("debug_lists", C.c_int32), ("assume_batch", C.c_int32), ("k1_threads", C.c_int32),
        ("k2_dense", C.c_int32), ("fuse_finalize", C.c_int32), ("host_threads", C.c_int32),
        ("pack_clusters", C.c_int32),
    ]


def _f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        a = a.reshape(shape)
    return a


def _i32(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    if shape is not None:
        a = a.reshape(shape)
    return a


@dataclass
class ImplicitSolventData:
    """GB-OBC implicit solvent of a NoCutoff System (BluesImplicitSolventDesc in include/blues_engine.h)."""
    model: int                           # GB_OBC1 / GB_OBC2
    radius: np.ndarray                   # [n] nm (prmtop RADII)
    scale: np.ndarray                    # [n] (prmtop SCREEN)
    solute_dielectric: float = 1.0
    solvent_dielectric: float = 78.5
    surface_area_energy: float = GB_SURFACE_AREA_ENERGY   # 0 switches the ACE surface term off

    def subset(self, index):
        """The same model over a selection (or repetition) of the atoms."""
        return ImplicitSolventData(self.model, np.asarray(self.radius, dtype=np.float64)[index].copy(), np.asarray(self.scale, dtype=np.float64)[index].copy(),
                                   self.solute_dielectric, self.solvent_dielectric, self.surface_area_energy)

    def to_desc(self):
        keep = {"radius": _f64(self.radius, (-1,)), "scale": _f64(self.scale, (-1,))}
        d = BluesImplicitSolventDesc()
        d.model = int(self.model)
        d.solute_dielectric = float(self.solute_dielectric); d.solvent_dielectric = float(self.solvent_dielectric)
        d.surface_area_energy = float(self.surface_area_energy)
        d.radius = keep["radius"].ctypes.data_as(_dp); d.scale = keep["scale"].ctypes.data_as(_dp)
        return d, keep


@dataclass
class SystemData:
    """Host-side description of the alchemical System (numpy, OpenMM units).

    Field meanings follow BluesSystemDesc in include/blues_engine.h.
    """
    box: np.ndarray                      # (3,) orthorhombic edge lengths, nm
    mass: np.ndarray
    charge: np.ndarray
    sigma: np.ndarray
    epsilon: np.ndarray
    exclusions: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int32))
    exception_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int32))
    exception_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    bond_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int32))
    bond_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 2)))
    angle_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.int32))
    angle_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 2)))
    torsion_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0, 4), np.int32))
    torsion_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    constraint_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int32))
    constraint_dist: np.ndarray = field(default_factory=lambda: np.zeros((0,)))
    alchemical_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0,), np.int32))
    restraint_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0,), np.int32))
    restraint_x0: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    restraint_k: float = 0.0
    nonbonded_method: int = NB_PME_DIRECT
    cutoff: float = 1.0
    ewald_alpha: float = 0.0
    softcore_alpha: float = 0.5
    annihilate_electrostatics: bool = True
    annihilate_sterics: bool = False
    remove_cm_motion: bool = False
    pme_grid: tuple = (0, 0, 0)          # NB_PME: mesh of the reciprocal sum
    pme_order: int = 5
    dispersion_correction: bool = True   # NB_PME: OpenMM's NonbondedForce default
    barostat: tuple = None               # (pressure [bar], temperature [K], frequency): MonteCarloBarostat of the MD leg (host-side, blues_amd/barostat.py)
    positions: np.ndarray = None         # (n,3) nm, optional initial coordinates
    residue_of_atom: np.ndarray = None   # optional bookkeeping for host-side selections
    names: list = None
    extras: dict = None                  # oracle-only test extras (custom forces of the ethylene known-answer system); refused by the engine, which takes them from the two typed fields below
    custom_pair_mode: int = PAIR_STANDARD  # NB_NOCUTOFF only; PAIR_ETHYLENE: q/r^2 + lambda-scaled 12-6 between alchemical and non-alchemical atoms
    centroid_bonds: tuple = ()           # NB_NOCUTOFF only; entries (idx1, w1, idx2, w2, k): E = 0.5 k |c1 - c2|^2, c = sum(w x) / sum(w)
    implicit_solvent: ImplicitSolventData = None   # NB_NOCUTOFF only; GB-OBC with the ACE surface term (blues_engine_create_gb)
    alchemical_pme_treatment: str = "direct-space"   # NB_PME: "direct-space" or "exact" (openmmtools' alchemical_pme_treatment; blues_engine_create_ext)
    cmap_maps: tuple = ()                # CMAPTorsionForce maps: (n, n) arrays, kJ/mol, E[i, j] at phi = 2 pi i / n, psi = 2 pi j / n (blues_engine_create_ext)
    cmap_torsions: np.ndarray = field(default_factory=lambda: np.zeros((0, 9), np.int32))   # (m, 9): map, a1..a4 (phi), b1..b4 (psi)
    # CHARMM terms of a chamber topology (blues_engine_create_ext).  Urey-Bradley: E = 0.5 k (r - r0)^2 between the 1-3 atoms of an
    # angle -- a force, not a bond: it joins no molecule, fragment or constraint.  Improper: E = k (psi - psi0)^2, psi the dihedral 1-2-3-4
    urey_bradley_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int32))
    urey_bradley_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 2)))   # (n, 2): r0 nm, k kJ/mol/nm^2
    improper_atoms: np.ndarray = field(default_factory=lambda: np.zeros((0, 4), np.int32))
    improper_params: np.ndarray = field(default_factory=lambda: np.zeros((0, 2)))       # (n, 2): psi0 rad, k kJ/mol/rad^2
    # createSystem's switchDistance, nm: the Lennard-Jones switching function of a periodic System between this distance and the cutoff
    # (BluesSystemExtV4).  0, or a value >= the cutoff: no switch; on a NoCutoff System it is stored and has no effect, like the box
    switch_distance: float = 0.0

    def __post_init__(self):
        alchemical_pme_treatment_code(self.alchemical_pme_treatment)

    @property
    def n_atoms(self):
        return int(len(self.mass))

    def check_alchemical_pme_treatment(self, integrator=None):
        """What blues_engine_create_ext refuses about the treatment (with `integrator`, an IntegratorData: about the pair), raised
        before a library is loaded (ValueError)."""
        if alchemical_pme_treatment_code(self.alchemical_pme_treatment) == 0:
            return
        if int(self.nonbonded_method) != NB_PME or not all(int(k) > 0 for k in tuple(self.pme_grid)):
            raise ValueError("alchemical_pme_treatment 'exact' needs nonbonded_method = PME with a mesh: without reciprocal space "
                             "(NoCutoff, direct-space-only PME) there is nothing for it to treat")
        if not self.annihilate_electrostatics:
            raise ValueError("alchemical_pme_treatment 'exact' needs annihilate_electrostatics = 1: the alchemical charges are scaled by "
                             "lambda_electrostatics as a whole (exact PME can only annihilate)")
        if integrator is not None and (integrator.measure_shadow_work or integrator.measure_heat):
            raise ValueError("alchemical_pme_treatment 'exact' together with measure_shadow_work / measure_heat is not supported: the energy "
                             "ledger's device-side energy sum does not know the exact treatment's partials")
        if integrator is not None and int(integrator.switching_mode) != 0:
            raise ValueError("alchemical_pme_treatment 'exact' with a switching_mode integrator is not supported: its force and energy "
                             "bookkeeping does not know the exact treatment's terms")

    def check_switch_distance(self):
        """What blues_engine_create_ext refuses about the switch distance, raised before a library is loaded (ValueError)."""
        d = float(self.switch_distance)
        if not np.isfinite(d) or d < 0.0:
            raise ValueError("switch_distance %r: the switch distance of the Lennard-Jones switching function must be finite and not negative "
                             "(0: no switch)" % (self.switch_distance,))

    @property
    def lj_switch_in_force(self):
        """The switch distance the pair kernels apply: switch_distance on a periodic System where 0 < switch_distance < cutoff, else 0."""
        d = float(self.switch_distance)
        return d if int(self.nonbonded_method) != NB_NOCUTOFF and 0.0 < d < float(self.cutoff) else 0.0

    @property
    def has_cmap(self):
        return len(tuple(self.cmap_maps or ())) > 0 or np.asarray(self.cmap_torsions).size > 0

    @property
    def has_charmm(self):
        return np.asarray(self.urey_bradley_atoms).size > 0 or np.asarray(self.improper_atoms).size > 0

    def ext_desc(self):
        """BluesSystemExt of this System -- BluesSystemExtV3 where it carries Urey-Bradley terms or impropers, BluesSystemExtV4 where a
        Lennard-Jones switch is in force (and only then: every other System passes the descriptor it always has) --, or None where
        blues_engine_create / blues_engine_create_gb say everything.  The numpy buffers of the maps and of the CHARMM terms stay alive
        with the descriptor (its _keep)."""
        code = alchemical_pme_treatment_code(self.alchemical_pme_treatment)
        self.check_switch_distance()
        switch = self.lj_switch_in_force
        if code == 0 and not self.has_cmap and not self.has_charmm and switch == 0.0:
            return None
        d = BluesSystemExtV4() if switch != 0.0 else (BluesSystemExtV3() if self.has_charmm else BluesSystemExt())
        d.struct_size = C.sizeof(d); d.alchemical_pme_treatment = code
        if switch != 0.0:
            d.lj_switch_distance = switch
        if self.has_cmap:
            maps = [_f64(m) for m in self.cmap_maps]
            tors = _i32(self.cmap_torsions, (-1, 9))
            keep = {"size": _i32([m.shape[0] for m in maps], (-1,)),
                    # E[i, j] is stored energy[i + n * j]: the transpose, row by row
                    "energy": _f64(np.concatenate([m.T.reshape(-1) for m in maps]) if maps else np.zeros(0), (-1,)),
                    "map": _i32(tors[:, 0], (-1,)), "atoms": _i32(tors[:, 1:], (-1,))}
            d.n_cmap_maps = len(maps); d.n_cmap_torsions = len(tors)
            d.cmap_size = keep["size"].ctypes.data_as(_ip); d.cmap_energy = keep["energy"].ctypes.data_as(_dp)
            d.cmap_torsion_map = keep["map"].ctypes.data_as(_ip); d.cmap_torsion_atoms = keep["atoms"].ctypes.data_as(_ip)
            d._keep = keep
        if self.has_charmm:
            keep = getattr(d, "_keep", {})
            keep.update({"ub_atoms": _i32(self.urey_bradley_atoms, (-1, 2)), "ub_params": _f64(self.urey_bradley_params, (-1, 2)),
                         "impr_atoms": _i32(self.improper_atoms, (-1, 4)), "impr_params": _f64(self.improper_params, (-1, 2))})
            d.n_urey_bradley = len(keep["ub_atoms"]); d.n_impropers = len(keep["impr_atoms"])
            d.urey_bradley_atoms = keep["ub_atoms"].ctypes.data_as(_ip); d.urey_bradley_params = keep["ub_params"].ctypes.data_as(_dp)
            d.improper_atoms = keep["impr_atoms"].ctypes.data_as(_ip); d.improper_params = keep["impr_params"].ctypes.data_as(_dp)
            d._keep = keep
        return d

    def check_charmm(self):
        """What blues_engine_create_ext refuses about the Urey-Bradley terms and the impropers, raised before a library is loaded
        (ValueError)."""
        for label, atoms, params, width in (("Urey-Bradley term", self.urey_bradley_atoms, self.urey_bradley_params, 2),
                                            ("improper", self.improper_atoms, self.improper_params, 4)):
            atoms, params = np.asarray(atoms), np.asarray(params, dtype=np.float64)
            if atoms.size == 0 and params.size == 0:
                continue
            if atoms.ndim != 2 or atoms.shape[1] != width or params.ndim != 2 or params.shape != (len(atoms), 2):
                raise ValueError("%ss: an (n, %d) array of atoms and an (n, 2) array of parameters; got shapes %s and %s" % (label, width, atoms.shape, params.shape))
            for t, (row, (x0, k)) in enumerate(zip(atoms, params)):
                if np.any(row < 0) or np.any(row >= self.n_atoms):
                    raise ValueError("%s %d: atom index out of range" % (label, t))
                if len(set(int(a) for a in row)) != width:
                    raise ValueError("%s %d: two equal atoms within one term" % (label, t))
                if not np.isfinite(k) or k < 0.0:
                    raise ValueError("%s %d: force constant %g is negative or not finite" % (label, t, k))
                if width == 2 and not (np.isfinite(x0) and x0 > 0.0):
                    raise ValueError("%s %d: r0 %g is not a positive length" % (label, t, x0))
                if width == 4 and not abs(x0) <= np.pi:
                    raise ValueError("%s %d: psi0 %g lies outside [-pi, pi]" % (label, t, x0))

    def check_cmap(self):
        """What blues_engine_create_ext refuses about the CMAP maps and torsions, raised before a library is loaded (ValueError)."""
        maps = tuple(self.cmap_maps or ())
        tors = np.asarray(self.cmap_torsions)
        if tors.size and (tors.ndim != 2 or tors.shape[1] != 9):
            raise ValueError("cmap_torsions: an (m, 9) array of map, a1..a4, b1..b4; got shape %s" % (tors.shape,))
        for k, m in enumerate(maps):
            m = np.asarray(m, dtype=np.float64)
            if m.ndim != 2 or m.shape[0] != m.shape[1] or not CMAP_MIN_SIZE <= m.shape[0] <= CMAP_MAX_SIZE:
                raise ValueError("CMAP map %d: size %s; a map is n x n with n from %d to %d" % (k, "x".join(str(q) for q in m.shape), CMAP_MIN_SIZE, CMAP_MAX_SIZE))
            if not np.all(np.isfinite(m)):
                raise ValueError("CMAP map %d: an energy is not finite" % k)
        for t, row in enumerate(tors.reshape(-1, 9)):
            if row[0] < 0 or row[0] >= len(maps):
                raise ValueError("CMAP torsion %d: map %d of %d" % (t, row[0], len(maps)))
            if np.any(row[1:] < 0) or np.any(row[1:] >= self.n_atoms):
                raise ValueError("CMAP torsion %d: atom index out of range" % t)
            for d in (row[1:5], row[5:9]):
                if len(set(int(a) for a in d)) != 4:
                    raise ValueError("CMAP torsion %d: two equal atoms within one dihedral" % t)

    def check_custom_forces(self):
        """What blues_engine_create refuses about the two custom forces, raised before a library is loaded (ValueError)."""
        mode, bonds, n = int(self.custom_pair_mode), tuple(self.centroid_bonds or ()), self.n_atoms
        if mode not in (PAIR_STANDARD, PAIR_ETHYLENE):
            raise ValueError("custom_pair_mode %d: the engine knows 0 (none) and 1 (the ethylene pair form)" % mode)
        if (mode or bonds) and int(self.nonbonded_method) != NB_NOCUTOFF:
            raise ValueError("custom forces (custom_pair_mode, centroid_bonds) need nonbonded_method = NoCutoff: they have no periodic form")
        if mode == PAIR_ETHYLENE and len(np.asarray(self.alchemical_atoms).reshape(-1)) == 0:
            raise ValueError("custom_pair_mode 1 acts between alchemical and non-alchemical atoms: the System has no alchemical atom")
        if len(bonds) > MAX_CENTROID_BONDS:
            raise ValueError("%d centroid bonds: at most %d" % (len(bonds), MAX_CENTROID_BONDS))
        for b, bond in enumerate(bonds):
            if len(bond) != 5:
                raise ValueError("centroid bond %d: an entry is (idx1, w1, idx2, w2, k)" % b)
            for idx, w in ((bond[0], bond[1]), (bond[2], bond[3])):
                idx, w = np.asarray(idx).reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1)
                if len(idx) != len(w):
                    raise ValueError("centroid bond %d: %d atoms but %d weights" % (b, len(idx), len(w)))
                if len(idx) == 0 or len(idx) > MAX_CENTROID_GROUP:
                    raise ValueError("centroid bond %d: a group of %d atoms (1 to %d)" % (b, len(idx), MAX_CENTROID_GROUP))
                if np.any(idx < 0) or np.any(idx >= n):
                    raise ValueError("centroid bond %d: atom index out of range" % b)
                if not np.all(np.isfinite(w)) or w.sum() == 0.0:
                    raise ValueError("centroid bond %d: the weights of a group sum to zero (or are not finite)" % b)

    def check_implicit_solvent(self, integrator=None):
        """What blues_engine_create_gb refuses about implicit solvent (with `integrator`, an IntegratorData: about the pair), raised
        before a library is loaded (ValueError)."""
        gb = self.implicit_solvent
        if gb is None or int(gb.model) == GB_NONE:
            return
        if integrator is not None and (integrator.measure_shadow_work or integrator.measure_heat):
            raise ValueError("implicit solvent together with measure_shadow_work / measure_heat is not supported: the energy ledger's "
                             "device-side energy sum does not know the GB partials")
        if int(gb.model) not in (GB_OBC1, GB_OBC2):
            raise ValueError("implicit solvent: model %d; the engine knows 1 (OBC1) and 2 (OBC2)" % int(gb.model))
        if int(self.nonbonded_method) != NB_NOCUTOFF:
            raise ValueError("implicit solvent needs nonbonded_method = NoCutoff: GB has no periodic or cutoff form here")
        if gb.radius is None or gb.scale is None:
            raise ValueError("implicit solvent without its radius / scale arrays")
        radius, scale = np.asarray(gb.radius, dtype=np.float64).reshape(-1), np.asarray(gb.scale, dtype=np.float64).reshape(-1)
        if len(radius) != self.n_atoms or len(scale) != self.n_atoms:
            raise ValueError("implicit solvent: %d radii and %d scale factors for %d atoms" % (len(radius), len(scale), self.n_atoms))
        if not (gb.solute_dielectric > 0.0 and gb.solvent_dielectric > 0.0):
            raise ValueError("implicit solvent: the dielectric constants must be positive (solute %g, solvent %g)" % (gb.solute_dielectric, gb.solvent_dielectric))
        if not gb.surface_area_energy >= 0.0:
            raise ValueError("implicit solvent: surface_area_energy %g is negative" % gb.surface_area_energy)
        bad = np.nonzero(~(radius > GB_RADIUS_OFFSET))[0]
        if len(bad):
            raise ValueError("implicit solvent: radius %g nm of atom %d is not above the 0.009 nm offset" % (radius[bad[0]], bad[0]))
        if not np.all(np.isfinite(scale)) or np.any(scale < 0.0):
            raise ValueError("implicit solvent: a scale factor is negative or not finite")
        if int(self.custom_pair_mode) != PAIR_STANDARD or tuple(self.centroid_bonds or ()):
            raise ValueError("implicit solvent together with the custom forces (custom_pair_mode, centroid bonds) is not supported")
        if not self.annihilate_electrostatics:
            raise ValueError("implicit solvent needs annihilate_electrostatics = 1: the GB charges of the alchemical atoms are scaled by lambda_electrostatics as a whole")

    def to_desc(self):
        """Returns (BluesSystemDesc, keepalive) -- keepalive owns the numpy buffers."""
        n = self.n_atoms
        keep = {}
        d = BluesSystemDesc()
        d.n_atoms = n
        box = np.asarray(self.box, dtype=np.float64).reshape(-1)
        if box.size == 3:
            box9 = np.zeros(9); box9[0], box9[4], box9[8] = box
        else:
            box9 = box
        for i in range(9):
            d.box[i] = float(box9[i])

        def put_f(name, arr, shape=None):
            a = _f64(arr, shape); keep[name] = a
            setattr(d, name, a.ctypes.data_as(_dp))
            return a

        def put_i(name, arr, shape=None):
            a = _i32(arr, shape); keep[name] = a
            setattr(d, name, a.ctypes.data_as(_ip))
            return a

        put_f("mass", self.mass, (n,)); put_f("charge", self.charge, (n,))
        put_f("sigma", self.sigma, (n,)); put_f("epsilon", self.epsilon, (n,))
        d.n_exclusions = len(put_i("exclusions", self.exclusions, (-1, 2)))
        d.n_exceptions = len(put_i("exception_atoms", self.exception_atoms, (-1, 2)))
        put_f("exception_params", self.exception_params, (-1, 3))
        d.n_bonds = len(put_i("bond_atoms", self.bond_atoms, (-1, 2))); put_f("bond_params", self.bond_params, (-1, 2))
        d.n_angles = len(put_i("angle_atoms", self.angle_atoms, (-1, 3))); put_f("angle_params", self.angle_params, (-1, 2))
        d.n_torsions = len(put_i("torsion_atoms", self.torsion_atoms, (-1, 4))); put_f("torsion_params", self.torsion_params, (-1, 3))
        d.n_constraints = len(put_i("constraint_atoms", self.constraint_atoms, (-1, 2))); put_f("constraint_dist", self.constraint_dist, (-1,))
        d.n_alchemical = len(put_i("alchemical_atoms", self.alchemical_atoms, (-1,)))
        d.n_restraints = len(put_i("restraint_atoms", self.restraint_atoms, (-1,))); put_f("restraint_x0", self.restraint_x0, (-1, 3))
        d.restraint_k = float(self.restraint_k)
        d.nonbonded_method = int(self.nonbonded_method)
        d.cutoff = float(self.cutoff); d.ewald_alpha = float(self.ewald_alpha); d.softcore_alpha = float(self.softcore_alpha)
        d.annihilate_electrostatics = int(bool(self.annihilate_electrostatics))
        d.annihilate_sterics = int(bool(self.annihilate_sterics))
        d.remove_cm_motion = int(bool(self.remove_cm_motion))
        for k in range(3):
            d.pme_grid[k] = int(self.pme_grid[k])
        d.pme_order = int(self.pme_order); d.dispersion_correction = int(bool(self.dispersion_correction))
        # the custom forces (ABI 7): groups flattened, bond b = groups 2b and 2b + 1
        d.custom_pair_mode = int(self.custom_pair_mode)
        bonds = tuple(self.centroid_bonds or ())
        start, atoms, weights = [0], [], []
        for bond in bonds:
            for idx, w in ((bond[0], bond[1]), (bond[2], bond[3])):
                atoms.extend(int(i) for i in np.asarray(idx).reshape(-1)); weights.extend(float(x) for x in np.asarray(w, dtype=np.float64).reshape(-1))
                start.append(len(atoms))
        d.n_centroid_bonds = len(bonds)
        put_i("centroid_group_start", start, (-1,)); put_i("centroid_atoms", atoms, (-1,))
        put_f("centroid_weights", weights, (-1,)); put_f("centroid_k", [bond[4] for bond in bonds], (-1,))
        return d, keep


@dataclass
class IntegratorData:
    """Numeric form of AlchemicalExternalLangevinIntegrator's constructor arguments."""
    timestep: float                      # ps
    temperature: float                   # K
    nsteps_neq: int
    lambda_sterics: np.ndarray           # [n_lambda_steps+1]
    lambda_electrostatics: np.ndarray
    splitting: str = "H V R O R V H"
    collision_rate: float = 1.0
    nprop: int = 1
    prop_lambda_min: float = 0.2
    prop_lambda_max: float = 0.8
    constraint_tolerance: float = 1e-8
    seed: int = 0
    replica: int = 0
    precision: int = 0                   # 0 mixed, 1 double
    switching_mode: int = 0              # SWITCH_NONE / SWITCH_VV / SWITCH_GHMC (reference blues/switching.py)
    steps_per_propagation: int = 1
    measure_shadow_work: int = 0         # SWITCH_NONE only: book the shadow work of the R and V substeps on the device
    measure_heat: int = 0                # SWITCH_NONE only: book the heat of the O substeps

    @property
    def n_lambda_steps(self):
        if self.switching_mode:
            return int(self.nsteps_neq)
        return int(self.nsteps_neq) * self.splitting.count("H")

    def to_desc(self):
        if self.switching_mode and (self.measure_shadow_work or self.measure_heat):
            raise ValueError("measure_shadow_work / measure_heat belong to the Langevin switch: a switching_mode integrator keeps its own shadow work")
        keep = {}
        d = BluesIntegratorDesc()
        d.timestep = float(self.timestep); d.temperature = float(self.temperature)
        d.collision_rate = float(self.collision_rate)
        d.nsteps_neq = int(self.nsteps_neq); d.nprop = int(self.nprop)
        d.prop_lambda_min = float(self.prop_lambda_min); d.prop_lambda_max = float(self.prop_lambda_max)
        keep["splitting"] = self.splitting.encode()
        d.splitting = keep["splitting"]
        nl = self.n_lambda_steps
        d.n_lambda_steps = nl
        ls = _f64(self.lambda_sterics, (-1,)); le = _f64(self.lambda_electrostatics, (-1,))
        if len(ls) != nl + 1 or len(le) != nl + 1:
            raise ValueError("lambda tables must have n_lambda_steps+1 = %d entries" % (nl + 1))
        keep["ls"], keep["le"] = ls, le
        d.lambda_sterics = ls.ctypes.data_as(_dp); d.lambda_electrostatics = le.ctypes.data_as(_dp)
        d.constraint_tolerance = float(self.constraint_tolerance)
        d.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF; d.replica = int(self.replica); d.precision = int(self.precision)
        d.switching_mode = int(self.switching_mode); d.steps_per_propagation = int(self.steps_per_propagation)
        d.measure_shadow_work = int(bool(self.measure_shadow_work)); d.measure_heat = int(bool(self.measure_heat))
        return d, keep


def declare_engine_prototypes(lib):
    """Attach argtypes/restype for every symbol include/blues_engine.h declares."""
    H = C.c_void_p
    protos = {
        "blues_engine_create": ([C.POINTER(BluesSystemDesc), C.POINTER(BluesIntegratorDesc), C.c_int, C.POINTER(H)], C.c_int),
        "blues_engine_create_gb": ([C.POINTER(BluesSystemDesc), C.POINTER(BluesIntegratorDesc), C.POINTER(BluesImplicitSolventDesc), C.c_int, C.POINTER(H)], C.c_int),
        "blues_engine_create_ext": ([C.POINTER(BluesSystemDesc), C.POINTER(BluesIntegratorDesc), C.POINTER(BluesImplicitSolventDesc), C.c_void_p, C.c_int, C.POINTER(H)], C.c_int),   # (ext: BluesSystemExt, BluesSystemExtV3 or BluesSystemExtV4, told apart by struct_size)
        "blues_engine_destroy": ([H], C.c_int),
        "blues_last_error": ([H], C.c_char_p),
        "blues_abi_version": ([], C.c_int),
        "blues_tuning_default": ([C.POINTER(BluesTuning)], None),
        "blues_set_tuning": ([C.POINTER(BluesTuning)], C.c_int),
        "blues_get_tuning": ([C.POINTER(BluesTuning)], C.c_int),
        "blues_set_positions": ([H, _dp, C.c_int32], C.c_int),
        "blues_set_velocities": ([H, _dp, C.c_int32], C.c_int),
        "blues_set_box": ([H, _dp], C.c_int),
        "blues_get_positions": ([H, _dp, C.c_int32], C.c_int),
        "blues_get_velocities": ([H, _dp, C.c_int32], C.c_int),
        "blues_get_forces": ([H, _dp, C.c_int32], C.c_int),
        "blues_get_box": ([H, _dp], C.c_int),
        "blues_set_velocities_to_temperature": ([H, C.c_double, C.c_uint64], C.c_int),
        "blues_get_energy": ([H, _dp, _dp], C.c_int),
        "blues_get_energy_at": ([H, C.c_double, C.c_double, _dp], C.c_int),
        "blues_get_energy_terms": ([H, _dp], C.c_int),
        "blues_mesh_energy": ([H, C.c_int32, _dp], C.c_int),
        "blues_step": ([H, C.c_int32], C.c_int),
        "blues_run_switch": ([H, C.c_int32, _dp], C.c_int),
        "blues_get_global": ([H, C.c_char_p, _dp], C.c_int),
        "blues_set_global": ([H, C.c_char_p, C.c_double], C.c_int),
        "blues_reset": ([H], C.c_int),
        "blues_get_stats": ([H, C.POINTER(C.c_int64)], C.c_int),
        "blues_get_exact_pme_path": ([H, C.POINTER(C.c_int64)], C.c_int),
        "blues_get_pme_path": ([H, C.POINTER(C.c_int64)], C.c_int),
        "blues_get_lj_switch": ([H, _dp], C.c_int),
        "blues_get_alchemical_layout": ([H, C.POINTER(C.c_int64)], C.c_int),
        "blues_get_cmap_angles": ([H, _dp], C.c_int),
        "blues_time_nonbonded": ([H, C.c_int32, _dp], C.c_int),
        "blues_time_list_build": ([H, C.c_int32, _dp], C.c_int),
        "blues_audit_lists": ([H, C.POINTER(C.c_int64)], C.c_int),
        "blues_snapshot_capture": ([H, C.c_int32, C.POINTER(H)], C.c_int),
        "blues_snapshot_release": ([H], C.c_int),
        "blues_snapshot_read": ([H, C.c_int32, _dp, C.c_int32], C.c_int),
        "blues_set_positions_from_snapshot": ([H, H], C.c_int),
        "blues_set_velocities_from_snapshot": ([H, H], C.c_int),
        "blues_snapshot_read_atoms": ([H, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _dp], C.c_int),
        "blues_set_positions_from_snapshot_edited": ([H, H, C.POINTER(C.c_int32), C.c_int32, _dp], C.c_int),
        "blues_batch_create": ([C.POINTER(H), C.c_int32, C.POINTER(H)], C.c_int),
        "blues_batch_destroy": ([H], C.c_int),
        "blues_batch_last_error": ([H], C.c_char_p),
        "blues_batch_size": ([H], C.c_int),
        "blues_batch_step": ([H, C.c_int32, _dp, C.POINTER(C.c_int32)], C.c_int),
        "blues_batch_set_active": ([H, C.POINTER(C.c_int32)], C.c_int),
        "blues_batch_prefetch_energies": ([H, C.c_int32], C.c_int),
        "blues_batch_snapshot_capture": ([H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(H)], C.c_int),
        "blues_batch_restore": ([H, C.POINTER(H), C.c_int32], C.c_int),
        "blues_batch_restore_edited": ([H, C.POINTER(H), C.POINTER(C.c_int32), C.c_int32, _dp], C.c_int),
        "blues_batch_read_atoms": ([H, C.POINTER(H), C.c_int32, C.POINTER(C.c_int32), C.c_int32, _dp], C.c_int),
        "blues_batch_reset": ([H, C.POINTER(C.c_int32)], C.c_int),
        "blues_batch_set_velocities_to_temperature": ([H, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)], C.c_int),
        "blues_batch_mesh_energy": ([H, C.c_int32, C.POINTER(C.c_int32), _dp], C.c_int),
        "blues_batch_get_stats": ([H, C.POINTER(C.c_int64)], C.c_int),
        "blues_batch_get_counters": ([H, _dp], C.c_int),
        "blues_batch_time_nonbonded": ([H, C.c_int32, _dp], C.c_int),
        "blues_batch_time_nonbonded_modes": ([H, C.c_int32, _dp, _dp], C.c_int),
        "blues_debug_setup_seconds": ([_dp], C.c_int),
        "blues_debug_check_guards": ([C.POINTER(C.c_int64)], C.c_int),
        "blues_batch_kernel_timing": ([H, C.c_int32], C.c_int),
        "blues_batch_get_kernel_timing": ([H, _dp], C.c_int),
        "blues_minimize_default": ([C.POINTER(BluesMinimizeDesc)], None),
        "blues_minimize": ([H, C.c_double, C.c_int32, C.POINTER(BluesMinimizeDesc), C.POINTER(BluesMinimizeResult)], C.c_int),
        "blues_batch_minimize": ([H, C.c_double, C.c_int32, C.POINTER(BluesMinimizeDesc), C.POINTER(C.c_int32), C.POINTER(BluesMinimizeResult), C.POINTER(C.c_int32)], C.c_int),
    }
    for name, (args, res) in protos.items():
        if name in OPTIONAL_SYMBOLS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.argtypes = args
        fn.restype = res
    return sorted(protos)


ENGINE_SYMBOLS = (
    "blues_engine_create", "blues_engine_create_gb", "blues_engine_create_ext", "blues_engine_destroy", "blues_last_error", "blues_abi_version",
    "blues_tuning_default", "blues_set_tuning", "blues_get_tuning",
    "blues_set_positions", "blues_set_velocities", "blues_set_box", "blues_get_positions",
    "blues_get_velocities", "blues_get_forces", "blues_get_box", "blues_set_velocities_to_temperature",
    "blues_get_energy", "blues_get_energy_at", "blues_get_energy_terms", "blues_mesh_energy", "blues_step", "blues_run_switch", "blues_get_global",
    "blues_set_global", "blues_reset", "blues_get_stats", "blues_get_exact_pme_path", "blues_get_pme_path", "blues_get_lj_switch", "blues_get_alchemical_layout", "blues_get_cmap_angles", "blues_time_nonbonded", "blues_time_list_build", "blues_audit_lists",
    "blues_snapshot_capture", "blues_snapshot_release", "blues_snapshot_read", "blues_set_positions_from_snapshot",
    "blues_set_velocities_from_snapshot", "blues_snapshot_read_atoms", "blues_set_positions_from_snapshot_edited",
    "blues_batch_create", "blues_batch_destroy", "blues_batch_last_error", "blues_batch_size", "blues_batch_step", "blues_batch_set_active", "blues_batch_prefetch_energies",
    "blues_batch_snapshot_capture", "blues_batch_restore", "blues_batch_restore_edited", "blues_batch_read_atoms", "blues_batch_reset",
    "blues_batch_set_velocities_to_temperature", "blues_batch_mesh_energy",
    "blues_batch_get_stats", "blues_batch_get_counters", "blues_batch_time_nonbonded", "blues_batch_time_nonbonded_modes",
    "blues_batch_kernel_timing", "blues_batch_get_kernel_timing", "blues_debug_setup_seconds", "blues_debug_check_guards",
    "blues_minimize_default", "blues_minimize", "blues_batch_minimize",
)
