"""CPU suite of the chamber reader and of CHARMM's Urey-Bradley terms and impropers: the prmtop formats, the written chamber file
(tests/charmm_cases.py) through amber.system_from_amber, the refusals, the helpers that carry the four fields, the descriptor, and
the numpy reference tests/charmm_reference.py pinned by itself."""
import ctypes
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import charmm_cases as cc
import charmm_reference as ref
from blues_amd import _abi, amber, systems

ROOT = cc.ROOT
KCAL = 4.184
_ARRAYS = ("mass", "charge", "sigma", "epsilon", "exclusions", "exception_atoms", "exception_params", "bond_atoms", "bond_params", "angle_atoms",
           "angle_params", "torsion_atoms", "torsion_params", "constraint_atoms", "constraint_dist", "alchemical_atoms")


# ---- 0. the reference, by itself
def _fd(fun, x, h):
    g = np.zeros_like(x)
    for a in range(len(x)):
        for k in range(3):
            xp, xm = x.copy(), x.copy(); xp[a, k] += h; xm[a, k] -= h
            g[a, k] = -(fun(xp) - fun(xm)) / (2.0 * h)
    return g


@pytest.mark.parametrize("box", [None, (0.9, 1.0, 1.1)])
def test_reference_forces_are_the_gradient_to_second_order(box):
    """forces = -central difference, and the error falls about fourfold when h is halved (a second-order check, not a number)"""
    rng = np.random.default_rng(4)
    x = ref.four_atoms(0.4) + rng.normal(size=(4, 3)) * 0.01
    if box is not None:     # every atom wrapped into the box by itself, the second one moved across a face
        x[1] += np.array(box) * np.array([1.0, 0.0, -1.0])
    terms = {
        "improper": lambda y: ref.impropers([[0, 1, 2, 3]], [[0.1, 50.0]], y, box),
        "Urey-Bradley": lambda y: ref.urey_bradley([[0, 2], [1, 3]], [[0.2, 3.0e4], [0.26, 1.0e4]], y, box),
        "1-4": lambda y: ref.exceptions([[0, 3], [1, 2]], [[0.02, 0.25, 0.4], [-0.03, 0.2, 0.0]], y, box),
    }
    for name, fun in terms.items():
        f = fun(x)[1]
        err = [np.abs(_fd(lambda y: fun(y)[0], x, h) - f).max() for h in (2e-3, 1e-3, 5e-4)]
        assert np.abs(f).max() > 1.0, name
        assert 3.0 < err[0] / err[1] < 5.0 and 3.0 < err[1] / err[2] < 5.0, (name, err)


def test_reference_angles_and_wrap():
    for psi in (0.0, 1e-7, -1e-7, 0.3, -0.3, np.pi - 1e-7, -3.0):
        assert abs(ref.dihedral(ref.four_atoms(psi))[0] - psi) <= 1e-12
    assert ref.wrap(-6.0) == pytest.approx(2.0 * np.pi - 6.0, abs=1e-15) and ref.wrap(np.pi) == np.pi and ref.wrap(-np.pi) == np.pi
    e, _ = ref.impropers([[0, 1, 2, 3]], [[3.0, 10.0]], ref.four_atoms(-3.0))
    assert e == pytest.approx(10.0 * (2.0 * np.pi - 6.0) ** 2, rel=1e-12)
    # the fixture's own angles (planar centres near 0, tetrahedral ones near -0.6)
    a = ref.improper_angles(cc.IMPROPERS, cc.positions()[0])
    assert np.allclose(a, [0.0084, 0.154, 0.055, -0.61, -0.54], atol=6e-3), a


# ---- 1. formats
def test_formats():
    today = {"(20a4)": (20, "a", 4), "(10I8)": (10, "i", 8), "(5E16.8)": (5, "e", 16), "(1a80)": (1, "a", 80), "(3I8)": (3, "i", 8), "(1I8)": (1, "i", 8),
             "(20I4)": (20, "i", 4), "(8F9.5)": (8, "f", 9), "(2I8)": (2, "i", 8), "(6I8)": (6, "i", 8), " (10i8) ": (10, "i", 8), "(1a4,1x)": (1, "a", 4)}
    for fmt, want in today.items():
        assert amber._parse_format(fmt) == want, fmt
    assert amber._parse_format("(a80)") == (1, "a", 80)
    assert amber._parse_format("(i2,a78)")[1] == "line"
    for bad in ("(x)", "", "(80)", "(i2;a78)"):
        with pytest.raises(ValueError, match="unsupported prmtop format"):
            amber._parse_format(bad)


def test_written_file_round_trips(tmp_path):
    path, exp = cc.write_chamber(tmp_path)
    prm, plain = amber.read_prmtop(path), amber.read_prmtop(cc.plain_prmtop())
    assert prm["CTITLE"] == ["chamber-style topology of the valine dipeptide, written for the tests"]
    assert len(prm["FORCE_FIELD_TYPE"]) == 1 and prm["FORCE_FIELD_TYPE"][0].startswith(" 1 CHARMM  36") and "TITLE" not in prm
    assert amber.is_chamber(prm) and not amber.is_chamber(plain)
    for k, v in plain.items():
        if k in ("TITLE", "SCEE_SCALE_FACTOR", "SCNB_SCALE_FACTOR"):
            continue
        assert np.array_equal(np.asarray(prm[k]), np.asarray(v)), k
    assert np.all(prm["SCEE_SCALE_FACTOR"] == 1.0) and np.all(prm["SCNB_SCALE_FACTOR"] == 1.0) and len(prm["SCEE_SCALE_FACTOR"]) == len(plain["SCEE_SCALE_FACTOR"])
    assert prm["CHARMM_UREY_BRADLEY_COUNT"].tolist() == [len(exp["ub_atoms"]), len(cc.UB_K)]
    assert np.array_equal(prm["CHARMM_UREY_BRADLEY"].reshape(-1, 3)[:, :2] - 1, exp["ub_atoms"])
    assert np.array_equal(prm["CHARMM_IMPROPERS"].reshape(-1, 5)[:, :4] - 1, exp["improper_atoms"])
    assert np.array_equal(prm["LENNARD_JONES_14_ACOEF"], exp["a14"]) and np.array_equal(prm["LENNARD_JONES_14_BCOEF"], exp["b14"])
    assert "%COMMENT" in open(path).read()


# ---- 2. system_from_amber
def test_chamber_file_becomes_the_fields(tmp_path):
    path, exp = cc.write_chamber(tmp_path)
    prm = amber.read_prmtop(path)
    pos, box = cc.positions()
    s = amber.system_from_amber(prm, pos, box, nonbonded_method="NoCutoff")
    p = amber.system_from_amber(amber.read_prmtop(cc.plain_prmtop()), pos, box, nonbonded_method="NoCutoff")
    assert len(exp["ub_atoms"]) > 30 and s.has_charmm and s.ext_desc() is not None
    assert np.array_equal(s.urey_bradley_atoms, exp["ub_atoms"]) and s.urey_bradley_atoms.dtype == np.int32
    assert np.array_equal(s.improper_atoms, exp["improper_atoms"])
    np.testing.assert_allclose(s.urey_bradley_params[:, 0], 0.1 * exp["ub_s0"], rtol=1e-15, atol=0.0)
    np.testing.assert_allclose(s.urey_bradley_params[:, 1], 2.0 * exp["ub_k"] * KCAL * 100.0, rtol=1e-15, atol=0.0)
    np.testing.assert_allclose(s.improper_params[:, 0], exp["improper_phase"] * np.pi / 180.0, rtol=1e-15, atol=0.0)
    np.testing.assert_allclose(s.improper_params[:, 1], KCAL * exp["improper_k"], rtol=1e-15, atol=0.0)
    assert np.count_nonzero(s.improper_params[:, 0]) == 2
    # exceptions from the 1-4 table (SCEE = SCNB = 1), pair for pair
    ntypes, tidx, nbidx = int(prm["POINTERS"][1]), prm["ATOM_TYPE_INDEX"], prm["NONBONDED_PARM_INDEX"]
    assert np.array_equal(s.exception_atoms, p.exception_atoms)
    want = np.zeros((len(s.exception_atoms), 3))
    for r, (i, l) in enumerate(s.exception_atoms):
        k = int(nbidx[ntypes * (int(tidx[i]) - 1) + int(tidx[l]) - 1]) - 1
        a, b = exp["a14"][k], exp["b14"][k]
        want[r] = (s.charge[i] * s.charge[l], 0.1 * (a / b) ** (1.0 / 6.0), KCAL * b * b / (4.0 * a)) if a != 0.0 and b != 0.0 else (s.charge[i] * s.charge[l], 0.1, 0.0)
    np.testing.assert_allclose(s.exception_params, want, rtol=1e-15, atol=0.0)
    assert np.count_nonzero(want[:, 2]) > 10 and not np.allclose(s.exception_params[:, 1:], p.exception_params[:, 1:], rtol=1e-3)   # (a reader that ignores the table gives the right-hand side)
    # everything else is the Amber file's
    for name in _ARRAYS:
        if name != "exception_params":
            assert np.array_equal(np.asarray(getattr(s, name)), np.asarray(getattr(p, name))), name
    assert not p.has_charmm and p.ext_desc() is None
    for k, v in cc.EMPTY.items():
        assert np.asarray(getattr(p, k)).shape == v.shape


def _parent_exceptions(prm, s):
    """exception_params as system_from_amber made them before the 1-4 table existed: the per-atom diagonal sigma / epsilon, the file's
    SCEE / SCNB, first dihedral that names the pair"""
    dihs = np.vstack([np.asarray(prm[n]).reshape(-1, 5) for n in ("DIHEDRALS_INC_HYDROGEN", "DIHEDRALS_WITHOUT_HYDROGEN")])
    exc = {}
    for d in dihs:
        i, l, t = int(d[0]) // 3, abs(int(d[3])) // 3, int(d[4]) - 1
        if int(d[2]) >= 0 and int(d[3]) >= 0 and (min(i, l), max(i, l)) not in exc:
            exc[(min(i, l), max(i, l))] = (s.charge[i] * s.charge[l] / prm["SCEE_SCALE_FACTOR"][t], 0.5 * (s.sigma[i] + s.sigma[l]),
                                           np.sqrt(s.epsilon[i] * s.epsilon[l]) / prm["SCNB_SCALE_FACTOR"][t])
    return np.array([exc[k] for k in sorted(exc)])


def _golden_maker():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_amber_arrays", os.path.join(cc.GOLDEN, "make_amber_arrays.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", ["vacDivaline", "vacDivaline_free", "TOL-parm"])
def test_amber_files_give_the_recorded_arrays(case):
    """Every array that system_from_amber makes of a non-chamber prmtop is bitwise what the commit before the chamber reader made of
    it (tests/golden/amber_arrays.npz, written by that commit's reader through tests/golden/make_amber_arrays.py): NoCutoff with and
    without constraints, and the periodic fixture with repartitioned hydrogens."""
    maker = _golden_maker()
    z = np.load(os.path.join(cc.GOLDEN, "amber_arrays.npz"))
    now = maker.arrays(case)
    assert sorted(now) == sorted(maker.FIELDS) and all("%s/%s" % (case, f) in z.files for f in maker.FIELDS)
    for f, a in now.items():
        want = z["%s/%s" % (case, f)]
        assert a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes(), (case, f)
    assert len(now["exception_params"]) > 10 and len(now["torsion_params"]) > 10


def test_plain_amber_file_is_untouched():
    prm = amber.read_prmtop(cc.plain_prmtop())
    pos, box = cc.positions()
    s = amber.system_from_amber(prm, pos, box, nonbonded_method="NoCutoff")
    assert np.array_equal(s.exception_params, _parent_exceptions(prm, s))          # bit for bit
    z = np.load(os.path.join(ROOT, "blues_amd", "data", "tol_box.npz"))          # (a System the parent wrote loads with the new fields empty)
    t, _ = systems.load_system(os.path.join(ROOT, "blues_amd", "data", "tol_box.npz"))
    assert not t.has_charmm and "urey_bradley_atoms" not in z.files
    for k, v in cc.EMPTY.items():
        assert np.asarray(getattr(s, k)).shape == v.shape and np.asarray(getattr(t, k)).shape == v.shape


# ---- 3. what the reader refuses
def _ints(values, per_line=10):
    values = list(values)
    return ["".join("%8d" % v for v in values[k:k + per_line]) for k in range(0, len(values), per_line)]


def _edit_numbers(name, fun):
    """an edit for cc.write_chamber: the integers of section `name` through fun(list) -> list"""
    def edit(new):
        at = next(k for k, line in enumerate(new[name]) if line.startswith("%FORMAT"))
        vals = [int(v) for line in new[name][at + 1:] for v in line.split()]
        new[name] = new[name][:at + 1] + _ints(fun(vals))
    return edit


def _set(pos, value):
    def fun(vals):
        vals = list(vals); vals[pos] = value
        return vals
    return fun


@pytest.mark.parametrize("name, fun, why", [
    ("CHARMM_UREY_BRADLEY_COUNT", _set(0, 7), "Urey-Bradley term: 7 terms are announced but CHARMM_UREY_BRADLEY holds"),
    ("CHARMM_UREY_BRADLEY_COUNT", _set(1, 5), "5 types are announced but CHARMM_UREY_BRADLEY_FORCE_CONSTANT holds 4"),
    ("CHARMM_NUM_IMPROPERS", _set(0, 4), "improper: 4 terms are announced but CHARMM_IMPROPERS holds 25 integers"),
    ("CHARMM_NUM_IMPR_TYPES", _set(0, 2), "2 types are announced but CHARMM_IMPROPER_FORCE_CONSTANT holds 3"),
    ("CHARMM_UREY_BRADLEY", _set(2, 5), "Urey-Bradley term 1: type 5 of 4"),
    ("CHARMM_UREY_BRADLEY", _set(5, 0), "Urey-Bradley term 2: type 0 of 4"),
    ("CHARMM_UREY_BRADLEY", _set(0, 36), "Urey-Bradley term 1: atom out of range"),
    ("CHARMM_IMPROPERS", _set(9, 4), "improper 2: type 4 of 3"),
    ("CHARMM_IMPROPERS", _set(3, 0), "improper 1: atom out of range"),
    ("CHARMM_IMPROPERS", _set(1, 17), "improper 1: two equal atoms within one term"),
])
def test_reader_refusals(tmp_path, name, fun, why):
    path, _ = cc.write_chamber(tmp_path, edit=_edit_numbers(name, fun))
    pos, box = cc.positions()
    with pytest.raises(ValueError, match=why):
        amber.system_from_amber(amber.read_prmtop(path), pos, box, nonbonded_method="NoCutoff")


def test_equal_atoms_in_a_urey_bradley_term(tmp_path):
    def fun(vals):
        vals = list(vals); vals[1] = vals[0]
        return vals
    path, _ = cc.write_chamber(tmp_path, edit=_edit_numbers("CHARMM_UREY_BRADLEY", fun))
    with pytest.raises(ValueError, match="Urey-Bradley term 1: two equal atoms within one term"):
        amber.charmm_from_prmtop(amber.read_prmtop(path), 35)


def _scaled_off_diagonal(text):
    """the text with one off-diagonal entry of LENNARD_JONES_ACOEF (a pair of types that atoms use) scaled by 1.01; returns (text, pair)"""
    prm = amber.read_prmtop(cc.plain_prmtop())
    nt = int(prm["POINTERS"][1])
    a, b = 0, 1
    k = int(prm["NONBONDED_PARM_INDEX"][nt * a + b]) - 1
    assert k >= 0 and prm["LENNARD_JONES_ACOEF"][k] != 0.0
    lines = text.split("\n")
    at = next(n for n, line in enumerate(lines) if line.split()[:2] == ["%FLAG", "LENNARD_JONES_ACOEF"])
    while not lines[at].startswith("%FORMAT"):
        at += 1
    row, col = at + 1 + k // 5, 16 * (k % 5)
    old = lines[row][col:col + 16]
    assert float(old) == prm["LENNARD_JONES_ACOEF"][k]
    lines[row] = lines[row][:col] + "%16.8E" % (1.01 * float(old)) + lines[row][col + 16:]
    return "\n".join(lines), (a + 1, b + 1)


def test_nbfix_is_refused_for_chamber_only(tmp_path):
    pos, box = cc.positions()
    path, _ = cc.write_chamber(tmp_path)
    text, pair = _scaled_off_diagonal(open(path).read())
    bad = tmp_path / "nbfix.prmtop"; bad.write_text(text)
    with pytest.raises(ValueError, match=r"NBFIX: LENNARD_JONES_ACOEF of the type pair \(%d, %d\)" % pair):
        amber.system_from_amber(amber.read_prmtop(str(bad)), pos, box, nonbonded_method="NoCutoff")
    text, _ = _scaled_off_diagonal(open(cc.plain_prmtop()).read())
    same = tmp_path / "amber.prmtop"; same.write_text(text)
    s = amber.system_from_amber(amber.read_prmtop(str(same)), pos, box, nonbonded_method="NoCutoff")           # today's behaviour: not looked at
    p = amber.system_from_amber(amber.read_prmtop(cc.plain_prmtop()), pos, box, nonbonded_method="NoCutoff")
    assert np.array_equal(s.sigma, p.sigma) and np.array_equal(s.exception_params, p.exception_params)


# ---- 4. check_charmm and the helpers that carry the fields
@pytest.mark.parametrize("case", sorted(cc.bad_systems()))
def test_check_charmm_refusals(case):
    why, s = cc.bad_systems()[case]
    with pytest.raises(ValueError, match=why):
        s.check_charmm()
    from blues_amd import engine
    data = _abi.IntegratorData(timestep=0.002, temperature=300.0, nsteps_neq=2, lambda_sterics=np.ones(5), lambda_electrostatics=np.ones(5))
    with pytest.raises(engine.EngineError, match=why):          # the wrapper, before any library is loaded
        engine.NativeEngine(s, data)


def test_check_charmm_shapes():
    s = cc.chamber_divaline()
    s.check_charmm()
    with pytest.raises(ValueError, match="an \\(n, 4\\) array of atoms and an \\(n, 2\\) array of parameters"):
        dataclasses.replace(s, improper_params=s.improper_params[:3]).check_charmm()
    cc.without(s).check_charmm()


def test_save_load_tile_and_plan_carry_the_fields(tmp_path):
    s = cc.chamber_divaline()
    systems.save_system(str(tmp_path / "s.npz"), s)
    back, extra = systems.load_system(str(tmp_path / "s.npz"))
    assert extra == {} and back.has_charmm
    for k in cc.EMPTY:
        assert np.array_equal(getattr(back, k), getattr(s, k)), k
    systems.save_system(str(tmp_path / "p.npz"), cc.without(s))
    assert not any(k.startswith(("urey", "improper")) for k in np.load(str(tmp_path / "p.npz")).files)
    s.box = np.array([3.0, 3.0, 3.0])
    t = systems.tile_system(s, (2, 1, 1))
    n, m = len(s.urey_bradley_atoms), len(s.improper_atoms)
    assert np.array_equal(t.urey_bradley_atoms[:n], s.urey_bradley_atoms) and np.array_equal(t.urey_bradley_atoms[n:], s.urey_bradley_atoms + 35)
    assert np.array_equal(t.improper_atoms[:m], s.improper_atoms) and np.array_equal(t.improper_atoms[m:], s.improper_atoms + 35)
    assert np.array_equal(t.urey_bradley_params, np.concatenate([s.urey_bradley_params] * 2)) and np.array_equal(t.improper_params, np.concatenate([s.improper_params] * 2))
    t.check_charmm()
    e0 = ref.energy_forces(s, s.positions)
    e1 = ref.energy_forces(t, t.positions)
    assert e1[0] == pytest.approx(2.0 * e0[0], rel=1e-13) and e1[1] == pytest.approx(2.0 * e0[1], rel=1e-13)
    f = systems.freeze_atoms(s, [16, 18])
    assert np.array_equal(f.improper_atoms, s.improper_atoms) and np.array_equal(f.urey_bradley_params, s.urey_bradley_params)
    # an alchemical / plain pair that differs only in an improper constant has no differential plan
    plain = dataclasses.replace(s, alchemical_atoms=np.zeros(0, np.int32))
    assert systems.alchemical_difference_plan(s, plain) == {"kind": "zero"}
    q = s.improper_params.copy(); q[0, 1] *= 1.5
    other = dataclasses.replace(plain, improper_params=q)
    assert systems.alchemical_difference_plan(s, other) is None
    u = s.urey_bradley_params.copy(); u[3, 0] += 0.001
    assert systems.alchemical_difference_plan(s, dataclasses.replace(plain, urey_bradley_params=u)) is None


# ---- 5. the descriptor
def test_ctypes_mirror_of_the_grown_descriptor(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    D, D2 = _abi.BluesSystemExtV3, _abi.BluesSystemExt
    fields = [n for n, _ in D._fields_]
    assert fields[-6:] == ["n_urey_bradley", "urey_bradley_atoms", "urey_bradley_params", "n_impropers", "improper_atoms", "improper_params"]
    probe = tmp_path / "ext_sizes.c"
    probe.write_text('#include "blues_engine.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu ' + "%zu " * len(fields) + '%d %d %d %zu\\n", sizeof(BluesSystemExtV3), '
                     + ", ".join("offsetof(BluesSystemExtV3, %s)" % f for f in fields)
                     + ', BLUES_ABI_VERSION, BLUES_SYSTEM_EXT_SIZE_V1, BLUES_SYSTEM_EXT_SIZE_V2, sizeof(BluesSystemExt)); return 0; }\n')
    exe = tmp_path / "ext_sizes"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields] + [_abi.ABI_VERSION, _abi.SYSTEM_EXT_SIZE_V1, _abi.SYSTEM_EXT_SIZE_V2, ctypes.sizeof(D2)]
    assert _abi.ABI_VERSION == 9
    assert D.n_urey_bradley.offset == _abi.SYSTEM_EXT_SIZE_V2 == D.cmap_torsion_atoms.offset + D.cmap_torsion_atoms.size      # the new fields begin where the struct ended
    assert ctypes.sizeof(D) > _abi.SYSTEM_EXT_SIZE_V2 == ctypes.sizeof(D2) > _abi.SYSTEM_EXT_SIZE_V1
    # the grown struct begins with BluesSystemExt, field for field: a caller compiled against that one stays what it was
    assert fields[:-6] == [n for n, _ in D2._fields_] and all(getattr(D, f).offset == getattr(D2, f).offset for f, _ in D2._fields_)


def test_ext_desc_carries_the_terms():
    s = cc.chamber_divaline()
    d = s.ext_desc()
    n, m = len(s.urey_bradley_atoms), len(s.improper_atoms)
    assert isinstance(d, _abi.BluesSystemExtV3) and d.struct_size == ctypes.sizeof(_abi.BluesSystemExtV3) and d.alchemical_pme_treatment == 0 and d.n_cmap_maps == 0 and d.n_cmap_torsions == 0
    assert d.n_urey_bradley == n and d.n_impropers == m == 5
    assert [d.urey_bradley_atoms[k] for k in range(2 * n)] == s.urey_bradley_atoms.reshape(-1).tolist()
    assert [d.urey_bradley_params[k] for k in range(2 * n)] == s.urey_bradley_params.reshape(-1).tolist()
    assert [d.improper_atoms[k] for k in range(4 * m)] == s.improper_atoms.reshape(-1).tolist()
    assert [d.improper_params[k] for k in range(2 * m)] == s.improper_params.reshape(-1).tolist()
    only = dataclasses.replace(cc.without(s), improper_atoms=s.improper_atoms, improper_params=s.improper_params).ext_desc()
    assert only.n_urey_bradley == 0 and only.n_impropers == 5
    assert cc.without(s).ext_desc() is None


def test_assemble_s23k_solute_copies_the_ligand_terms():
    """the solute builder on a small base (the toluene box, terms on the ligand's ring): the ligand keeps its terms, every inserted
    molecule gets a copy with shifted indices, and removing waters moves no index of either"""
    base, vel = systems.toluene_box()
    base, path = cc.with_ring_terms(base)
    n_lig = len(base.alchemical_atoms)
    assert n_lig == 15 and max(path) < n_lig
    res = np.asarray(base.residue_of_atom)
    waters = [int(np.nonzero(res == r)[0][0]) for r in (3, 7)]
    rng = np.random.default_rng(2)
    ins_x = np.concatenate([base.positions[:n_lig] + d for d in ([0.3, 0.0, 0.0], [0.0, 0.3, 0.0])]); ins_v = rng.normal(size=ins_x.shape)
    s, v = systems.assemble_s23k_solute(base, vel, waters, ins_x, ins_v)
    assert s.n_atoms == base.n_atoms + 2 * n_lig - 6
    for atoms, params, a0, p0 in ((s.urey_bradley_atoms, s.urey_bradley_params, base.urey_bradley_atoms, base.urey_bradley_params),
                                  (s.improper_atoms, s.improper_params, base.improper_atoms, base.improper_params)):
        assert atoms.dtype == np.int32 and atoms.shape == (3 * len(a0), a0.shape[1]) and params.shape == (3 * len(p0), 2)
        assert np.array_equal(atoms, np.concatenate([a0, a0 + n_lig, a0 + 2 * n_lig])) and np.array_equal(params, np.concatenate([p0] * 3))
    s.check_charmm()
    eu0, ei0, _ = ref.energy_forces(base, base.positions, base.box)
    eu, ei, _ = ref.energy_forces(s, s.positions, s.box)          # (the inserted molecules are translated copies: three times the terms)
    assert eu == pytest.approx(3.0 * eu0, rel=1e-12) and ei == pytest.approx(3.0 * ei0, rel=1e-12)
    # a term that reaches into a removed water is dropped, one into a kept water is re-indexed
    far = int(np.nonzero(res == 9)[0][0])
    b2 = dataclasses.replace(base, urey_bradley_atoms=np.array([[0, waters[0]], [1, far]], np.int32), urey_bradley_params=np.array([[0.3, 1.0], [0.4, 2.0]]))
    s2, _ = systems.assemble_s23k_solute(b2, vel, waters, ins_x, ins_v)
    assert s2.urey_bradley_atoms.tolist() == [[1, far + 2 * n_lig - 3 * sum(1 for w in waters if w < far)]] and s2.urey_bradley_params.tolist() == [[0.4, 2.0]]
