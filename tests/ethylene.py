"""The reference's known-answer System (blues/tests/test_ethylene.py; fixture tests/golden/ethylene_system.json) and a second System with
the same two custom forces, in the form the HIP engine takes them: the TYPED fields SystemData.custom_pair_mode / .centroid_bonds.

A charged ethylene (atoms 2-7: alchemical, mobile, C-H bonds constrained) between two frozen charge sites (atoms 0, 1), NoCutoff.  Its
CustomNonbondedForce acts between the two sites and the ethylene only (q/r^2 + a 12-6 term whose sigma is scaled by lambda_sterics and
whose epsilon by lambda_electrostatics); a CustomCentroidBondForce ties the centroid of the two carbons to that of the two sites.

The CPU oracle does not read the typed fields: configure_oracle() sets the same forces through its own setters, and extras_form()
returns the System as the oracle-backed test doubles of tests/conftest.py want it (SystemData.extras, typed fields cleared), so a GPU
test can hold the engine against the oracle without touching either.
"""
import dataclasses
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAIR_ENERGY = "q/(r^2) + 4*epsilon*((sigma/r)^12-(sigma/r)^6)"


def load():
    """(SystemData with the typed custom-force fields, the test protocol of the fixture)."""
    from blues_amd import _abi
    with open(os.path.join(GOLDEN, "ethylene_system.json")) as fh:
        d = json.load(fh)
    cn, cb = d["custom_nonbonded"], d["centroid_bond"]
    assert cn["energy"].startswith(PAIR_ENERGY) and cn["method"] == 0 and cb["energy"] == "0.5*k*distance(g1,g2)^2"
    par = np.array(cn["particles"])
    masses = np.array(d["masses"])
    groups = []
    for g in cb["groups"]:
        idx = [int(p[0]) for p in g]
        w = [float(p[1]) if p[1] is not None else float(masses[p[0]]) for p in g]      # OpenMM's default weight: the particle's mass
        groups.append((idx, w))
    s = _abi.SystemData(
        box=np.array(d["box"]), mass=masses, charge=par[:, 2], sigma=par[:, 0], epsilon=par[:, 1],
        bond_atoms=np.array([b[:2] for b in d["bonds"]], np.int32), bond_params=np.array([b[2:] for b in d["bonds"]]),
        angle_atoms=np.array([a[:3] for a in d["angles"]], np.int32), angle_params=np.array([a[3:] for a in d["angles"]]),
        torsion_atoms=np.array([t[:4] for t in d["torsions"]], np.int32), torsion_params=np.array([t[4:] for t in d["torsions"]], float),
        constraint_atoms=np.array([c[:2] for c in d["constraints"]], np.int32), constraint_dist=np.array([c[2] for c in d["constraints"]]),
        alchemical_atoms=np.array(d["test"]["alchemical_atoms"], np.int32), nonbonded_method=_abi.NB_NOCUTOFF, cutoff=1.0,
        remove_cm_motion=False, positions=np.array(d["positions_nm"]),
        custom_pair_mode=_abi.PAIR_ETHYLENE,
        centroid_bonds=((groups[0][0], groups[0][1], groups[1][0], groups[1][1], float(cb["k"])),))
    assert cn["set1"] == [0, 1] and cn["set2"] == list(s.alchemical_atoms)
    return s, d["test"]


def divaline(frozen=False):
    """vacDivaline (35 atoms, NoCutoff, HBonds, side chain 22-31 alchemical: tests/test_nocutoff_cpu.py) with the pair form and two
    centroid bonds of unequal weights: backbone of residue 1 against its side chain (stiff, unequal explicit weights), and a group of
    three against a single atom (soft; one atom sits in both bonds).  frozen: the non-alchemical atoms 0-5 and 14 have mass 0, members of both
    bonds among them."""
    from blues_amd import amber
    prm = amber.read_prmtop(os.path.join(GOLDEN, "vacDivaline.prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "vacDivaline.inpcrd"))
    s = amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=list(range(22, 32)), nonbonded_method="NoCutoff")
    bonds = (([4, 6, 8, 10], [1.0, 2.5, 0.5, 3.0], [22, 24, 26, 28, 30], [12.0, 1.0, 0.25, 4.0, 2.0], 850.0),
             ([0, 14, 24], [3.0, 1.0, 2.0], [33], [0.7], 120.0))
    s = dataclasses.replace(s, custom_pair_mode=1, centroid_bonds=bonds)
    if frozen:
        m = s.mass.copy(); m[[0, 1, 2, 3, 4, 5, 14]] = 0.0
        # (constraints between a frozen and a mobile atom are not what this fixture is about: drop every constraint that touches a frozen atom)
        keep = np.array([m[a] != 0.0 and m[b] != 0.0 for a, b in s.constraint_atoms], bool)
        s = dataclasses.replace(s, mass=m, constraint_atoms=s.constraint_atoms[keep], constraint_dist=s.constraint_dist[keep])
    return s


def configure_oracle(o, s):
    """The custom forces of `s` (typed fields) on an oracle.Oracle made from the same SystemData."""
    if s.custom_pair_mode:
        o.set_custom_pair_mode(int(s.custom_pair_mode))
    for idx1, w1, idx2, w2, k in s.centroid_bonds:
        o.add_centroid_bond(list(idx1), list(w1), list(idx2), list(w2), float(k))
    return o


def make_oracle(oracle_mod, s, data):
    return configure_oracle(oracle_mod.Oracle(s, data), s)


def extras_form(s):
    """The same System for the oracle-backed test doubles (tests/conftest.py: OracleBackedEngine reads SystemData.extras only): the
    custom forces in `extras`, the typed fields cleared."""
    ex = {"custom_pair_mode": int(s.custom_pair_mode), "centroid_bonds": [tuple(b) for b in s.centroid_bonds]}
    return dataclasses.replace(s, custom_pair_mode=0, centroid_bonds=(), extras=ex)


class DistanceReporter(object):
    """|x_i - x_j| of every MD report (the reference's observable: blues/tests/test_ethylene.py:121-131)."""

    def __init__(self, interval, i, j):
        self.interval, self.i, self.j, self.dist = interval, i, j, []

    def describeNextReport(self, simulation):
        return (self.interval - simulation.currentStep % self.interval, True, False, False, False)

    def report(self, simulation, state):
        x = state.getPositions(asNumpy=True)._value
        self.dist.append(float(np.linalg.norm(x[self.i] - x[self.j])))


def build_chain(context_module, s, t, r, seed0, **sim_kw):
    """One chain of the known-answer protocol (tests/test_ethylene_known_answer.py: _run_repeat, the reference's triple of Simulations
    on ONE System, thermostats at t["temperature"]) with streams of its own, all derived from seed0 and r.  Returns (chain, reporter)."""
    from blues_amd import integrators, moves, simulation
    seed = int(seed0) + 1009 * int(r)
    md_int = integrators.LangevinIntegrator(t["temperature"], t["friction"], t["dt"], seed=seed)
    alch_int = integrators.LangevinIntegrator(t["temperature"], t["friction"], t["dt"], seed=seed + 1)
    ncmc_int = integrators.AlchemicalExternalLangevinIntegrator(nsteps_neq=t["nstepsNC"], alchemical_functions=integrators.DEFAULT_ALCHEMICAL_FUNCTIONS,
                                                                splitting=t["splitting"], temperature=t["temperature"], timestep=t["dt"], seed=seed + 7919)
    md = context_module.Simulation(None, s, md_int, replica=r, **sim_kw)
    alch = context_module.Simulation(None, s, alch_int, replica=r, **sim_kw)
    ncmc = context_module.Simulation(None, s, ncmc_int, replica=r, **sim_kw)
    for sim, integ in ((md, md_int), (alch, alch_int), (ncmc, ncmc_int)):
        sim.context.setVelocitiesToTemperature(integ.getTemperature(), seed + 2)
    rep = DistanceReporter(t["reportInterval"], *t["distance_atoms"])
    md.reporters.append(rep)
    lig = list(s.alchemical_atoms)
    mover = moves.MoveEngine(moves.RandomLigandRotationMove(lig, s.mass[lig], random_state=np.random.RandomState(seed + 31)))
    cfg = {"nIter": t["nIter"], "nstepsNC": t["nstepsNC"], "nstepsMD": t["nstepsMD"], "moveStep": t["moveStep"]}
    chain = simulation.BLUESSimulation(simulation.SimulationSet(ncmc, md=md, alch=alch), cfg, mover, rng=np.random.RandomState(seed + 77))
    return chain, rep


def run_known_answer(context_module, s, t, R, seed0, make_all=None, **sim_kw):
    """R chains of the protocol through BatchedBLUESSimulation (MD velocities re-drawn at the driver's default 300 K: the reference's
    quirk, blues/tests/test_ethylene.py:104).  Returns (per-chain fraction of MD reports with |x0 - x2| <= cut, per-chain acceptance
    rate, the retired chains)."""
    from blues_amd import simulation
    build = lambda r: build_chain(context_module, s, t, r, seed0, **sim_kw)
    pairs = make_all(build, R) if make_all is not None else [build(r) for r in range(R)]
    chains, reps = [p[0] for p in pairs], [p[1] for p in pairs]
    B = simulation.BatchedBLUESSimulation(chains, isolate_failures=True)
    B.run(nIter=t["nIter"], nstepsNC=t["nstepsNC"], moveStep=t["moveStep"], nstepsMD=t["nstepsMD"])
    n_rep = t["nIter"] * t["nstepsMD"] // t["reportInterval"]
    dead = dict(B.dead)
    frac = np.array([np.mean(np.array(rp.dist) <= t["distance_cut_nm"]) if len(rp.dist) == n_rep else np.nan for rp in reps])
    acc = np.array([c.accept / float(t["nIter"]) for c in chains])
    B.close()
    return frac, acc, dead
