"""Records what amber.system_from_amber makes of the two Amber fixtures, array by array, into tests/golden/amber_arrays.npz.

The file in the repository was written by the commit BEFORE the chamber reader (run with that commit's blues_amd on the path):
tests/test_charmm_cpu.py holds every later reader to those bits for a non-chamber prmtop.  Running this script again overwrites the
record with the current reader's output, which is only right for a change that means to alter it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))

from blues_amd import amber  # noqa: E402

FIELDS = ("box", "mass", "charge", "sigma", "epsilon", "exclusions", "exception_atoms", "exception_params", "bond_atoms", "bond_params",
          "angle_atoms", "angle_params", "torsion_atoms", "torsion_params", "constraint_atoms", "constraint_dist", "alchemical_atoms",
          "pme_grid", "ewald_alpha", "residue_of_atom", "positions")
CASES = {
    "vacDivaline": ("vacDivaline", dict(constraints="HBonds", alchemical_atoms=list(range(22, 32)), nonbonded_method="NoCutoff")),
    "vacDivaline_free": ("vacDivaline", dict(constraints=None, nonbonded_method="NoCutoff")),
    "TOL-parm": ("TOL-parm", dict(constraints="HBonds", hydrogen_mass=3.024, alchemical_atoms=list(range(15)))),
}


def arrays(case):
    name, kw = CASES[case]
    prm = amber.read_prmtop(os.path.join(HERE, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(HERE, name + ".inpcrd"))
    s = amber.system_from_amber(prm, pos, box, **kw)
    return {f: np.asarray(getattr(s, f)) for f in FIELDS}


if __name__ == "__main__":
    out = {"%s/%s" % (c, f): a for c in CASES for f, a in arrays(c).items()}
    np.savez_compressed(os.path.join(HERE, "amber_arrays.npz"), **out)
    print("wrote %d arrays" % len(out))
