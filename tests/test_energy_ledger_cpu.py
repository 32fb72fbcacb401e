"""CPU suite: the measure_shadow_work / measure_heat flags of the Langevin switch (ABI 9) through the host mirror, the ctypes
descriptor and the oracle, which compiles from the same header and ignores the two fields."""
import ctypes

import numpy as np
import pytest

from blues_amd import _abi, integrators

FUNCS = dict(integrators.DEFAULT_ALCHEMICAL_FUNCTIONS)


def test_constructor_accepts_measure_shadow_work_and_to_data_carries_the_flags():
    it = integrators.AlchemicalExternalLangevinIntegrator(FUNCS, measure_shadow_work=True, nsteps_neq=4)
    d = it.to_data()
    assert d.measure_shadow_work == 1 and d.measure_heat == 1        # measure_heat=True is the reference's default
    it = integrators.AlchemicalExternalLangevinIntegrator(FUNCS, measure_shadow_work=True, measure_heat=False, nsteps_neq=4)
    d = it.to_data()
    assert d.measure_shadow_work == 1 and d.measure_heat == 0
    desc, keep = d.to_desc()
    assert desc.measure_shadow_work == 1 and desc.measure_heat == 0


def test_default_arguments_send_neither_flag():
    d = integrators.AlchemicalExternalLangevinIntegrator(FUNCS, nsteps_neq=4).to_data()
    assert d.measure_shadow_work == 0 and d.measure_heat == 0        # the default path does not pay for the reference's measure_heat=True
    d = integrators.generateNCMCIntegrator(nstepsNC=4).to_data()
    assert d.measure_shadow_work == 0 and d.measure_heat == 0
    desc, keep = d.to_desc()
    assert desc.measure_shadow_work == 0 and desc.measure_heat == 0
    d = integrators.generateNCMCIntegrator(nstepsNC=4, measure_shadow_work=True, measure_heat=False).to_data()
    assert d.measure_shadow_work == 1 and d.measure_heat == 0
    one = _abi.IntegratorData(timestep=0.002, temperature=300.0, nsteps_neq=1, lambda_sterics=np.ones(3), lambda_electrostatics=np.ones(3), measure_heat=1)
    assert one.to_desc()[0].measure_heat == 1 and one.to_desc()[0].measure_shadow_work == 0   # heat alone


def test_abi_version_and_descriptor_layout():
    assert _abi.ABI_VERSION == 9
    names = [f[0] for f in _abi.BluesIntegratorDesc._fields_]
    assert names[-2:] == ["measure_shadow_work", "measure_heat"] and names[-4:-2] == ["switching_mode", "steps_per_propagation"]
    assert _abi.BluesIntegratorDesc.measure_heat.offset == _abi.BluesIntegratorDesc.steps_per_propagation.offset + 2 * ctypes.sizeof(ctypes.c_int32)


@pytest.mark.parametrize("flags", [dict(measure_shadow_work=1), dict(measure_heat=1)])
def test_switching_mode_integrator_with_a_flag_is_refused(flags):
    d = _abi.IntegratorData(timestep=0.002, temperature=300.0, nsteps_neq=2, lambda_sterics=np.ones(3), lambda_electrostatics=np.ones(3),
                            switching_mode=_abi.SWITCH_VV, **flags)
    with pytest.raises(ValueError, match="switching_mode"):
        d.to_desc()


def test_oracle_builds_and_steps_from_a_descriptor_with_the_new_fields(oracle_mod, tol_box):
    s, v = tol_box
    it = integrators.generateNCMCIntegrator(nstepsNC=3, dt=0.002, temperature=300.0, seed=3, measure_shadow_work=True)
    plain = integrators.generateNCMCIntegrator(nstepsNC=3, dt=0.002, temperature=300.0, seed=3)
    data = it.to_data(precision=1)
    desc, keep = data.to_desc()
    assert data.measure_shadow_work == 1 and desc.measure_shadow_work == 1 and desc.measure_heat == 1   # (what the oracle is handed carries the fields)
    assert ctypes.sizeof(_abi.BluesIntegratorDesc) >= _abi.BluesIntegratorDesc.measure_heat.offset + 4
    o, p = oracle_mod.Oracle(s, data), oracle_mod.Oracle(s, plain.to_data(precision=1))
    o.set_velocities(v); p.set_velocities(v)
    o.step(3); p.step(3)
    assert o.get_global("protocol_work") == p.get_global("protocol_work")     # the oracle ignores the fields
    assert o.get_global("heat") == p.get_global("heat") and abs(o.get_global("heat")) > 0.0
    assert np.array_equal(o.get_positions(), p.get_positions())
