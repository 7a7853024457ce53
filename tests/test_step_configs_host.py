"""The step lanes' host build (helpers.load_emu: the kernel's lane source compiled by g++) against the oracle at non-default physics settings and on the joint-limit and
twist-clamp rows: the CPU twin of tests/test_gpu_step_configs.py.  It proves the case table, the reach conditions and the gates of step_config_cases.py without a GPU;
the wave ballots, the LDS row parking and -ffast-math exist on the device only."""
import pytest

import step_config_cases as K
from helpers import HostSim, load_emu


@pytest.fixture(scope="module")
def emu():
    return load_emu()


@pytest.mark.parametrize("name", list(K.CASES))
def test_step_config_on_the_host_build(emu, name):
    stats = K.run_case(emu, HostSim, None, name)
    assert stats["reach"]["env_steps"] == stats["envs"] * K.STEPS


@pytest.mark.parametrize("control_type", K.TORQUE_CONTROL_TYPES)
@pytest.mark.parametrize("decimation", K.TORQUE_DECIMATIONS)
def test_torque_trace_at_other_decimations_on_the_host_build(emu, decimation, control_type):
    K.torque_case(emu, HostSim, None, decimation, control_type)
