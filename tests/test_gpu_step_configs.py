"""go2_step_kernel on the MI355X against the oracle at physics settings other than go2sim_default_cfg — substep and sweep counts, time step, armature, tilted gravity, the
contact-row parameters, every randomisation off — and on the rows the default settings hardly reach (joint stops, the twist clamp); the delay select and the torque law
at decimations other than 4.  The cases, the gates and the reach conditions are step_config_cases.py's, proven on the host build by tests/test_step_configs_host.py;
what only the device has is the wave ballots, the LDS row parking and -ffast-math.  The statistics of every case are printed and collected in one JSON file: the path in
GO2_STEP_CONFIG_REPORT if that is set (profiles/step_config_parity.json is a copy of such a run), a file in pytest's temporary directory otherwise.  Run with -m gpu."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

import step_config_cases as K  # noqa: E402
from helpers import DeviceSim, load_hip  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    """-> record(stats): adds one case's statistics to the report, which starts empty with every run of this module"""
    path = os.environ.get("GO2_STEP_CONFIG_REPORT") or str(tmp_path_factory.mktemp("step_configs") / "step_configs.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    report = {}

    def add(stats):
        report[stats["case"]] = stats
        with open(path, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
    yield add
    print("[step configs] statistics of %d cases in %s" % (len(report), path))


@pytest.mark.parametrize("name", list(K.CASES))
def test_step_config_on_gpu(hip, record, name):
    stats = K.run_case(hip, DeviceSim, DEV, name, record=record)
    assert stats["reach"]["env_steps"] == stats["envs"] * K.STEPS


@pytest.mark.parametrize("control_type", K.TORQUE_CONTROL_TYPES)
@pytest.mark.parametrize("decimation", K.TORQUE_DECIMATIONS)
def test_torque_trace_at_other_decimations_on_gpu(hip, decimation, control_type):
    K.torque_case(hip, DeviceSim, DEV, decimation, control_type)
