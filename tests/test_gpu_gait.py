"""The evaluator's gait scores on a real MI355X: the device build of the go2nn_gait_* kernels against the float64 restatement of tests/test_gait_host.py (same script, same
bounds) at the wave and workgroup edges, the reduce against the host build bit for bit, graph replay against eager execution with the pretrained student — whose feet touch
down in the middle of captured chunks —, and the gait table of the default evaluation.  Run with -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip, load_nn_emu  # noqa: E402
import test_gait_host as gh  # noqa: E402
from test_gpu_robust import DeviceMemory  # noqa: E402
from go2_rl_gym_amd._nn import GO2NN_GAIT_OUT_NUM, gait_out_col  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.fixture(scope="module")
def nn(hip):
    from go2_rl_gym_amd._nn import load_nn
    return load_nn()


def device_reduce(nn, table, group, G):
    N = table.shape[1]
    t_d, g_d = torch.from_numpy(np.ascontiguousarray(table)).to(DEV), torch.from_numpy(group).to(DEV)
    out = torch.full((G, GO2NN_GAIT_OUT_NUM), -1.0, dtype=torch.float64, device=DEV)
    assert nn.go2nn_gait_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, G, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0, nn.go2nn_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_accumulate_and_reduce_on_the_device(nn, N):
    """one lane, one short of a wave, a whole wave, one more, one more than a 256-lane workgroup; field-major buffers as the HIP simulator keeps them"""
    emu = load_nn_emu()
    table, ref, _ = gh.run_script(nn, DeviceMemory(), N, layout=1)
    gh.check_table(table, ref, N, "device N=%d field-major" % N)
    G = 5
    for tab, group in (gh.reduce_case(N, G), (table, (np.arange(N) % 4).astype(np.int32))):          # a random table; the script's own, grouped by its four patterns
        outs = [device_reduce(nn, tab, group, G) for _ in range(2)]
        assert outs[0].tobytes() == outs[1].tobytes()
        assert outs[0].tobytes() == gh.emu_reduce(emu, np.ascontiguousarray(tab), group, G).tobytes()
    if N >= 63:
        tab, group = gh.reduce_case(N, G)
        gh.check_reduce(device_reduce(nn, tab, group, G), tab, group, G, N, "device N=%d" % N)


def forward_groups(ev):
    return [gi for gi, (_, s) in enumerate(ev.groups) if s == "forward_1.0"]


def test_replay_equals_eager_with_gait(hip, monkeypatch):
    """a captured chunk is 25 steps and is replayed 5 times (one warm-up chunk, four counted ones).  The step counter and every foot's phase live in the table, so the SAME
    captured launch skips the warm-up in one replay and follows touchdowns and lift-offs at any offset inside the later ones, as the eager run does"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    m, _ = pretrained_policy()
    m = m.to(DEV)
    env_cfg, _ = task_registry.get_cfgs("go2_cts")
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True, gait=True, record=1)
    ev = PolicyEvaluator(env_cfg, cfg, task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    eager = ev.evaluate(m, use_graph=False)
    t_eager = ev.gtable.cpu().numpy()
    gh.check_recorded_robots(ev, eager, "eager")
    gh.check_gait_result(ev, eager, "eager")
    replay = ev.evaluate(m)
    t_replay = ev.gtable.cpu().numpy()
    gh.check_recorded_robots(ev, replay, "replayed")
    again = ev.evaluate(m, use_graph=False)
    assert (eager["mode"], replay["mode"], again["mode"]) == ("eager", "graph", "eager") and ev.chunk == 25 and ev.steps == 100 and ev.warmup_steps == 25
    assert t_eager.tobytes() == t_replay.tobytes() == ev.gtable.cpu().numpy().tobytes()
    for other in (replay, again):
        assert eager["gait_table"].tobytes() == other["gait_table"].tobytes() and eager["table"].tobytes() == other["table"].tobytes()
        assert eager["trace"]["frames"].tobytes() == other["trace"]["frames"].tobytes() and str(eager["gait"]) == str(other["gait"])
    # the run has shown something: the robots told to walk touch down and stride
    rows = eager["gait_table"][forward_groups(ev)]
    tds, strides = sum(rows[:, gait_out_col(f, "touchdowns")].sum() for f in range(4)), sum(rows[:, gait_out_col(f, "strides")].sum() for f in range(4))
    print("forward_1.0 groups: %d touchdowns, %d strides" % (tds, strides))
    assert len(rows) > 0 and tds > 0 and strides >= 1
    ev.close()


def test_gait_of_the_pretrained_student_full_evaluation(hip):
    """the committed pretrained CTS student on go2_cts, the default evaluation (1024 robots, every terrain kind x six commands, 10 s) with gait on: the table is printed —
    these figures are what the run is there to show — and only its structure is asserted"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import GAIT_KEYS, PolicyEvaluator, format_table
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    m, _ = pretrained_policy()
    env_cfg, train_cfg = task_registry.get_cfgs("go2_cts")
    ev = PolicyEvaluator(env_cfg, dict(class_to_dict(train_cfg.evaluation), gait=True, record=1), task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    res = ev.evaluate(m.to(DEV))
    print(format_table(res))
    print("overall per foot: %s" % {k: round(v, 4) for k, v in res["gait"]["overall"].items() if "/" in k})
    gh.check_gait_result(ev, res, "default evaluation")          # support sums to used, diagonal <= support[2], phases need touchdowns, the partitions add up to overall
    gh.check_recorded_robots(ev, res, "default evaluation")
    leaves = [res["gait"]["overall"]] + [d for per in res["gait"]["groups"].values() for d in per.values()]
    for d in leaves:
        for k, v in d.items():
            if k.startswith("duty_factor") or k in ("trot_share", "flight_share"):
                assert math.isnan(v) or 0.0 <= v <= 1.0, (k, v)
        assert set(GAIT_KEYS) < set(d) and (math.isnan(d["mean_feet_in_contact"]) or 0.0 <= d["mean_feet_in_contact"] <= 4.0)
    assert res["gait"]["overall"]["n_envs"] == 1024 and ev.steps == 500
    ev.close()
