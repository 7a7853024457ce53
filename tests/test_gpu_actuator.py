"""The evaluator's actuator loads on a real MI355X: the device build of the go2nn_actuator_* kernels against the float64 restatement of tests/test_actuator_host.py (same
script, same bounds) at the wave and workgroup edges, the reduce and the bootstrap against the host build bit for bit, graph replay against eager execution with the
pretrained student, and the actuator table of the default evaluation.  Run with -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip, load_nn_emu  # noqa: E402
import test_actuator_host as ah  # noqa: E402
import test_bootstrap_host as tb  # noqa: E402
import test_bootstrap_modes_host as tm  # noqa: E402
from test_gpu_bootstrap_modes import DeviceBackend  # noqa: E402
from test_gpu_robust import DeviceMemory  # noqa: E402
from go2_rl_gym_amd._nn import GO2NN_ACTUATOR_OUT_NUM, actuator_out_col  # noqa: E402
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
    out = torch.full((G, GO2NN_ACTUATOR_OUT_NUM), -1.0, dtype=torch.float64, device=DEV)
    assert nn.go2nn_actuator_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, G, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0, nn.go2nn_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_accumulate_reduce_and_bootstrap_on_the_device(nn, N):
    """one lane, one short of a wave, a whole wave, one more, one more than a 256-lane workgroup; field-major buffers as the HIP simulator keeps them"""
    emu = load_nn_emu()
    table, ref, wrote = ah.run_script(nn, DeviceMemory(), N, layout=1)
    ah.check_table(table, ref, wrote, N, "device N=%d field-major" % N)
    G = 5
    for tab, group in (ah.reduce_case(N, G), (table, (np.arange(N) % 4).astype(np.int32))):          # a random table; the script's own, grouped by its patterns
        outs = [device_reduce(nn, tab, group, G) for _ in range(2)]
        assert outs[0].tobytes() == outs[1].tobytes()
        assert outs[0].tobytes() == ah.emu_reduce(emu, np.ascontiguousarray(tab), group, G).tobytes()
    for G in (1, 5):
        tab, group = ah.reduce_case(N, G)
        ah.check_reduce(device_reduce(nn, tab, group, G), tab, group, G, N, "device N=%d G=%d" % (N, G))
    dev, host = DeviceBackend(nn), tm.HostBackend(emu)
    for G in (1, 5):          # the script's own table, its robots dealt to G cells in turn: the device's replicates are the host build's, bit for bit
        start, envs = tb.csr((np.arange(N) % G).astype(np.int32), G)
        for B in (1, 257):
            got, want = tm.bootstrap(dev, ah.FAMILY, table, start, envs, B, tm.SEED), tm.bootstrap(host, ah.FAMILY, table, start, envs, B, tm.SEED)
            assert got.shape == (B, G, GO2NN_ACTUATOR_OUT_NUM) and got.tobytes() == want.tobytes(), (N, G, B)


def forward_groups(ev):
    return [gi for gi, (_, s) in enumerate(ev.groups) if s == "forward_1.0"]


def test_replay_equals_eager_with_actuators(hip, monkeypatch):
    """a captured chunk is 25 steps and is replayed 5 times (one warm-up chunk, four counted ones).  The step counter lives in the table, so the SAME captured launch skips
    the warm-up in one replay and counts in the later ones, as the eager run does"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    m, _ = pretrained_policy()
    m = m.to(DEV)
    env_cfg, _ = task_registry.get_cfgs("go2_cts")
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True, actuators=True, record=1)
    ev = PolicyEvaluator(env_cfg, cfg, task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    eager = ev.evaluate(m, use_graph=False)
    t_eager = ev.act_table.cpu().numpy()
    ah.check_recorded_robots(ev, eager, "eager")
    ah.check_actuator_result(ev, eager, "eager")
    replay = ev.evaluate(m)
    t_replay = ev.act_table.cpu().numpy()
    ah.check_recorded_robots(ev, replay, "replayed")
    again = ev.evaluate(m, use_graph=False)
    assert (eager["mode"], replay["mode"], again["mode"]) == ("eager", "graph", "eager") and ev.chunk == 25 and ev.steps == 100 and ev.warmup_steps == 25
    assert t_eager.tobytes() == t_replay.tobytes() == ev.act_table.cpu().numpy().tobytes()
    for other in (replay, again):
        assert eager["actuator_table"].tobytes() == other["actuator_table"].tobytes() and eager["table"].tobytes() == other["table"].tobytes()
        assert eager["actuator_extremes"].tobytes() == other["actuator_extremes"].tobytes()
        assert eager["trace"]["frames"].tobytes() == other["trace"]["frames"].tobytes() and str(eager["actuators"]) == str(other["actuators"])
    # the run has shown something: the robots told to walk are all counted, do positive work, travel and load their motors
    groups = forward_groups(ev)
    rows = eager["actuator_table"][groups]
    ids = np.nonzero(np.isin(ev.group_host, groups))[0]
    work, dist = sum(rows[:, actuator_out_col("work_pos", j)].sum() for j in range(12)), rows[:, actuator_out_col("dist")].sum()
    peaks = [eager["actuators"]["groups"][t][s]["torque_peak"] for t, s in (ev.groups[g] for g in groups)]
    print("forward_1.0 groups: %d robots, positive work sum %.1f, distance sum %.1f (x dt), torque_peak %s" % (len(ids), work, dist, [round(p, 2) for p in peaks]))
    assert len(rows) > 0 and (t_eager[ah.actuator_row("used"), ids] > 0).all() and work > 0 and dist > 0 and all(p > 0 for p in peaks)
    ev.close()


def test_actuators_of_the_pretrained_student_full_evaluation(hip):
    """the committed pretrained CTS student on go2_cts, the default evaluation (1024 robots, every terrain kind x six commands, 10 s) with the actuator and gait scorers on: the
    table is printed — these figures are what the run is there to show — and only its structure is asserted"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator, format_table
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    m, _ = pretrained_policy()
    env_cfg, train_cfg = task_registry.get_cfgs("go2_cts")
    ev = PolicyEvaluator(env_cfg, dict(class_to_dict(train_cfg.evaluation), actuators=True, gait=True), task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    res = ev.evaluate(m.to(DEV))
    print(format_table(res))
    o = res["actuators"]["overall"]
    print("overall per joint: %s" % {k: round(v, 4) for k, v in o.items() if k.split("/")[0] in ("torque_rms", "torque_peak_max", "torque_saturation", "limit_margin_min") and "_" in k.split("/")[-1]})
    ah.check_actuator_result(ev, res, "default evaluation")
    leaves = [o] + [d for per in res["actuators"]["groups"].values() for d in per.values()]
    limits = dict(zip(ev.joint_names, ev.act_torque_limits.tolist()))
    for d in leaves:
        for k, v in d.items():
            if k.split("/")[0] in ("torque_saturation", "joint_speed_saturation", "torque_rms_share"):
                assert math.isnan(v) or 0.0 <= v <= 1.0, (k, v)
        for name, limit in limits.items():          # the simulator clips the applied torque at the joint's limit
            peak, top, rms = d["torque_peak/" + name], d["torque_peak_max/" + name], d["torque_rms/" + name]
            assert math.isnan(peak) or (peak <= top <= limit * (1 + 1e-6) and rms <= top), (name, peak, top, rms, limit)
        assert math.isnan(d["torque_rms"]) or d["torque_rms"] <= d["torque_peak_max"]
    assert o["n_envs"] == 1024 and ev.steps == 500
    ev.close()
