"""The evaluator's terrain-difficulty ladder on a real MI355X: the device build of the go2nn_ladder_* kernels against the float64 restatement of tests/test_ladder_host.py
(same script, same bounds) at the wave and workgroup edges, graph replay against eager execution with robots that clear in the middle of a captured chunk, and the ladder
of a policy that is known to walk.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_ladder_host as lh  # noqa: E402
from test_gpu_robust import DeviceMemory  # noqa: E402
from go2_rl_gym_amd._nn import GO2NN_LADDER_OUT_NUM  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils import get_args  # noqa: E402

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


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_accumulate_and_reduce_on_the_device(nn, N):
    """one lane, one short of a wave, a whole wave, one more, one more than a 256-lane workgroup; field-major buffers as the HIP simulator keeps them"""
    table, ref = lh.run_script(nn, DeviceMemory(), N, layout=1)
    lh.check_table(table, ref, N, "device N=%d field-major" % N)
    G = 5
    tab, group = lh.reduce_case(N, G)
    t_d, g_d = torch.from_numpy(tab).to(DEV), torch.from_numpy(group).to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((G, GO2NN_LADDER_OUT_NUM), -1.0, dtype=torch.float64, device=DEV)
        assert nn.go2nn_ladder_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, G, lh.DIST2_THR, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    lh.check_reduce(outs[0], tab, group, G, N, "device N=%d" % N)
    # the reduce of the script's own table: the counts of the float64 reference
    grp = (np.arange(N) % 6).astype(np.int32)
    out = torch.zeros(6, GO2NN_LADDER_OUT_NUM, dtype=torch.float64, device=DEV)
    t_d, g_d = torch.from_numpy(np.ascontiguousarray(table)).to(DEV), torch.from_numpy(grp).to(DEV)
    assert nn.go2nn_ladder_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, 6, lh.DIST2_THR, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0
    want, _ = ref.reduce(grp, 6)
    np.testing.assert_array_equal(out.cpu().numpy()[:, :5], want[:, :5])


def test_replay_equals_eager_with_the_ladder(hip, monkeypatch):
    """a captured chunk is 25 steps and is replayed 5 times (one warm-up chunk, four counted ones).  The step counter and every robot's record live in the table, so the SAME
    captured launch takes the origin in one replay, latches robots at different offsets inside later ones and leaves them alone afterwards, as the eager run does"""
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    args = get_args(["--task", "go2", "--num_envs", "64", "--headless"])
    env, _ = task_registry.make_env("go2", args)
    runner, _ = task_registry.make_alg_runner(env, "go2", args, log_root=None)
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True, ladder=True, ladder_distance=0.1)
    ev = PolicyEvaluator(env.cfg, cfg, task_class=type(env), sim_params=env.sim_params, device=env.sim_device)
    ac = runner.alg.actor_critic
    eager = ev.evaluate(ac, use_graph=False)
    t_eager = ev.ltable.cpu().numpy()
    replay = ev.evaluate(ac)
    t_replay = ev.ltable.cpu().numpy()
    again = ev.evaluate(ac, use_graph=False)
    assert (eager["mode"], replay["mode"], again["mode"]) == ("eager", "graph", "eager") and ev.chunk == 25 and ev.steps == 100 and ev.warmup_steps == 25
    for other in (again, replay):
        assert eager["table"].tobytes() == other["table"].tobytes() and eager["ladder_table"].tobytes() == other["ladder_table"].tobytes()
        assert str(eager["ladder"]) == str(other["ladder"]) and str(eager["ladder_summary"]) == str(other["ladder_summary"])
    assert t_eager.tobytes() == t_replay.tobytes()
    # the states sum to the cell sizes, and robots cleared in the middle of a chunk, in more than one chunk
    state, clear_step = t_eager[lh.R["state"]].astype(int), t_eager[lh.R["clear_step"]].astype(int)
    sizes = np.bincount(ev.cell_host, minlength=ev.num_cells)
    lt = eager["ladder_table"]
    np.testing.assert_array_equal(lt[:, lh.O["n"]], sizes)
    running = np.bincount(ev.cell_host, weights=(state == lh.RUNNING), minlength=ev.num_cells)
    np.testing.assert_array_equal(running + lt[:, lh.O["cleared"]] + lt[:, lh.O["fell"]] + lt[:, lh.O["timed_out"]], sizes)
    assert (t_eager[lh.R["step"]] == ev.steps).all() and np.isfinite(eager["table"]).all() and eager["table"][:, 0].sum() == 256 * ev.steps
    at = clear_step[state == lh.CLEARED] - 1          # the counted step at which each cleared robot cleared
    print("states: %s; cleared at steps %s" % (np.bincount(state, minlength=4).tolist(), np.bincount(at // 25, minlength=4).tolist()))
    assert len(at) > 0 and (at % 25 != 0).any() and len(set((at // 25).tolist())) > 1, sorted(at.tolist())
    ev.close(); env.close()


def test_ladder_of_the_pretrained_student(hip):
    """the committed pretrained CTS student on go2_cts, the default evaluation with the ladder on: 1024 robots over every terrain kind x 10 levels, forward 1 m/s for 10 s,
    4 m (half a tile) to cover.  On the flat kind — the same ground at every level — it walks 0.97 m/s without a fall, 9.7 m against those 4 m: every
    level cleared by every robot.  No bound on any other terrain kind: those figures are what the run is there to show"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator, format_table
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    m, _ = pretrained_policy()
    m = m.to(DEV)
    env_cfg, train_cfg = task_registry.get_cfgs("go2_cts")
    ev = PolicyEvaluator(env_cfg, dict(class_to_dict(train_cfg.evaluation), ladder=True), task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    res = ev.evaluate(m)
    print(format_table(res))
    for t, d in res["ladder_summary"].items():
        print("%-14s level_cleared %2d mean_level_cleared %.3f" % (t, d["level_cleared"], d["mean_level_cleared"]))
    assert ev.ladder_distance == 4.0 and res["levels"] == list(range(10)) and res["scenarios"] == ["forward_1.0"] and "flat" in res["ladder"]
    for t, levels in res["ladder"].items():
        for lv, per in levels.items():
            for s, cell in per.items():
                assert cell["n_envs"] > 0 and cell["cleared"] + cell["fell"] + cell["timed_out"] <= 1, (t, lv, s, cell)
    assert all(res["ladder"]["flat"][lv]["forward_1.0"]["cleared"] == 1.0 for lv in res["levels"]), res["ladder"]["flat"]
    assert res["ladder_summary"]["flat"]["level_cleared"] == res["levels"][-1]
    ev.close()
