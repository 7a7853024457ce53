"""The evaluator's scripted command maneuvers on a real MI355X: the device build of the go2nn_maneuver_* kernels against the float64 restatement of
tests/test_maneuver_host.py (same script, same bounds) at the wave and workgroup edges, graph replay against eager execution with command switches in the middle of two
different captured chunks, the one-segment equivalence with the plain evaluation, and the default maneuvers of a policy that is known to walk.  Run with -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_maneuver_host as mh  # noqa: E402
from test_gpu_robust import DeviceMemory  # noqa: E402
from go2_rl_gym_amd._nn import GO2NN_MANEUVER_ACC_NUM  # noqa: E402
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
def test_apply_accumulate_and_reduce_on_the_device(nn, N):
    """one lane, one short of a wave, a whole wave, one more, one more than a 256-lane workgroup; field-major buffers as the HIP simulator keeps them"""
    table, ref, man = mh.run_script(nn, DeviceMemory(), N, layout=1)
    mh.check_table(table, ref, man, N, "device N=%d field-major" % N)
    G = 5
    tab, group = mh.reduce_case(N, G)
    t_d, g_d = torch.from_numpy(tab).to(DEV), torch.from_numpy(group).to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((G, GO2NN_MANEUVER_ACC_NUM + 1), -1.0, dtype=torch.float64, device=DEV)
        assert nn.go2nn_maneuver_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, G, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    mh.check_reduce(outs[0], tab, group, G, N, "device N=%d" % N)
    # the reduce of the script's own table: the counts of the float64 reference
    grp = (np.arange(N) % mh.PATTERNS).astype(np.int32)
    out = torch.zeros(mh.PATTERNS, GO2NN_MANEUVER_ACC_NUM + 1, dtype=torch.float64, device=DEV)
    t_d, g_d = torch.from_numpy(np.ascontiguousarray(table)).to(DEV), torch.from_numpy(grp).to(DEV)
    assert nn.go2nn_maneuver_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, mh.PATTERNS, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0
    want, _ = mh.reduce_reference(ref.t, grp, mh.PATTERNS)
    for k in ("switches", "switch_falls", "settled", "settle_steps", "win_steps", "n"):
        np.testing.assert_array_equal(out.cpu().numpy()[:, mh.O[k]], want[:, mh.O[k]], err_msg=k)


# dt = 0.02 s: a switch at counted step 35 (every maneuver) and one at 65 (the second and the third); W = 25, H = 5
REPLAY_MANEUVERS = [["brake", [[0.0, 1.0, 0.0, 0.0], [0.7, 0.0, 0.0, 0.0]]], ["zigzag", [[0.0, 0.0, 0.5, 0.0], [0.7, 0.0, -0.5, 0.5], [1.3, 0.5, 0.0, -1.0]]],
                    ["stop_and_go", [[0.0, 1.0, 0.0, 0.0], [0.7, 0.0, 0.0, 0.0], [1.3, 1.0, 0.0, 0.0]]]]


def test_replay_equals_eager_with_maneuvers(hip, monkeypatch):
    """a captured chunk is 25 steps and is replayed 5 times (one warm-up chunk, four counted ones).  The step counter and every robot's window live in the table and the
    schedule is a function of that counter, so the SAME captured pair of launches holds the command in one replay, switches it 10 and 15 steps into two later ones and
    scores the windows that straddle the chunks' ends, as the eager run does"""
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    args = get_args(["--task", "go2_flat", "--num_envs", "64", "--headless"])
    env, _ = task_registry.make_env("go2_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True, maneuvers=REPLAY_MANEUVERS,
               maneuver_window_s=0.5, maneuver_hold_s=0.1)
    ev = PolicyEvaluator(env.cfg, cfg, task_class=type(env), sim_params=env.sim_params, device=env.sim_device)
    ac = runner.alg.actor_critic
    eager = ev.evaluate(ac, use_graph=False)
    t_eager = ev.mtable.cpu().numpy()
    replay = ev.evaluate(ac)
    t_replay = ev.mtable.cpu().numpy()
    again = ev.evaluate(ac, use_graph=False)
    assert (eager["mode"], replay["mode"], again["mode"]) == ("eager", "graph", "eager") and ev.chunk == 25 and ev.steps == 100 and ev.warmup_steps == 25
    assert (ev.maneuver_window, ev.maneuver_hold) == (25, 5) and eager["switch_steps"] == {"brake": [35], "zigzag": [35, 65], "stop_and_go": [35, 65]}
    for other in (again, replay):
        assert eager["table"].tobytes() == other["table"].tobytes() and eager["maneuver_table"].tobytes() == other["maneuver_table"].tobytes()
        assert str(eager["groups"]) == str(other["groups"]) and str(eager["maneuvers"]) == str(other["maneuvers"]) and str(eager["overall"]) == str(other["overall"])
    assert t_eager.tobytes() == t_replay.tobytes() == ev.mtable.cpu().numpy().tobytes()
    # both switches fall strictly inside a chunk, in different chunks (counted step s is step s + 25 of the run: chunks of 25 either way)
    inside = [(s // ev.chunk, s % ev.chunk) for s in (35, 65)]
    assert all(0 < off < ev.chunk - 1 for _, off in inside) and inside[0][0] != inside[1][0], inside
    sizes = np.bincount(ev.cell_host, minlength=ev.num_cells)
    mt = eager["maneuver_table"]
    np.testing.assert_array_equal(mt[:, mh.O["n"]], sizes)
    np.testing.assert_array_equal(mt[:, mh.O["switches"]], sizes * np.asarray([1, 2, 2]))
    assert (t_eager[mh.R["step"]] == ev.steps).all() and (t_eager[mh.R["open"]] == 0).all() and np.isfinite(eager["table"]).all() and eager["table"][:, 0].sum() == 256 * ev.steps
    assert (mt[:, mh.O["settled"]] <= mt[:, mh.O["switches"]]).all() and (mt[:, mh.O["win_steps"]] <= 25 * mt[:, mh.O["switches"]]).all() and np.isfinite(mt).all()
    print("per maneuver: %s" % {n: {k: d[k] for k in ("switches", "switch_falls", "settled", "settle_time_s")} for n, d in eager["maneuvers"].items()})
    ev.close(); env.close()


def test_one_segment_maneuvers_are_the_scenarios_on_the_device(hip):
    """a maneuver of one segment per default scenario: the two kernels write what the copy of the commands wrote, and the evaluation is the plain one, byte for byte"""
    from go2_rl_gym_amd.utils.evaluator import DEFAULT_SCENARIOS, PolicyEvaluator
    args = get_args(["--task", "go2_flat", "--num_envs", "64", "--headless"])
    env, _ = task_registry.make_env("go2_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=1.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None)
    results = []
    for over in ({}, {"maneuvers": [[s[0], [[0.0] + list(s[1:4])]] for s in DEFAULT_SCENARIOS]}):
        ev = PolicyEvaluator(env.cfg, dict(cfg, **over), task_class=type(env), sim_params=env.sim_params, device=env.sim_device)
        results.append(ev.evaluate(runner.alg.actor_critic))
        assert hasattr(ev, "mtable") == bool(over)
        ev.close()
    plain, one = results
    assert plain["table"].tobytes() == one["table"].tobytes() and plain["scenarios"] == one["scenarios"] and "maneuvers" not in plain
    assert not one["maneuver_table"][:, :GO2NN_MANEUVER_ACC_NUM].any() and one["overall"]["switches"] == 0
    env.close()


def test_maneuvers_of_the_pretrained_student(hip):
    """the committed pretrained CTS student on go2_cts, the default evaluation under the default maneuvers: 1024 robots over every terrain kind x 7 maneuvers, one switch
    each after 5 of the 10 s, a 3 s window.  Bookkeeping only — nobody has measured settle times or fall shares: the table is what the run is there to show"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import DEFAULT_MANEUVERS, MANEUVER_KEYS, PolicyEvaluator, format_table
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    m, _ = pretrained_policy()
    m = m.to(DEV)
    env_cfg, train_cfg = task_registry.get_cfgs("go2_cts")
    ev = PolicyEvaluator(env_cfg, dict(class_to_dict(train_cfg.evaluation), maneuvers=DEFAULT_MANEUVERS), task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    res = ev.evaluate(m)
    print(format_table(res))
    for t, per in res["groups"].items():
        for n, d in per.items():
            print("%-16s %-20s %s" % (t, n, " ".join("%s %.4g" % (k, d[k]) for k in MANEUVER_KEYS + ("falls",))))
    assert res["scenarios"] == [x[0] for x in DEFAULT_MANEUVERS] and ev.maneuver_window == 150 and ev.maneuver_hold == 15
    assert res["switch_steps"] == {x[0]: [250] for x in DEFAULT_MANEUVERS}
    robots = 0
    for t, per in res["groups"].items():
        for n, d in per.items():
            assert d["n_envs"] > 0 and d["switches"] == d["n_envs"] * 1, (t, n, d)          # robots x switches per maneuver
            assert d["settled"] + d["switch_falls"] <= 1.0, (t, n, d)                        # settled + switch_falls <= switches
            assert all(math.isfinite(d[k]) for k in MANEUVER_KEYS if k != "settle_time_s") and (math.isfinite(d["settle_time_s"]) or d["settled"] == 0), (t, n, d)
            robots += d["n_envs"]
    assert robots == 1024 == res["overall"]["switches"] and np.isfinite(res["maneuver_table"]).all() and np.isfinite(res["table"]).all()
    ev.close()
