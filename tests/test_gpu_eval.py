"""The policy evaluator on a real MI355X: the device build of the go2nn_eval_* kernels against the float64 restatements of tests/test_eval_host.py (same bounds),
graph replay against eager execution, isolation from a live training run, and what the scores say about a policy that is known to walk.  Run with -m gpu."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_eval_host as th  # noqa: E402
from go2_rl_gym_amd._nn import EVAL_FIELDS, GO2NN_EVAL_NUM  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils import get_args  # noqa: E402

DEV = "cuda:0"
SMALL = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True)


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.fixture(scope="module")
def nn(hip):
    from go2_rl_gym_amd._nn import load_nn
    return load_nn()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("N", [17, 4096])
def test_accumulate_and_reduce_on_the_device(nn, N):
    lim = torch.from_numpy(th.LIMITS.copy()).to(DEV)
    acc_d = torch.zeros(GO2NN_EVAL_NUM, N, device=DEV)

    def call(arrs, strides, vel_off, acc):
        dev = {k: torch.from_numpy(arrs[k]).to(DEV) for k in EVAL_FIELDS}
        a = th.eval_in(lambda k: dev[k].data_ptr(), strides, vel_off, lim.data_ptr())
        assert nn.go2nn_eval_accumulate(C.byref(a), C.c_void_p(acc_d.data_ptr()), N, _st()) == 0, nn.go2nn_last_error()
        torch.cuda.synchronize()
        return acc
    _, ref, mag = th.run_accumulate_case(call, N, layout=1)
    th.check_accumulate(acc_d.cpu().numpy(), ref, mag, 64, "device N=%d field-major" % N)
    G = 7
    acc, group = th.reduce_case(N, G)
    a_d, g_d = torch.from_numpy(acc).to(DEV), torch.from_numpy(group).to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((G, GO2NN_EVAL_NUM + 2), -1.0, dtype=torch.float64, device=DEV)
        assert nn.go2nn_eval_reduce(C.c_void_p(a_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, G, C.c_void_p(out.data_ptr()), _st()) == 0
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    th.check_reduce(outs[0], acc, group, G, N, "device N=%d" % N)
    assert nn.go2nn_eval_clear(C.c_void_p(acc_d.data_ptr()), N, _st()) == 0 and not acc_d.any()


def _runner(task, tmp=None, envs=256, extra=()):
    args = get_args(["--task", task, "--num_envs", str(envs), "--headless", *extra])
    env, _ = task_registry.make_env(task, args)
    runner, train_cfg = task_registry.make_alg_runner(env, task, args, log_root=tmp)
    return env, runner, args


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts", "go2_flat_rnn"])
def test_replay_equals_eager(hip, monkeypatch, task):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    env, runner, _ = _runner(task, envs=64)
    ev = PolicyEvaluator(env.cfg, SMALL, task_class=type(env), sim_params=env.sim_params, device=env.sim_device)
    ac = runner.alg.actor_critic
    eager = ev.evaluate(ac, use_graph=False)
    replay = ev.evaluate(ac)                  # the second evaluation of an evaluator captures a chunk and replays it
    again = ev.evaluate(ac, use_graph=False)
    assert (eager["mode"], replay["mode"], again["mode"]) == ("eager", "graph", "eager") and ev.chunk == 25
    print("%s: overall %s" % (task, eager["overall"]))
    assert np.isfinite(eager["table"]).all() and eager["overall"]["n_envs"] == 256 and eager["table"][:, 0].sum() == 256 * ev.steps
    assert eager["table"].tobytes() == again["table"].tobytes()
    assert eager["table"].tobytes() == replay["table"].tobytes()
    ev.close(); env.close()


def test_evaluation_during_training_leaves_the_run_untouched(hip, tmp_path):
    env, runner, _ = _runner("go2_flat", tmp=str(tmp_path))
    runner.eval_cfg = dict(SMALL)
    runner.save_interval = 1
    inner, seen = runner.update_evaluation, []

    def checked(it, last_model=False):
        before = th._snapshot(env, runner)
        res = inner(it, last_model)
        torch.cuda.synchronize()
        th.assert_same_snapshot(before, th._snapshot(env, runner))
        seen.append((it, last_model, res["mode"] if res else None))
        return res
    runner.update_evaluation = checked
    runner.learn(5, init_at_random_ep_len=True)
    assert runner.graphs_captured()["rollout"] is True
    assert [s[0] for s in seen] == [0, 1, 2, 3, 4, 4] and seen[1][2] == "graph"
    assert sorted(os.listdir(os.path.join(runner.log_dir, "eval_results"))) == ["results_%d.yaml" % i for i in range(6)]
    assert torch.isfinite(torch.cat([p.detach().reshape(-1) for p in runner.alg.actor_critic.parameters()])).all()
    env.close()


def _evaluator(task, **over):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    ev = dict(class_to_dict(train_cfg.evaluation), **over)
    return PolicyEvaluator(env_cfg, ev, task_class=task_registry.get_task_class(task), device=DEV)


def test_scores_of_the_pretrained_student(hip):
    """the committed pretrained CTS student on the plane, scenario forward_1.0: no fall and 0.8 < speed along the command < 1.1 (the bounds
    tests/test_gpu_parity.py::test_pretrained_policy_walks_on_gpu holds it to); the same network with zeroed weights tracks worse"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import format_table
    m, _ = pretrained_policy()
    m = m.to(DEV)
    ev = _evaluator("go2_flat_cts")
    res = ev.evaluate(m)
    print(format_table(res))
    fwd = res["groups"]["plane"]["forward_1.0"]
    assert fwd["falls"] == 0 and fwd["survival"] == 1.0 and 0.8 < fwd["speed_along_cmd"] < 1.1, fwd
    import copy
    z = copy.deepcopy(m)
    with torch.no_grad():
        for p in z.parameters():
            p.zero_()
    zero = ev.evaluate(z)
    assert zero["groups"]["plane"]["forward_1.0"]["lin_vel_err"] > fwd["lin_vel_err"]
    ev.close()
    rough = _evaluator("go2_cts")
    res = rough.evaluate(m)
    print(format_table(res))
    assert len(res["groups"]) > 1
    for per in res["groups"].values():
        for d in per.values():
            assert d["n_envs"] > 0 and all(np.isfinite(d[k]) for k in d), d
    rough.close()


def test_train_then_evaluate_all_checkpoints(hip, tmp_path, capsys):
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    env, runner, _ = _runner("go2_flat", tmp=str(tmp_path))
    runner.save_interval = 2
    runner.learn(4, init_at_random_ep_len=True)
    env.close()
    out = evaluate(["--task", "go2_flat", "--num_envs", "64", "--headless", "--all_checkpoints", "--metric", "lin_vel_err", "--eval_envs", "256"], log_root=str(tmp_path))
    assert [r["checkpoint"] for r in out["checkpoints"]] == ["model_0.pt", "model_2.pt", "model_4.pt"]
    assert out["best"] in ("model_0.pt", "model_2.pt", "model_4.pt") and out["best_value"] == min(r["overall"]["lin_vel_err"] for r in out["checkpoints"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert json.loads(line)["best"] == out["best"]
