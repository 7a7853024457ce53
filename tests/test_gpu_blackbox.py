"""The black box on a real MI355X: the device build of go2nn_blackbox_* against the host build on the same scripted resets (every frame is a copy: bit-identical, ring and
state block), real falls on the HIP simulator against the existing recorder's full trace, and the black box inside a replayed HIP graph against the eager run.
Run with -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip, load_nn_emu  # noqa: E402
import test_blackbox_host as bh  # noqa: E402
from test_gpu_robust import DeviceMemory  # noqa: E402
from test_robust_host import HostMemory  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils import get_args  # noqa: E402

DEV = "cuda:0"
LIMP_EVAL = dict(enabled=True, interval=1, num_envs=64, seconds=2.0, warmup_s=0.2, terrain_level=3, seed=77, scenarios=None, perturbations=bh.LIMP, push_first_s=0.5,
                 push_period_s=1.0, push_window_s=0.4, blackbox_seconds=0.3)


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.fixture(scope="module")
def nn(hip):
    from go2_rl_gym_amd._nn import load_nn
    return load_nn()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("N", [1, 3, 65, 300])
def test_kernel_equals_the_host_build(nn, N, T, layout):
    """N = 1: 112 frame lanes, one partial block;  3: 336 lanes, the second block partial and robot boundaries inside a wave;  65: one robot more than a wave of state
    lanes;  300: several blocks in both launches.  Both builds are held to the numpy model after every call (at the end for N = 300), bit for bit, so they are each other's"""
    emu = load_nn_emu()
    offsets = range(0, bh.PATTERNS, N) if N < bh.PATTERNS else [0]
    seen = set()
    for o in offsets:
        dev_f, dev_s, model = bh.run_script(nn, DeviceMemory(), N, T, layout, offset=o, check_every=N < 300)
        host_f, host_s, _ = bh.run_script(emu, HostMemory(), N, T, layout, offset=o, check_every=N < 300)
        assert dev_f.tobytes() == host_f.tobytes() and dev_s.tobytes() == host_s.tobytes()
        seen |= model.seen | ({"never_falls"} if (model.frozen == 0).any() else set())
    assert seen >= set(bh.CASES), set(bh.CASES) - seen
    if N == 300:
        assert model.frozen[16:].sum() > 50 and (model.frozen[16:] == 0).sum() > 5 and (model.written > T).any()


def test_frozen_stays_frozen_on_the_device(nn):
    frames, state, model = bh.run_script(nn, DeviceMemory(), 70, 5, 1, poison=True)
    assert model.frozen.sum() >= 20 and not (frames == -7777.0).any()


def test_real_falls_on_the_real_simulator(hip):
    """go2_flat, 64 robots, nominal / limp (motor strength 0.05) under a zero-weight actor, 0.2 s + 2 s, eagerly, every robot recorded: per fallen robot the black box's
    ring is the full trace's frames before its first fall, byte for byte; limp robots fall, nominal ones do not"""
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    cb, log = bh.reset_log()
    ev = PolicyEvaluator(env_cfg, dict(LIMP_EVAL, record=64, blackbox=64), task_class=task_registry.get_task_class("go2_flat"), device=DEV, step_callback=cb)
    res = ev.evaluate(bh.zero_actor().to(DEV), use_graph=False)
    assert ev.fall_recorder.T == 15 and ev.warmup_steps == 10 and ev.steps == 100 and res["mode"] == "eager"
    bh.check_falls_against_trace(ev, res, log, "HIP simulator, limp 0.05")
    assert res["falls"]["fell_total"] == round((1.0 - res["overall"]["survival"]) * 64)
    ev.close()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_blackbox_inside_the_replayed_graph(hip, monkeypatch, task):
    """the captured chunk's record call reads the step counter, every ring's cursor and every freeze flag from device memory, so the replayed run's falls are the eager
    run's byte for byte, with falls landing in the middle of chunks; the scores are those of the run without the black box.  The evaluator itself never picks a chunk that
    straddles the warm-up boundary (its own accumulators are cleared there, between two replays); the black box has no such need, which the last run shows: a forced chunk
    of 11 steps divides neither the 10 warm-up steps nor the steps of the falls, and only the falls are compared"""
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    args = get_args(["--task", task, "--num_envs", "64", "--headless"])
    env, _ = task_registry.make_env(task, args)
    runner, _ = task_registry.make_alg_runner(env, task, args, log_root=None)
    ac = runner.alg.actor_critic
    with torch.no_grad():
        for p in ac.actor.parameters():          # action 0: the robot holds its default pose
            p.zero_()
    make = lambda **kw: PolicyEvaluator(env.cfg, dict(LIMP_EVAL, **kw), task_class=type(env), sim_params=env.sim_params, device=env.sim_device)          # noqa: E731
    off = make()
    base = off.evaluate(ac, use_graph=True)
    off.close()
    ev = make(blackbox=64)
    eager = ev.evaluate(ac, use_graph=False)
    replay = ev.evaluate(ac, use_graph=True)
    assert (base["mode"], eager["mode"], replay["mode"]) == ("graph", "eager", "graph") and ev.chunk == 10 and ev.warmup_steps == 10
    assert eager["table"].tobytes() == replay["table"].tobytes() == base["table"].tobytes() and eager["robust_table"].tobytes() == replay["robust_table"].tobytes() == base["robust_table"].tobytes()
    falls = eager["falls"]
    bh.same_tree(replay["falls"], falls)
    steps = falls["fall_step"]
    assert falls["fell_total"] >= 1 and (falls["pert_of_robot"] == 1).all() and (steps % ev.chunk != 0).any() and np.isfinite(falls["frames"][:, -1]).all()
    ev.chunk = 11
    assert (ev.warmup_steps + ev.steps) % 11 == 0 and ev.warmup_steps % 11 != 0 and (steps % 11 != 0).any()
    forced = ev.evaluate(ac, use_graph=True)
    assert forced["mode"] == "graph"
    bh.same_tree(forced["falls"], falls)
    print("%s: %d robots fell at counted steps %s; replayed in chunks of 10 and of 11" % (task, falls["fell_total"], sorted(set(steps.tolist()))))
    ev.close(); env.close()
