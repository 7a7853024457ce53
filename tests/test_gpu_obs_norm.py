"""Empirical observation normalisation on the device (`runner.empirical_normalization`): go2nn_obs_norm_apply / _update against numpy bit for bit, against the host build
and against the float64 restatement (the cases of obs_norm_cases.py at the host tests' shapes), graph-mode PPO against the eager mode with the switch off and on in one
run (switch off is the yardstick), and train -> evaluate -> play end to end.  Run with -m gpu."""
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import obs_norm_cases as K  # noqa: E402
from helpers import load_hip, load_nn_emu  # noqa: E402
from test_gpu_parity import CLIP_OFF, GAP1_MED  # noqa: E402
from go2_rl_gym_amd import _nn  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1
    return lib


@pytest.fixture(scope="module")
def nn():
    return _nn.load_nn()


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", K.NS)
def test_y_on_gpu_is_numpy_and_the_host_build_bit_for_bit(nn, N):
    """per N: in place and out of place, clip 0 and 10, with and without the partial table; one launch of four jobs each"""
    emu = load_nn_emu()
    for in_place in (True, False):
        for clip in (0.0, 10.0):
            for with_partials in (True, False):
                res = K.apply_case(nn, DEV, N, in_place, clip, with_partials)
                K.check_apply_case(res, N, in_place, clip, with_partials)
                host = K.apply_case(emu, "cpu", N, in_place, clip, with_partials)
                for a, b in zip(res, host):
                    assert np.array_equal(K.bits(a["y"]), K.bits(b["y"])), (N, a["D"], in_place, clip)


@pytest.mark.parametrize("D", [45, 263])
def test_moments_on_gpu_equal_the_pooled_two_pass_statistics(nn, D):
    a = K.check_moments(nn, DEV, D, label=" gpu")
    assert K.check_moments(nn, DEV, D, label=" gpu") == a          # no atomics, a fixed order: two runs give the same bits


def test_refusals_on_gpu_write_nothing(nn):
    K.check_refusals(nn, DEV)


# ---- 2. graph mode against the eager mode ----------------------------------------------------------------------------------------------------------------------
N_ENVS, ITERS = 64, 3


def _preload(ac):
    rng = np.random.default_rng(1)
    pre = {}
    for key, n in (("a", ac.obs_normalizer), ("c", ac.critic_obs_normalizer)):
        D = n.num_features
        n.set_state(1000.0, rng.normal(0, 0.3, D), np.exp(rng.normal(-0.5, 0.7, D)))
        pre[key] = (n.state.cpu().numpy().copy(), n.mean32.cpu().numpy().copy(), n.inv32.cpu().numpy().copy())
    return pre


def _train_arm(monkeypatch, normalize, graph, iters):
    """tests/test_gpu_symmetry.py::_train_arm with the normalisation switch in the place of the symmetry flag: go2_flat at 64 envs x 24 steps, the same seed and initial
    weights, a fixed learning rate, the smooth objective (CLIP_OFF), pre-drawn exploration noise and ONE fixed permutation.  The statistics are preloaded, so iteration 1
    already runs on non-trivial ones.  -> env, runner, the weights after iteration 1, the state after iteration 1, (preloaded state, the raw rows of iteration 1)"""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic import ActorCritic
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", str(N_ENVS), "--headless", "--seed", "3"] + (["--normalize_obs"] if normalize else []))
    env, _ = task_registry.make_env("go2_flat", args)
    torch.manual_seed(3)
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    keep = (train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param, train_cfg.runner.empirical_normalization)
    train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param = "fixed", CLIP_OFF
    try:
        runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, train_cfg=train_cfg, log_root=None, use_graphs=graph)
    finally:
        train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param, train_cfg.runner.empirical_normalization = keep
    alg = runner.alg
    ac = alg.actor_critic
    assert alg.use_graphs == graph and hasattr(ac, "obs_normalizer") == normalize and alg.fused_loss and alg.fused_rollout
    pre, raw = (_preload(ac) if normalize else None), {"a": [], "c": []}
    if normalize:          # the raw rows of iteration 1 (an eager rollout in both arms), for the bound on the merged state
        inner = alg._obs_norm_rows

        def spy(on, s):
            if len(raw["a"]) < alg.storage.num_transitions_per_env and not torch.cuda.is_current_stream_capturing():
                raw["a"].append(alg.storage.observations[s].clone()); raw["c"].append(alg.storage.privileged_observations[s].clone())
            return inner(on, s)
        alg._obs_norm_rows = spy
    T, A = alg.storage.num_transitions_per_env, alg.storage.actions.shape[-1]
    gen, buf, calls = torch.Generator().manual_seed(17), torch.zeros(T, N_ENVS, A, device=alg.device), [0]

    def noise(self_, like):
        row = buf[calls[0] % T]; calls[0] += 1
        assert row.shape == like.shape
        return row
    monkeypatch.setattr(ActorCritic, "_noise", noise)
    perm = torch.randperm(N_ENVS * T, generator=torch.Generator().manual_seed(23)).to(alg.device)
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: perm)
    env.common_step_counter = 0
    first = state = None
    for it in range(iters):
        buf.copy_(torch.randn(buf.shape, generator=gen))
        runner.learn(1, init_at_random_ep_len=(it == 0))
        if it == 0:
            first = {n: p.detach().cpu().numpy().copy() for n, p in ac.named_parameters()}
            if normalize:
                state = {"a": ac.obs_normalizer.state.cpu().numpy().copy(), "c": ac.critic_obs_normalizer.state.cpu().numpy().copy()}
    torch.cuda.synchronize()
    return env, runner, first, state, (pre, {k: torch.stack(v).flatten(0, 1).cpu().numpy() for k, v in raw.items()} if normalize else None)


def test_graph_mode_matches_the_eager_mode_with_the_switch_off_and_on(hip, nn, monkeypatch):
    """After iteration 1 the per-tensor median gap between graph mode and the eager mode with the switch ON is at most 4 x the gap with the switch OFF measured in this
    same run (the code as it stands: the yardstick; the factor 4 is an allowance for the first layers' pre-activations growing when all 263 critic columns arrive at unit
    scale instead of mostly below it, not a measurement), plus the floor of tests/test_gpu_parity.py (GAP1_MED).  With the switch on the rollout and the update are
    captured, the weights stay finite over three iterations, and the state after iteration 1 agrees between the arms — and with the pooled two-pass statistics of the
    rollout's raw rows — within the derived bound of obs_norm_cases.py."""
    import torch
    gaps, graph_weights, states, raws, pres = {}, {}, {}, {}, {}
    for normalize in (False, True):
        first = {}
        for graph in (False, True):
            env, runner, first[graph], state, (pre, raw) = _train_arm(monkeypatch, normalize, graph, ITERS if (graph and normalize) else 1)
            alg = runner.alg
            if normalize:
                states[graph], raws[graph], pres[graph] = state, raw, pre
                for key, D in (("a", 45), ("c", 263)):
                    tot, mean, var, e_mean, e_var = K.pooled(pre[key], raw[key], D)
                    got_mean, got_var = state[key][1:1 + D], state[key][1 + D:] / state[key][0]
                    print("[obs norm %s, %s] state after iteration 1: max |mean err| %.3e (bound %.3e), max |var err| %.3e (bound %.3e)"
                          % ("graph" if graph else "eager", key, np.abs(got_mean - mean).max(), e_mean[np.abs(got_mean - mean).argmax()], np.abs(got_var - var).max(),
                             e_var[np.abs(got_var - var).argmax()]))
                    assert state[key][0] == tot == 1000.0 + N_ENVS * 24
                    assert (np.abs(got_mean - mean) <= e_mean).all() and (np.abs(got_var - var) <= e_var).all(), (graph, key)
            if graph and normalize:
                caps = runner.graphs_captured()
                assert caps["rollout"] and caps["update"], caps
                assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
                n = alg.actor_critic.obs_normalizer
                assert float(n.count) == 1000.0 + ITERS * N_ENVS * 24 and n.host_count() == float(n.count) and bool(torch.isfinite(n.inv32).all())
                assert float(alg.storage.privileged_observations.abs().max()) <= 10.0
            elif graph:
                assert alg._obs_norm() is None and alg._on_state is None
            env.close()
            del env, runner, alg          # (their HIP graphs, streams and events: collected here, with the device idle, not in the middle of the next arm's replay)
            torch.cuda.synchronize()
            gc.collect()
        graph_weights[normalize] = first[True]
        gaps[normalize] = {n: float(np.median(np.abs(first[True][n] - first[False][n]))) for n in first[True]}
        peak = {n: float(np.abs(first[True][n] - first[False][n]).max()) for n in first[True]}
        print("[obs norm %s] graph vs eager after iteration 1: largest per-tensor median gap %.2e (%s), largest element gap %.2e"
              % ("on" if normalize else "off", max(gaps[normalize].values()), max(gaps[normalize], key=gaps[normalize].get), max(peak.values())))
    # both arms ran the same kernels on the same rollout: the raw rows of iteration 1 are the same bits, and the merged states agree within the bound of test 2
    for key, D in (("a", 45), ("c", 263)):
        assert np.array_equal(K.bits(raws[True][key]), K.bits(raws[False][key])), "the two arms' rollouts of iteration 1 differ (%s)" % key
        _, _, _, e_mean, e_var = K.pooled(pres[True][key], raws[True][key], D)
        sg, se = states[True][key], states[False][key]
        d_mean, d_var = np.abs(sg[1:1 + D] - se[1:1 + D]), np.abs(sg[1 + D:] / sg[0] - se[1 + D:] / se[0])
        print("[obs norm] state graph vs eager after iteration 1 (%s): max |mean difference| %.3e (bound %.3e), max |var difference| %.3e (bound %.3e)"
              % (key, d_mean.max(), e_mean[d_mean.argmax()], d_var.max(), e_var[d_var.argmax()]))
        assert sg[0] == se[0] and (d_mean <= e_mean).all() and (d_var <= e_var).all(), key
    ratio = max(gaps[True][n] / (gaps[False][n] + GAP1_MED) for n in gaps[True])
    print("[obs norm] largest gap_on / (gap_off + GAP1_MED) over the tensors: %.3f (allowed: gap_on <= 4 gap_off + GAP1_MED)" % ratio)
    for n in gaps[True]:
        assert gaps[True][n] <= 4.0 * gaps[False][n] + GAP1_MED, (n, gaps[True][n], gaps[False][n])
    # the switch does something: the two settings have trained on different inputs (20 Adam steps of 1e-3 each)
    assert max(float(np.median(np.abs(graph_weights[True][n] - graph_weights[False][n]))) for n in graph_weights[True]) > 1e-4


# ---- the evaluator's captured chunk with a normaliser -------------------------------------------------------------------------------------------------------
def test_evaluator_replays_the_normalisation_launch(hip, nn):
    """ONE PolicyEvaluator under evaluation.replay, a model with non-trivial statistics: the first evaluation runs eagerly, the second captures a chunk of steps — the
    go2nn_obs_norm_apply launch and its scratch buffer inside it, of the mirrored observation too — and replays it: the same table, byte for byte."""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    from go2_rl_gym_amd.rsl_rl.modules.normalizer import attach_normalizers
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True, asymmetry=True)
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    ev = PolicyEvaluator(env_cfg, cfg, task_class=task_registry.get_task_class("go2_flat"), device=DEV)
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu").to(DEV)
    plain = ev.evaluate(ac, use_graph=False)
    attach_normalizers(ac, 45, 263)
    rng = np.random.default_rng(2)
    ac.obs_normalizer.set_state(500.0, rng.normal(0, 0.5, 45), np.exp(rng.normal(-1, 1, 45)))
    eager = ev.evaluate(ac, use_graph=False)
    replay = ev.evaluate(ac)          # (not the evaluator's first evaluation: a captured chunk, replayed)
    assert (eager["mode"], replay["mode"]) == ("eager", "graph")
    assert eager["table"].tobytes() == replay["table"].tobytes() and eager["table"].tobytes() != plain["table"].tobytes()
    assert eager["asymmetry"]["overall"] == replay["asymmetry"]["overall"] and np.isfinite(replay["asymmetry"]["overall"]["equivariance_rmse"])
    ev.close()


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------------------------------
def test_train_evaluate_play_with_the_switch(hip, nn, tmp_path):
    """train --normalize_obs (2 iterations, 64 envs) -> checkpoint -> scripts/evaluate.py plain and --asymmetry (finite, and a second run gives identical numbers) ->
    play --export, whose TorchScript module answers like the device policy's act_inference on 16 raw observations"""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.scripts.play import play
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", "64", "--headless", "--normalize_obs", "--seed", "2"])
    env, _ = task_registry.make_env("go2_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(2, init_at_random_ep_len=True)
    ac = runner.alg.actor_critic
    assert float(ac.obs_normalizer.count) == 2 * 64 * 24
    obs = torch.randn(16, 45, generator=torch.Generator().manual_seed(1)) * 2.0
    with torch.no_grad():
        want = ac.act_inference(obs.to(DEV)).cpu()
        assert not torch.allclose(want, ac.actor(obs.to(DEV)).cpu(), atol=1e-3)
    env.close()
    base = ["--task", "go2_flat", "--num_envs", "64", "--headless", "--eval_envs", "64"]          # (without --normalize_obs: the checkpoint carries what it needs)
    for extra in ([], ["--asymmetry"]):
        out = [evaluate(base + extra, log_root=str(tmp_path)) for _ in range(2)]
        o = out[0]["checkpoints"][0]
        assert all(np.isfinite(v) for v in o["overall"].values()), o["overall"]
        assert out[0]["checkpoints"][0]["overall"] == out[1]["checkpoints"][0]["overall"]
        if extra:
            a = o["asymmetry"]["overall"]
            assert np.isfinite(a["equivariance_rmse"]) and a == out[1]["checkpoints"][0]["asymmetry"]["overall"]
    env, exported = play(get_args(["--task", "go2_flat", "--num_envs", "64", "--headless"]), steps=5, log_root=str(tmp_path), export_policy=True)
    assert torch.isfinite(env.obs_buf).all() and os.path.exists(exported[0])
    jit = torch.jit.load(exported[0])
    with torch.no_grad():
        got = torch.cat([jit(obs[i:i + 1]) for i in range(16)])
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-6)
    assert "obs_normalizer.state" in torch.load(exported[1])
    env.close()
