"""Empirical observation normalisation (`runner.empirical_normalization`, --normalize_obs) on the CPU: go2nn_obs_norm_apply / _update (host build) against numpy bit for
bit and against a float64 restatement within a derived bound, PPO on the host libraries, the switch-off path, the CLI and the refusals, checkpoints and export, and the
evaluator on the host build.  The cases shared with the device tests live in obs_norm_cases.py."""
import copy
import os

import numpy as np
import pytest
import torch

import obs_norm_cases as K
from helpers import load_nn_emu, load_oracle
from go2_rl_gym_amd.envs import task_registry
from go2_rl_gym_amd.rsl_rl.modules.normalizer import EmpiricalNormalization, attach_normalizers
from go2_rl_gym_amd.utils import get_args
from go2_rl_gym_amd.utils.helpers import class_to_dict, update_cfg_from_args

FWD = dict(atol=2e-6, rtol=2e-6)          # the forward tolerance of tests/test_policy_kernel.py
ENTRY_POINTS = ("go2nn_obs_norm_apply", "go2nn_obs_norm_update", "go2nn_obs_norm_partial_rows")


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


# ---- 1. y bit for bit against numpy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_partials", [True, False])
@pytest.mark.parametrize("clip", [0.0, 10.0])
@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("N", K.NS)
def test_y_is_numpy_bit_for_bit(emu, N, in_place, clip, with_partials):
    """one launch of four jobs (D = 1, 45, 263, one more than the column tile); -0.0, a denormal, a constant column, outliers the clamp acts on; sentinels untouched"""
    K.check_apply_case(K.apply_case(emu, "cpu", N, in_place, clip, with_partials), N, in_place, clip, with_partials)


def test_torch_module_states_the_same_y(emu):
    rng = np.random.default_rng(3)
    x, mean32, inv32 = K.make_stream(rng, 65, 45)
    n = EmpiricalNormalization(45, clip=10.0)
    n.mean32.copy_(torch.from_numpy(mean32)); n.inv32.copy_(torch.from_numpy(inv32))
    assert np.array_equal(K.bits(n(torch.from_numpy(x)).numpy()), K.bits(K.np_normalise(x, mean32, inv32, 10.0)))
    n.clip = 0.0
    assert np.array_equal(K.bits(n(torch.from_numpy(x)).numpy()), K.bits(K.np_normalise(x, mean32, inv32, 0.0)))


# ---- 2. the moments against a float64 restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [45, 263])
def test_moments_equal_the_pooled_two_pass_statistics(emu, D):
    """one iteration, then three with 1, 3 and 24 steps of 65 rows and a shifted distribution each: the bound is obs_norm_cases.moment_bounds; two runs, the same bits"""
    a = K.check_moments(emu, "cpu", D)
    assert K.check_moments(emu, "cpu", D) == a


def test_torch_merge_states_the_same_update(emu):
    D = 45
    rng = np.random.default_rng(5)
    its = K.shifted_batches(rng, D)
    st, n = K.Stream(emu, "cpu", D), EmpiricalNormalization(D)
    seen, frozen = [], []
    for b in its:
        frozen.append(n.mean32.numpy().copy())
        st.iteration(b.copy())
        n.merge(torch.from_numpy(b.reshape(-1, D)))
        seen.append(b.reshape(-1, D))
        _, mean, var, mean32, inv32 = st.read()
        b_mean, b_var = K.moment_bounds(seen, frozen)
        assert float(n.count) == st.read()[0]
        d_mean, d_var = np.abs(n.mean.numpy() - mean), np.abs(n.var.numpy() - var)
        print("[obs norm] kernel vs torch merge after %d samples: max |mean difference| / bound %.3e, max |var difference| / bound %.3e"
              % (int(float(n.count)), (d_mean / b_mean).max(), (d_var / np.maximum(b_var, 1e-300)).max()))
        assert (d_mean <= b_mean).all() and (d_var <= b_var).all()          # the two formulations against each other, within the bound of test 2
        # (the fp32 vectors are roundings of values that agree to 1e-15: equal unless a rounding boundary lies between them)
        np.testing.assert_allclose(n.mean32.numpy(), mean32, rtol=2e-7, atol=1e-38)
        np.testing.assert_allclose(n.inv32.numpy(), inv32, rtol=2e-7)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(emu):
    K.check_refusals(emu, "cpu")


# ---- 4. the algorithm, without an env --------------------------------------------------------------------------------------------------------------------------
T4, N4 = 3, 8


def _ppo(emu, kernel=True, until=None, seed=0, attach=True, **kw):
    from go2_rl_gym_amd.rsl_rl.algorithms import PPO
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(seed)
    ac = ActorCritic(45, 263, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", init_noise_std=0.8)
    if attach:
        attach_normalizers(ac, 45, 263, until=until)
    args = dict(num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, max_grad_norm=1.0,
                use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01, device="cpu", lib=load_oracle(), fused_rollout=kernel)
    args.update(kw)
    alg = PPO(ac, **args)
    if kernel:
        alg.nn_lib = emu
    alg.init_storage(N4, T4, [45], [263], [12])
    return alg


def _preload(alg, seed=1):
    rng = np.random.default_rng(seed)
    for n in (alg.actor_critic.obs_normalizer, alg.actor_critic.critic_obs_normalizer):
        D = n.num_features
        n.set_state(100.0, rng.normal(0, 1, D), np.exp(rng.normal(0, 1, D)))
    return {k: (n.state.numpy().copy(), n.mean32.numpy().copy(), n.inv32.numpy().copy()) for k, n in (("a", alg.actor_critic.obs_normalizer), ("c", alg.actor_critic.critic_obs_normalizer))}


def _rollout(alg, seed=2):
    """T4 steps of random observations through act / process_env_step, then compute_returns.  -> the raw inputs (obs [T, N, 45], critic obs [T, N, 263], last critic obs)"""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(T4, N4, 45, generator=g) * 2.0 + 0.5
    cobs = torch.randn(T4, N4, 263, generator=g) * 3.0 - 1.0
    last = torch.randn(N4, 263, generator=g)
    torch.manual_seed(seed)
    with torch.inference_mode():
        for s in range(T4):
            alg.act(obs[s].clone(), cobs[s].clone())
            alg.process_env_step(torch.zeros(N4), torch.zeros(N4, dtype=torch.bool), {})
        alg.compute_returns(last.clone())
    return obs, cobs, last


def test_ppo_normalises_the_storage_rows_and_merges_after_the_update(emu):
    res = {}
    for kernel in (True, False):
        alg = _ppo(emu, kernel=kernel)
        assert alg.fused_rollout is kernel
        pre = _preload(alg)
        obs, cobs, last = _rollout(alg)
        st, ac = alg.storage, alg.actor_critic
        # the storage holds normalise(inputs), bit for bit; the env-side tensors handed in are untouched (clones above: nothing to check there)
        for x, rows, key in ((obs, st.observations, "a"), (cobs, st.privileged_observations, "c")):
            want = K.np_normalise(x.numpy(), pre[key][1], pre[key][2], 10.0)
            assert np.array_equal(K.bits(rows.numpy()), K.bits(want)), (kernel, key)
        # the stored mu / log-probability are the actor module's on the stored rows: the first mini-batch's ratio is 1
        with torch.no_grad():
            mu = ac.actor(st.observations.flatten(0, 1))
            lp = torch.distributions.Normal(mu, ac.std.expand_as(mu)).log_prob(st.actions.flatten(0, 1)).sum(-1)
            v_last = ac.critic(ac.critic_obs_normalizer(last))
        np.testing.assert_allclose(st.mu.flatten(0, 1).numpy(), mu.numpy(), **FWD)
        np.testing.assert_allclose(st.actions_log_prob.flatten().numpy(), lp.numpy(), atol=2e-5)
        assert float(torch.exp(lp - st.actions_log_prob.flatten()).sub(1).abs().max()) < 1e-4
        # the bootstrap value read the normalised last observation: returns[T - 1] = r + gamma * V(normalise(last)) with r = 0
        np.testing.assert_allclose(st.returns[-1].numpy(), alg.gamma * v_last.numpy(), atol=5e-6, rtol=5e-6)
        rows = {"a": st.observations.clone(), "c": st.privileged_observations.clone()}
        # frozen inside the iteration: nothing has moved yet
        for key, n in (("a", ac.obs_normalizer), ("c", ac.critic_obs_normalizer)):
            assert n.state.numpy().tobytes() == pre[key][0].tobytes() and n.mean32.numpy().tobytes() == pre[key][1].tobytes()
        alg.update()
        out = {}
        for key, n, x in (("a", ac.obs_normalizer, obs), ("c", ac.critic_obs_normalizer, cobs)):
            D = n.num_features
            tot, mean, var, e_mean, e_var = K.pooled(pre[key], x.reshape(-1, D).numpy(), D)
            assert float(n.count) == tot == 100.0 + T4 * N4 and n.host_count() == tot
            assert (np.abs(n.mean.numpy() - mean) <= e_mean).all() and (np.abs(n.var.numpy() - var) <= e_var).all(), (kernel, key)
            assert np.array_equal(K.bits(n.mean32.numpy()), K.bits(n.mean.numpy().astype(np.float32)))
            assert np.array_equal(K.bits(n.inv32.numpy()), K.bits((1.0 / (np.sqrt(n.var.numpy()) + 1e-2)).astype(np.float32)))
            out[key] = (n.mean.numpy().copy(), n.var.numpy().copy(), e_mean, e_var)
        assert all(torch.isfinite(p).all() for p in ac.parameters())
        res[kernel] = (rows, out)
    # the kernel formulation and the torch-module formulation: the same rows bit for bit, the same state within the bound
    for key in ("a", "c"):
        assert torch.equal(res[True][0][key], res[False][0][key])
        (m1, v1, e_mean, e_var), (m2, v2, _, _) = res[True][1][key], res[False][1][key]
        print("[obs norm] PPO kernel vs torch formulation (%s): max |mean difference| / bound %.3e, max |var difference| / bound %.3e"
              % (key, (np.abs(m1 - m2) / e_mean).max(), (np.abs(v1 - v2) / np.maximum(e_var, 1e-300)).max()))
        assert (np.abs(m1 - m2) <= e_mean).all() and (np.abs(v1 - v2) <= e_var).all()          # within the bound of test 2


def test_until_stops_the_merging_at_the_right_iteration(emu):
    for kernel in (True, False):
        alg = _ppo(emu, kernel=kernel, until=2 * T4 * N4)
        counts, frozen = [], None
        for it in range(4):
            _rollout(alg, seed=10 + it)
            alg.update()
            counts.append(float(alg.actor_critic.obs_normalizer.count))
            if it == 1:
                frozen = alg.actor_critic.critic_obs_normalizer.state.numpy().copy()
        assert counts == [T4 * N4, 2 * T4 * N4, 2 * T4 * N4, 2 * T4 * N4], (kernel, counts)
        assert alg.actor_critic.critic_obs_normalizer.state.numpy().tobytes() == frozen.tobytes()


def test_algorithm_refusals(emu, monkeypatch):
    from go2_rl_gym_amd.envs.go2.go2_config import GO2Cfg
    from go2_rl_gym_amd.rsl_rl.algorithms import PPO, ppo
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic_recurrent import ActorCriticRecurrent
    from go2_rl_gym_amd.utils.symmetry import mirror_tables
    tables = mirror_tables(GO2Cfg())
    with pytest.raises(NotImplementedError, match="symmetry"):
        _ppo(emu, symmetry=tables)
    with pytest.raises(NotImplementedError, match="symmetry"):
        _ppo(emu, symmetry=tables, mirror_loss_coef=0.5)
    _ppo(emu, symmetry=tables, attach=False)
    ac = ActorCriticRecurrent(45, 263, 12, actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_hidden_size=16)
    attach_normalizers(ac, 45, 263)
    with pytest.raises(NotImplementedError, match="recurrent"):
        PPO(ac, device="cpu", lib=load_oracle())
    monkeypatch.setattr(ppo, "_world", lambda: 2)          # a forced multi-rank group
    with pytest.raises(NotImplementedError, match="one rank"):
        _ppo(emu)


# ---- 5. / 6. the runner: switch off, CLI, refusals, sensors ----------------------------------------------------------------------------------------------------
def _args(task="go2_flat", *flags, n=8, seed=5):
    return get_args(["--task", task, "--num_envs", str(n), "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", str(seed), *flags])


def _runner(emu, task="go2_flat", flags=(), log_root=None, env_cfg=None, train_cfg=None, drop_keys=False, nn=None, n=8):
    args = _args(task, *flags, n=n)
    env, _ = task_registry.make_env(task, args, env_cfg=env_cfg, lib=load_oracle(), **({"nn": nn} if nn is not None else {}))
    if drop_keys:          # a train config from before this switch existed
        from go2_rl_gym_amd.rsl_rl.runners import OnPolicyRunner
        _, cfg = task_registry.get_cfgs(task)
        d = class_to_dict(update_cfg_from_args(None, cfg, args)[1])
        for k in [k for k in d["runner"] if k.startswith("empirical_normalization")]:
            del d["runner"][k]
        runner = OnPolicyRunner(env, d, None, device="cpu")
    else:
        runner, _ = task_registry.make_alg_runner(env, None if train_cfg is not None else task, args, train_cfg=train_cfg, log_root=log_root)
    runner.alg.fused_rollout = True
    runner.alg.nn_lib = emu
    return env, runner


def _counting(monkeypatch, lib):
    calls = {k: 0 for k in ENTRY_POINTS}
    for k in ENTRY_POINTS:
        fn = getattr(lib, k)

        def wrapped(*a, _fn=fn, _k=k):
            calls[_k] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, k, wrapped)
    return calls


def _weights(runner):
    return torch.cat([p.detach().reshape(-1) for p in runner.alg.actor_critic.parameters()]).numpy().tobytes()


def test_switch_off_changes_nothing(emu, monkeypatch):
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    calls = _counting(monkeypatch, emu)
    out = []
    for drop in (False, True):
        env, runner = _runner(emu, drop_keys=drop)
        assert runner.cfg.get("empirical_normalization", False) is False
        ac = runner.alg.actor_critic
        today = set(ActorCritic(45, 263, 12, **runner.policy_cfg).state_dict())
        assert set(ac.state_dict()) == today and not any("normalizer" in k for k in today)
        assert runner.alg._obs_norm() is None and runner.alg._on_state is None
        torch.manual_seed(9)
        runner.learn(1, init_at_random_ep_len=True)
        out.append(_weights(runner))
        env.close()
    assert out[0] == out[1]
    assert calls == {k: 0 for k in ENTRY_POINTS}


def test_flag_reaches_the_runner_and_two_iterations_train(emu):
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    r = train_cfg.runner
    assert (r.empirical_normalization, r.empirical_normalization_eps, r.empirical_normalization_clip, r.empirical_normalization_until) == (False, 1e-2, 10.0, None)
    for flag in ((), ("--normalize_obs",)):
        _, cfg = update_cfg_from_args(None, copy.deepcopy(train_cfg), _args("go2_flat", *flag))
        assert cfg.runner.empirical_normalization is bool(flag)
    env, runner = _runner(emu, flags=("--normalize_obs",))
    ac = runner.alg.actor_critic
    assert runner.cfg["empirical_normalization"] is True
    assert isinstance(ac.obs_normalizer, EmpiricalNormalization) and ac.obs_normalizer.num_features == 45 and ac.critic_obs_normalizer.num_features == 263
    assert (ac.obs_normalizer.eps, ac.obs_normalizer.clip, ac.obs_normalizer.until) == (1e-2, 10.0, None)
    assert not any("normalizer" in n for n, _ in ac.named_parameters())          # buffers: the optimizer never sees them
    torch.manual_seed(9)
    runner.learn(2, init_at_random_ep_len=True)
    assert all(torch.isfinite(p).all() for p in ac.parameters())
    for n in (ac.obs_normalizer, ac.critic_obs_normalizer):
        assert float(n.count) == 2 * 8 * 24 and torch.isfinite(n.state).all() and torch.isfinite(n.inv32).all() and float(n.var.min()) >= 0.0
    assert runner.alg._on_state["lib"] is emu
    # the env keeps the simulator's raw frame: the storage rows are not the env's buffers
    raw = env.get_privileged_observations()
    assert raw.data_ptr() == env.privileged_obs_buf.data_ptr() and runner.alg.storage.privileged_observations.abs().max() <= 10.0
    assert not torch.equal(raw, runner.alg.storage.privileged_observations[-1])
    env.close()


@pytest.mark.parametrize("task,flags,match", [("go2_flat_cts", ("--normalize_obs",), "CTS"), ("go2_flat_rnn", ("--normalize_obs",), "recurrent"),
                                              ("go2_flat", ("--normalize_obs", "--symmetry"), "symmetry")])
def test_runner_refusals(emu, task, flags, match):
    args = _args(task, *flags)
    env, _ = task_registry.make_env(task, args, lib=load_oracle())
    with pytest.raises(NotImplementedError, match=match):
        task_registry.make_alg_runner(env, task, args, log_root=None)
    env.close()


def test_a_forced_multi_rank_group_is_refused(emu, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setenv("GO2_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29533")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        args = _args("go2_flat", "--normalize_obs")
        env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
        with pytest.raises(NotImplementedError, match="one rank"):
            task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
        env.close()
    finally:
        dist.destroy_process_group()


def test_randomised_sensors_train_with_the_switch(emu):
    """domain_rand.randomize_sensors + the switch: one iteration, and the stored rows are the normalised DELIVERED frames (what go2nn_sensor_rand_apply wrote)"""
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    env_cfg.domain_rand.randomize_sensors = True
    env, runner = _runner(emu, flags=("--normalize_obs",), env_cfg=env_cfg, nn=emu)
    alg = runner.alg
    for n in (alg.actor_critic.obs_normalizer, alg.actor_critic.critic_obs_normalizer):
        n.set_state(50.0, 0.3, 0.5)
    seen, inner = [], alg._obs_norm_rows

    def spy(on, s):
        seen.append((alg.storage.observations[s].clone(), env._sensors["delivered"].clone() if s == 0 else None))
        return inner(on, s)
    alg._obs_norm_rows = spy
    n = alg.actor_critic.obs_normalizer
    m32, i32 = n.mean32.numpy().copy(), n.inv32.numpy().copy()
    torch.manual_seed(3)
    runner.learn(1, init_at_random_ep_len=True)
    assert len(seen) == 24 and torch.equal(seen[0][0], seen[0][1])          # step 0: the delivered buffer's frame
    raw = torch.stack([r for r, _ in seen]).numpy()
    sim = raw[1:] != 0
    assert sim.any()
    # (storage.clear() keeps the rows) every stored row is normalise(the frame the sensor kernel delivered there)
    assert np.array_equal(K.bits(alg.storage.observations.numpy()), K.bits(K.np_normalise(raw, m32, i32, 10.0)))
    assert float(n.count) == 50.0 + 8 * 24 and all(torch.isfinite(p).all() for p in alg.actor_critic.parameters())
    env.close()


# ---- 7. checkpoints and export ---------------------------------------------------------------------------------------------------------------------------------
def _trained(emu, tmp_path, iters=1):
    env, runner = _runner(emu, flags=("--normalize_obs",))
    torch.manual_seed(9)
    runner.learn(iters, init_at_random_ep_len=True)
    path = str(tmp_path / "model.pt")
    runner.save(path)
    return env, runner, path


def test_checkpoint_round_trip_and_the_three_loading_cases(emu, tmp_path, capsys):
    env, runner, path = _trained(emu, tmp_path)
    sd = {k: v.clone() for k, v in runner.alg.actor_critic.state_dict().items()}
    assert {"obs_normalizer.state", "obs_normalizer.mean32", "obs_normalizer.inv32", "critic_obs_normalizer.state"} <= set(sd)
    assert float(sd["obs_normalizer.state"][0]) == 8 * 24
    # switch on -> on: exact
    env2, r2 = _runner(emu, flags=("--normalize_obs",))
    r2.load(path)
    sd2 = r2.alg.actor_critic.state_dict()
    assert set(sd2) == set(sd) and all(torch.equal(sd[k], sd2[k]) and sd[k].dtype == sd2[k].dtype for k in sd)
    assert r2.alg.actor_critic.obs_normalizer.host_count() == 8 * 24
    # keys in the checkpoint, switch off: the children are attached before loading, act_inference normalises, and training resumes on them
    env3, r3 = _runner(emu)
    assert not hasattr(r3.alg.actor_critic, "obs_normalizer")
    r3.load(path)
    ac3 = r3.alg.actor_critic
    sd3 = ac3.state_dict()
    assert set(sd3) == set(sd) and all(torch.equal(sd[k], sd3[k]) for k in sd)
    obs = torch.randn(16, 45) * 2
    with torch.no_grad():
        want = ac3.actor(torch.from_numpy(K.np_normalise(obs.numpy(), sd["obs_normalizer.mean32"].numpy(), sd["obs_normalizer.inv32"].numpy(), 10.0)))
        got = r3.get_inference_policy()(obs)
        assert torch.equal(got, want) and not torch.allclose(got, ac3.actor(obs), atol=1e-3)
    r3.learn(1)
    assert float(ac3.obs_normalizer.count) == 2 * 8 * 24
    # no keys in the checkpoint, switch on: from the initial state, one printed line
    env4, r4 = _runner(emu)
    plain = str(tmp_path / "plain.pt")
    r4.save(plain)
    capsys.readouterr()
    r2.load(plain)
    assert capsys.readouterr().out.count("carries no observation statistics") == 1
    n = r2.alg.actor_critic.obs_normalizer
    assert float(n.count) == 0 and float(n.mean.abs().max()) == 0 and torch.equal(n.inv32, torch.full((45,), float(1.0 / 1.01)))
    assert all(torch.equal(a, b) for a, b in zip(r2.alg.actor_critic.actor.parameters(), r4.alg.actor_critic.actor.parameters()))
    # neither: as ever
    r4.load(plain)
    assert not hasattr(r4.alg.actor_critic, "obs_normalizer")
    for e in (env, env2, env3, env4):
        e.close()


def test_a_loaded_eps_and_clip_win_over_the_config_and_say_so(emu, tmp_path, capsys):
    """eps and clip travel in the checkpoint: loaded into a run configured otherwise they replace the config's values with one printed line, and the job arrays (which hold
    the clip by value) are rebuilt, a run that had already stepped included"""
    env, runner, path = _trained(emu, tmp_path)
    _, cfg = task_registry.get_cfgs("go2_flat")
    cfg = copy.deepcopy(cfg)
    cfg.runner.empirical_normalization_clip, cfg.runner.empirical_normalization_eps = 5.0, 1e-3
    env2, r2 = _runner(emu, flags=("--normalize_obs",), train_cfg=cfg)
    n = r2.alg.actor_critic.obs_normalizer
    assert (n.eps, n.clip) == (1e-3, 5.0)
    r2.learn(1)
    assert r2.alg._on_state["jobs"][0][0].clip == 5.0 and float(r2.alg.storage.privileged_observations.abs().max()) <= 5.0
    capsys.readouterr()
    r2.load(path)
    out = capsys.readouterr().out
    assert out.count("are not used") == 1 and "clip = 10" in out and "clip = 5" in out
    assert (n.eps, n.clip) == (1e-2, 10.0) and r2.alg._on_state.get("storage") is None
    r2.learn(1)
    assert r2.alg._on_state["jobs"][0][0].clip == 10.0
    # the same values: nothing is printed
    env3, r3 = _runner(emu, flags=("--normalize_obs",))
    capsys.readouterr()
    r3.load(path)
    assert "are not used" not in capsys.readouterr().out
    for e in (env, env2, env3):
        e.close()


def test_export_carries_the_normaliser(emu, tmp_path):
    from go2_rl_gym_amd.utils.exporter import export_policy_as_jit, export_policy_as_onnx, export_policy_as_pkl
    alg = _ppo(emu)
    _preload(alg)
    ac = alg.actor_critic
    obs = torch.randn(16, 45) * 3
    with torch.no_grad():
        want = ac.act_inference(obs)
        assert not torch.allclose(want, ac.actor(obs), atol=1e-3)
    mod = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "n"), normalizer=ac.obs_normalizer))
    with torch.no_grad():
        got = torch.cat([mod(obs[i:i + 1]) for i in range(16)])
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-6)          # the tolerance of tests/test_export.py
    assert "obs_normalizer.mean32" in torch.load(export_policy_as_pkl(ac, str(tmp_path / "n")))
    try:
        import onnx  # noqa: F401
        import onnxruntime
    except ImportError:
        onnxruntime = None
    if onnxruntime is not None:
        sess = onnxruntime.InferenceSession(export_policy_as_onnx(ac, str(tmp_path / "n"), normalizer=ac.obs_normalizer))
        got = np.concatenate([sess.run(None, {"obs": obs[i:i + 1].numpy()})[0] for i in range(16)])
        np.testing.assert_allclose(got, want.numpy(), atol=1e-6)
    # without the child the exported module is what it was: no normaliser in it, the actor's answer
    plain = _ppo(emu, attach=False).actor_critic
    mod = torch.jit.load(export_policy_as_jit(plain, str(tmp_path / "p")))
    assert mod.normalizer.original_name == "Identity"
    with torch.no_grad():
        assert torch.equal(mod(obs[:1]), plain.actor(obs[:1])) and torch.equal(plain.act_inference(obs), plain.actor(obs))


def test_play_exports_the_normaliser(emu, tmp_path, monkeypatch):
    """scripts/play.py hands model.obs_normalizer to the exporters when the child is there"""
    from go2_rl_gym_amd.scripts import play as P
    seen = []
    monkeypatch.setattr(P, "export_policy_as_jit", lambda model, path, normalizer=None: seen.append(("jit", normalizer)) or "jit")
    monkeypatch.setattr(P, "export_policy_as_onnx", lambda model, path, normalizer=None: seen.append(("onnx", normalizer)) or "onnx")
    monkeypatch.setattr(P, "export_policy_as_pkl", lambda model, path: "pkl")
    os.makedirs(str(tmp_path / "logs" / "run"))
    env, runner, path = _trained(emu, tmp_path / "logs" / "run")
    env.close()
    os.rename(path, str(tmp_path / "logs" / "run" / "model_1.pt"))
    real = task_registry.make_env
    monkeypatch.setattr(task_registry, "make_env", lambda name, args, env_cfg=None, **kw: real(name, args, env_cfg=env_cfg, lib=load_oracle()))
    env, exported = P.play(_args("go2_flat"), steps=2, log_root=str(tmp_path / "logs"), export_policy=True)
    assert [k for k, _ in seen] == ["jit", "onnx"] and all(isinstance(n, EmpiricalNormalization) and float(n.count) == 8 * 24 for _, n in seen)
    env.close()


# ---- 8. the evaluator on the host build -------------------------------------------------------------------------------------------------------------------------
EVAL = dict(enabled=True, interval=2, num_envs=12, seconds=0.4, warmup_s=0.1, terrain_level=3, seed=77, scenarios=[["forward_1.0", 1.0, 0.0, 0.0], ["turn_1.0", 0.0, 0.0, 1.0]])


def _evaluator(emu, **over):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    return PolicyEvaluator(env_cfg, dict(EVAL, **over), task_class=task_registry.get_task_class("go2_flat"), device="cpu", lib=load_oracle(), nn_lib=emu)


@pytest.mark.parametrize("mode", ["plain", "asymmetry", "sensors"])
def test_evaluator_normalises_in_front_of_the_forward_kernel(emu, monkeypatch, mode):
    from go2_rl_gym_amd.utils import evaluator as E
    over = {"plain": {}, "asymmetry": {"asymmetry": True}, "sensors": {"sensors": [[n, dict(f)] for n, f in E.DEFAULT_SENSORS[:2]]}}[mode]
    ev = _evaluator(emu, **over)
    ac = _ppo(emu, attach=False).actor_critic
    calls = _counting(monkeypatch, emu)
    before = ev.evaluate(ac)["table"].tobytes()
    assert calls == {k: 0 for k in ENTRY_POINTS}          # no child: nothing is launched
    attach_normalizers(ac, 45, 263)
    rng = np.random.default_rng(2)
    ac.obs_normalizer.set_state(500.0, rng.normal(0, 0.5, 45), np.exp(rng.normal(-1, 1, 45)))
    seen = []
    for name in ("act", "act_mirrored"):
        inner = getattr(E._MlpPolicy, name)

        def spy(self, obs, *a, _inner=inner, _name=name):
            out = _inner(self, obs, *a)
            seen.append((_name, obs.clone(), out.clone(), obs.data_ptr()))
            return out
        monkeypatch.setattr(E._MlpPolicy, name, spy)
    res = ev.evaluate(ac)
    n_steps = ev.warmup_steps + ev.steps
    assert calls["go2nn_obs_norm_apply"] == n_steps * (2 if mode == "asymmetry" else 1) and calls["go2nn_obs_norm_update"] == 0
    assert res["table"].tobytes() != before and np.isfinite(res["table"]).all()
    with torch.no_grad():
        for name, obs, out, ptr in seen:
            np.testing.assert_allclose(out.numpy(), ac.actor(ac.obs_normalizer(obs)).numpy(), **FWD)
            if mode == "sensors":
                assert ptr == ev.delivered.data_ptr()          # the delivered frame is what is normalised
            if mode == "asymmetry" and name == "act_mirrored":
                assert ptr == ev.asym_obs[1].data_ptr()          # the mirror image of the RAW observation
    assert {n for n, *_ in seen} == ({"act", "act_mirrored"} if mode == "asymmetry" else {"act"})
    state = ac.obs_normalizer.state.clone()
    assert ev.evaluate(ac)["table"].tobytes() == res["table"].tobytes() and torch.equal(ac.obs_normalizer.state, state)          # the statistics never move
    # without the child again: byte for byte what it was
    del ac.obs_normalizer, ac.critic_obs_normalizer
    assert ev.evaluate(ac)["table"].tobytes() == before
    ev.close()
