"""Value normalisation (`algorithm.normalize_value`, --normalize_value) on the CPU: go2nn_value_norm_apply / _update / go2nn_value_head_fold (host build) against numpy
bit for bit and against float64 restatements within derived bounds, PPO and CTS on the host libraries (raw values in the rollout, normalised rows behind GAE, the
reward-scale invariance the feature exists for), the switch-off path, checkpoints, the refusals and the CLI.  The cases shared with the device tests live in
value_norm_cases.py."""
import copy

import numpy as np
import pytest
import torch

import value_norm_cases as K
from helpers import load_nn_emu, load_oracle
from go2_rl_gym_amd.envs import task_registry
from go2_rl_gym_amd.rsl_rl.modules.normalizer import ValueNormalization
from go2_rl_gym_amd.utils import get_args
from go2_rl_gym_amd.utils.helpers import update_cfg_from_args

ENTRY_POINTS = ("go2nn_value_norm_apply", "go2nn_value_norm_update", "go2nn_value_head_fold", "go2nn_value_norm_partial_rows")
GAP_FLOOR = 2e-6          # GAP1_MED of tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_partials", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", K.NS)
def test_values_and_returns_are_numpy_bit_for_bit(emu, n, offset, with_partials):
    """aligned tensors and views offset by one float; -0.0, a denormal, returns around 20 with spread 0.5; sentinels in front of and behind the views untouched"""
    K.check_apply_case(K.apply_case(emu, "cpu", n, offset, with_partials), with_partials)


def test_torch_module_states_the_same_normalisation():
    rng = np.random.default_rng(3)
    v, r = K.make_data(rng, 300)
    vn = ValueNormalization()
    vn.set_state(1000.0, 19.7, 0.3)
    stat = vn.stat32.numpy().copy()
    assert np.array_equal(K.bits(stat), K.bits(K.stat_of(19.7, 0.3)))
    assert np.array_equal(K.bits(vn.normalize(torch.from_numpy(r)).numpy()), K.bits(K.np_normalise(r, stat)))
    vhat = torch.from_numpy(K.np_normalise(v, stat))
    raw = vn.denormalize(vhat).numpy()
    assert np.array_equal(K.bits(raw), K.bits(vhat.numpy() * stat[1] + stat[0]))
    fresh = ValueNormalization()
    assert fresh.state.tolist() == [0.0, 0.0, 0.0] and float(fresh.var) == 1.0 and np.array_equal(K.bits(fresh.stat32.numpy()), K.bits(K.stat_of(0.0, 1.0)))


def test_moments_equal_the_pooled_two_pass_statistics(emu):
    """three iterations of 1, 3 and 24 steps' worth of rows, shifted distributions; the bound is obs_norm_cases.moment_bounds; two runs, the same bits"""
    a = K.check_moments(emu, "cpu")
    assert K.check_moments(emu, "cpu") == a


def test_torch_merge_states_the_same_update(emu):
    import obs_norm_cases as O
    rng = np.random.default_rng(5)
    st, vn = K.Stream(emu, "cpu"), ValueNormalization()
    seen, frozen = [], []
    for b in K.shifted_returns(rng):
        frozen.append(vn.stat32.numpy()[:1].copy())
        st.iteration(b.copy())
        vn.merge(torch.from_numpy(b))
        seen.append(b.reshape(-1, 1))
        count, mean, var, stat32 = st.read()
        b_mean, b_var = O.moment_bounds(seen, frozen)
        d_mean, d_var = abs(float(vn.mean) - mean), abs(float(vn.var) - var)
        print("[value norm] kernel vs torch merge after %d samples: |mean difference| / bound %.3e, |var difference| / bound %.3e" % (int(count), d_mean / b_mean[0], d_var / b_var[0]))
        assert float(vn.count) == count and d_mean <= b_mean[0] and d_var <= b_var[0]
        np.testing.assert_allclose(vn.stat32.numpy(), stat32, rtol=2e-7)          # (roundings of values that agree to 1e-15)


@pytest.mark.parametrize("Kw", [1, 37, 128])
def test_folded_critic_answers_in_raw_units(emu, Kw):
    K.check_fold(emu, "cpu", Kw)


@pytest.mark.parametrize("Kw", [1, 37, 128])
def test_update_preserves_the_raw_value(emu, Kw):
    K.check_preservation(emu, "cpu", Kw)


def test_refusals_write_nothing(emu):
    K.check_refusals(emu, "cpu")


def test_round_trip_size():
    """((v^ std32 + mean32) - mean32) inv32 is not v^ bit for bit: its size in ulp of v^ over the test's data (DESIGN.md section 8 quotes these figures)"""
    rng = np.random.default_rng(0)
    for mean, var in ((19.7, 0.3), (0.5, 4.0), (120.0, 900.0)):
        stat = K.stat_of(mean, var)
        vhat = rng.normal(size=20000).astype(np.float32)
        u = K.round_trip_ulp(vhat[np.abs(vhat) > 1e-3], stat)
        print("[value norm] round trip at mean %.1f, std %.2f: median %.1f ulp, 99th percentile %.1f ulp, max %.1f ulp of v^ (|v^| > 1e-3)" % (mean, stat[1], np.median(u), np.percentile(u, 99), u.max()))
        # the raw value carries half an ulp of |mean| + |v^| std: in units of v^ that is (|mean| / std + |v^|) 2^-24, and the way back adds the product's own roundings
        raw_err = (abs(mean) / stat[1] + np.abs(vhat[np.abs(vhat) > 1e-3])) * 2.0 ** -24
        assert (u * np.spacing(np.abs(vhat[np.abs(vhat) > 1e-3])) <= 4.0 * raw_err + 1e-7).all()


# ---- 2. the algorithm, without an env ---------------------------------------------------------------------------------------------------------------------------
T4, N4 = 3, 8
PRE = (500.0, 6.0, 2.25)          # preloaded statistics: count, mean, variance


def _alg(emu, kind="ppo", kernel=True, seed=0, critic_scale=1.0, **kw):
    """the pattern of tests/test_obs_norm_host.py::_ppo, for PPO and CTS: small networks, the oracle library for GAE / the heads, the host build for the policy side"""
    from go2_rl_gym_amd.rsl_rl.algorithms import CTS, PPO
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic, ActorCriticCTS
    torch.manual_seed(seed)
    args = dict(num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, max_grad_norm=1.0,
                use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01, device="cpu", lib=load_oracle(), fused_rollout=kernel)
    args.update(kw)
    if kind == "ppo":
        net = ActorCritic(45, 263, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", init_noise_std=0.8)
        alg = PPO(net, **args)
    else:
        net = ActorCriticCTS(45, 263, 12, N4, 5, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], teacher_encoder_hidden_dims=[32], student_encoder_hidden_dims=[32], latent_dim=8)
        alg = CTS(net, N4, 5, **args)
    if critic_scale != 1.0:
        with torch.no_grad():
            net.critic[-1].weight.mul_(critic_scale); net.critic[-1].bias.mul_(critic_scale)
    if kernel:
        alg.nn_lib = emu
    alg.init_storage(N4, T4, [45], [263], [12])
    return alg


def _pair(monkeypatch, kind):
    """the CTS policy kernel is planned by modules/fused_cts.py, which wants the simulator-side library set too (on a GPU the algorithm does that itself)"""
    if kind == "cts":
        from go2_rl_gym_amd.rsl_rl.modules import fused
        monkeypatch.setattr(fused, "_LIB", load_oracle())


def _inputs(seed=2):
    g = torch.Generator().manual_seed(seed)
    return dict(obs=torch.randn(T4 + 1, N4, 45, generator=g), cobs=torch.randn(T4 + 1, N4, 263, generator=g), hist=torch.randn(T4 + 1, N4, 225, generator=g),
                rew=4.0 + torch.randn(T4, N4, generator=g), touts=torch.rand(T4, N4, generator=g) < 0.25)


def _rollout(alg, kind, x, reward_scale=1.0, seed=2, watch=None):
    """T4 steps through act / process_env_step (a quarter of the steps time out: the bootstrap reads the stored raw value), then compute_returns"""
    torch.manual_seed(seed)
    with torch.inference_mode():
        for s in range(T4):
            if kind == "ppo":
                alg.act(x["obs"][s].clone(), x["cobs"][s].clone())
            else:
                alg.act(x["obs"][s].clone(), x["cobs"][s].clone(), x["hist"][s].clone())
            if watch is not None:
                watch(s)
            alg.process_env_step(x["rew"][s] * reward_scale, x["touts"][s].clone(), {"time_outs": x["touts"][s].clone()})
        if kind == "ppo":
            alg.compute_returns(x["cobs"][T4].clone())
        else:
            alg.compute_returns(x["cobs"][T4].clone(), x["hist"][T4].clone())


def _critic_of(alg, kind, x, s):
    """the critic MODULE's answer (normalised units) on step s's inputs"""
    with torch.no_grad():
        if kind == "ppo":
            return alg.actor_critic.critic(x["cobs"][s])
        latent = alg._latent_env_order(x["cobs"][s], x["hist"][s])
        return alg.model.evaluate_joint(x["cobs"][s], latent, x["obs"][s])


def _spy_raw(alg):
    """-> a dict that receives the raw values / returns as they are when the normalising hook runs"""
    raw, inner = {}, alg._vn_after_gae

    def spy():
        raw["values"], raw["returns"], raw["adv"] = alg.storage.values.clone(), alg.storage.returns.clone(), alg.storage.advantages.clone()
        return inner()
    alg._vn_after_gae = spy
    return raw


@pytest.mark.parametrize("kernel", [True, False])
@pytest.mark.parametrize("kind", ["ppo", "cts"])
def test_rollout_holds_raw_values_and_the_update_reads_normalised_rows(emu, monkeypatch, kind, kernel):
    _pair(monkeypatch, kind)
    alg = _alg(emu, kind, kernel, normalize_value=True, normalize_value_until=2 * T4 * N4 + PRE[0])
    vn = alg.actor_critic.value_normalizer
    assert isinstance(vn, ValueNormalization) and alg._vn is vn
    vn.set_state(*PRE)
    stat = vn.stat32.numpy().copy()
    x, raw, seen = _inputs(), _spy_raw(alg), []
    _rollout(alg, kind, x, watch=lambda s: seen.append(alg.storage.values[s].clone()))
    if kernel:
        assert alg._kernel() is not None and alg._kernel().critic.fold is not None and alg._vn_state["lib"] is emu          # the folded critic and the three launches
    else:
        assert alg._kernel() is None and alg._vn_state["lib"] is None
    st = alg.storage
    for s in range(T4):          # during the rollout: raw values, v^ std32 + mean32 of the critic module's answer
        want = _critic_of(alg, kind, x, s).numpy().astype(np.float64) * stat[1] + stat[0]
        np.testing.assert_allclose(seen[s].numpy(), want, atol=2e-6 * (abs(stat[0]) + stat[1]), rtol=2e-6)
        assert torch.equal(seen[s], raw["values"][s])
    # the bootstrap value is raw too: returns[T - 1] = r + gamma v time_out + gamma (1 - done) V(last), every time-out of this rollout being a done
    v_last = _critic_of(alg, kind, x, T4).numpy() * stat[1] + stat[0]
    to = x["touts"][T4 - 1].numpy()
    want_last = x["rew"][T4 - 1].numpy() + alg.gamma * to * raw["values"][T4 - 1].view(-1).numpy() + alg.gamma * (1.0 - to) * v_last.reshape(-1)
    np.testing.assert_allclose(raw["returns"][T4 - 1].view(-1).numpy(), want_last, rtol=2e-6, atol=2e-5)
    # behind GAE: the numpy normalisation of the raw rows, bit for bit; the advantages are not touched; the statistics have not moved
    assert np.array_equal(K.bits(st.values.numpy()), K.bits(K.np_normalise(raw["values"].numpy(), stat)))
    assert np.array_equal(K.bits(st.returns.numpy()), K.bits(K.np_normalise(raw["returns"].numpy(), stat)))
    assert torch.equal(st.advantages, raw["adv"]) and np.array_equal(K.bits(vn.stat32.numpy()), K.bits(stat)) and float(vn.count) == PRE[0]
    alg.update()
    import obs_norm_cases as O
    pre_state = np.array([PRE[0], PRE[1], PRE[2] * PRE[0]])
    tot, mean, var, e_mean, e_var = O.pooled((pre_state, stat[:1], None), raw["returns"].numpy().reshape(-1, 1), 1)
    assert float(vn.count) == tot == PRE[0] + T4 * N4 and vn.host_count() == tot
    assert abs(float(vn.mean) - mean[0]) <= e_mean[0] and abs(float(vn.var) - var[0]) <= e_var[0]
    assert np.array_equal(K.bits(vn.stat32.numpy()), K.bits(K.derived_stat(float(vn.mean), float(vn.var), 1e-2)))
    assert alg.return_stats == tuple(vn.stat32[:2].tolist())
    # count grows by T N per iteration and stops at `until`
    counts = []
    for it in range(3):
        _rollout(alg, kind, _inputs(10 + it))
        alg.update()
        counts.append(float(vn.count) - PRE[0])
    assert counts == [2 * T4 * N4] * 3, counts
    assert all(torch.isfinite(p).all() for p in alg.actor_critic.parameters())


def _weights(alg):
    return {n: p.detach().clone() for n, p in alg.actor_critic.named_parameters()}


@pytest.mark.parametrize("kernel", [True, False])
@pytest.mark.parametrize("kind", ["ppo", "cts"])
def test_reward_scale_invariance(emu, monkeypatch, kind, kernel):
    """Arm B: every reward x 8, statistics (c, 8 mu, 64 sigma^2), eps x 8; arm A: r, (c, mu, sigma^2), eps; the same weights, observations and noise.  Powers of two scale
    exactly, so the stored normalised values and returns are bit-identical; the advantages differ by the 1e-8 of go2sim_normalize_advantages only; the weights after one
    update agree as arm A agrees with itself on reordered mini-batch rows (x 4, floor 2e-6: the rule of tests/test_gpu_parity.py).  With the switch OFF the same pair's
    value losses differ by the factor 64: with values v from the same weights in both arms, the returns R are affine in (r, v) with coefficients of v summing to at most
    3 T + 1 (per step: the time-out bootstrap, gamma v', -v; plus the value itself), so R_B / 8 - R_A and the value's own share differ from the x 8 image by at most
    (7 / 8) (3 T + 2) max |v|, and by the triangle inequality in L2  |sqrt(loss_B) / 8 - sqrt(loss_A)| <= that."""
    _pair(monkeypatch, kind)
    real = torch.randperm
    state = {"flip": False}

    def randperm(n, **k):          # ONE fixed permutation; the yardstick arm reverses the rows inside every mini-batch (PPO: halves; CTS: teacher / student quarters)
        p = real(n, generator=torch.Generator().manual_seed(23 + n))
        if state["flip"]:
            half = n // 2
            p = torch.cat([p[:half].flip(0), p[half:].flip(0)])
        return p.to(k.get("device", "cpu"))
    monkeypatch.setattr(torch, "randperm", randperm)
    x = _inputs()

    def arm(scale, on, flip=False, epochs=2, nmb=2):
        state["flip"] = flip
        alg = _alg(emu, kind, kernel, critic_scale=0.1, normalize_value=on, normalize_value_eps=1e-2 * scale, num_learning_epochs=epochs, num_mini_batches=nmb)
        if on:
            alg.actor_critic.value_normalizer.set_state(PRE[0], PRE[1] * scale, PRE[2] * scale * scale)
        _rollout(alg, kind, x, reward_scale=scale)
        rows = {k: getattr(alg.storage, k).clone() for k in ("values", "returns", "advantages")}
        out = alg.update()
        return rows, _weights(alg), out[0]

    a, wa, la = arm(1.0, True)
    b, wb, lb = arm(8.0, True)
    _, wr, _ = arm(1.0, True, flip=True)
    assert torch.equal(a["values"], b["values"]) and torch.equal(a["returns"], b["returns"])
    np.testing.assert_allclose(b["advantages"].numpy(), a["advantages"].numpy(), rtol=1e-6, atol=1e-9)
    gap_ab = {n: float((wa[n] - wb[n]).abs().median()) for n in wa}
    gap_ar = {n: float((wa[n] - wr[n]).abs().median()) for n in wa}
    print("[value norm %s] reward x 8: largest per-tensor median weight gap %.2e; the same arm on reordered rows %.2e; value loss %.6f vs %.6f" % (kind, max(gap_ab.values()), max(gap_ar.values()), la, lb))
    for n in wa:
        assert gap_ab[n] <= 4.0 * gap_ar[n] + GAP_FLOOR, (n, gap_ab[n], gap_ar[n])
    assert abs(la - lb) <= 1e-5 * max(abs(la), 1.0)
    assert max(float((wa[n] - _weights(_alg(emu, kind, kernel, critic_scale=0.1))[n]).abs().max()) for n in wa) > 1e-4          # (the update did move the weights)
    # the switch off: one step on the whole rollout, so that the loss is the one of the weights both arms share
    oa, _, loa = arm(1.0, False, epochs=1, nmb=1)
    ob, _, lob = arm(8.0, False, epochs=1, nmb=1)
    assert torch.equal(oa["values"], ob["values"])          # raw values of the same critic: they do not follow the rewards
    slack = (7.0 / 8.0) * (3 * T4 + 2) * float(oa["values"].abs().max())
    print("[value norm %s] switch off, reward x 8: value loss %.4f vs %.4f (ratio %.2f); sqrt(loss_B) / 8 - sqrt(loss_A) = %.4f, allowed %.4f" % (kind, loa, lob, lob / loa, lob ** 0.5 / 8 - loa ** 0.5, slack))
    assert abs(lob ** 0.5 / 8.0 - loa ** 0.5) <= slack and slack < 0.1 * loa ** 0.5
    rel = slack / loa ** 0.5          # so sqrt(loss_B / loss_A) / 8 lies within 1 +- rel, rel < 0.1: the factor 64 within what was derived
    assert 64.0 * (1.0 - rel) ** 2 <= lob / loa <= 64.0 * (1.0 + rel) ** 2


def _counting(monkeypatch, lib):
    calls = {k: 0 for k in ENTRY_POINTS}
    for k in ENTRY_POINTS:
        def wrapped(*a, _fn=getattr(lib, k), _k=k):
            calls[_k] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, k, wrapped)
    return calls


@pytest.mark.parametrize("kind", ["ppo", "cts"])
def test_switch_off_changes_nothing(emu, monkeypatch, kind):
    """no new entry point is called, the state dict keeps its keys, and the weights and Adam moments after one update are bit for bit those of a run built without the key"""
    _pair(monkeypatch, kind)
    calls = _counting(monkeypatch, emu)
    out = []
    for kw in ({}, dict(normalize_value=False, normalize_value_eps=1e-2, normalize_value_until=None, normalize_value_preserve=False)):
        alg = _alg(emu, kind, True, **kw)
        keys = set(alg.actor_critic.state_dict())
        assert not any("value_normalizer" in k for k in keys) and alg._vn is None and alg._vn_state is None and alg.return_stats is None
        _rollout(alg, kind, _inputs())
        assert alg._kernel().critic.fold is None
        torch.manual_seed(4)
        alg.update()
        opts = [alg.optimizer] if kind == "ppo" else [alg.optimizer1, alg.optimizer2]
        moments = [v.clone() for o in opts for s in o.state.values() for k, v in sorted(s.items()) if torch.is_tensor(v)]
        out.append((keys, [p.detach().clone() for p in alg.actor_critic.parameters()], moments))
    assert out[0][0] == out[1][0]
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1])) and len(out[0][2]) == len(out[1][2]) > 0 and all(torch.equal(a, b) for a, b in zip(out[0][2], out[1][2]))
    assert calls == {k: 0 for k in ENTRY_POINTS}


@pytest.mark.parametrize("kind", ["ppo", "cts"])
def test_preserve_rewrites_the_last_layer_and_the_next_rollout_follows_it(emu, monkeypatch, kind):
    _pair(monkeypatch, kind)
    res = {}
    for kernel in (True, False):
        alg = _alg(emu, kind, kernel, normalize_value=True, normalize_value_preserve=True)
        vn = alg.actor_critic.value_normalizer
        vn.set_state(*PRE)
        x = _inputs()
        _rollout(alg, kind, x)
        old = vn.stat32.double().clone()
        alg.update()
        new = vn.stat32.double()
        assert float((new - old).abs()[:2].min()) > 1e-3
        # the same rewrite stated in fp64 on a copy of the stepped critic is what the layer now holds: undo it and compare with a run without preservation
        seen = []
        _rollout(alg, kind, x, watch=lambda s: seen.append(alg.storage.values[s].clone()))
        for s in range(T4):          # the next rollout's raw values follow the rewritten layer (the re-pack happened)
            want = _critic_of(alg, kind, x, s).double() * new[1] + new[0]
            np.testing.assert_allclose(seen[s].numpy(), want.numpy(), atol=2e-6 * float(new[0].abs() + new[1]), rtol=2e-6)
        res[kernel] = (seen, copy.deepcopy(alg.actor_critic.critic[-1]), old, new)
    # against the run without preservation: the critic's last layer differs by exactly the rewrite
    plain = _alg(emu, kind, True, normalize_value=True)
    plain.actor_critic.value_normalizer.set_state(*PRE)
    _rollout(plain, kind, _inputs())
    plain.update()
    w0, b0 = plain.actor_critic.critic[-1].weight.double(), plain.actor_critic.critic[-1].bias.double()
    for kernel in (True, False):
        _, last, old, new = res[kernel]
        np.testing.assert_allclose(last.weight.detach().double().numpy(), (w0 * old[1] / new[1]).detach().numpy(), rtol=3e-7)
        np.testing.assert_allclose(last.bias.detach().double().numpy(), ((old[1] * b0 + old[0] - new[0]) / new[1]).detach().numpy(), rtol=3e-7, atol=1e-7)


def test_refusals_at_construction(emu, monkeypatch):
    from go2_rl_gym_amd.rsl_rl.algorithms import PPO, _base
    from go2_rl_gym_amd.rsl_rl.modules import ActorCriticACMoECTS
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic_recurrent import ActorCriticRecurrent
    ac = ActorCriticRecurrent(45, 263, 12, actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_hidden_size=16)
    with pytest.raises(NotImplementedError, match="fused_rnn"):
        PPO(ac, device="cpu", lib=load_oracle(), normalize_value=True)
    PPO(ac, device="cpu", lib=load_oracle())
    assert not hasattr(ac, "value_normalizer")
    with monkeypatch.context() as m:
        m.setenv("GO2_FORCE_COLLECTIVES", "1")
        for kind in ("ppo", "cts"):
            with pytest.raises(NotImplementedError, match="one rank"):
                _alg(emu, kind, normalize_value=True)
            _alg(emu, kind)
    with monkeypatch.context() as m:
        m.setattr(_base, "_world", lambda: 2)
        with pytest.raises(NotImplementedError, match="all-reduce"):
            _alg(emu, "ppo", normalize_value=True)
    with pytest.raises(ValueError, match="eps"):
        _alg(emu, "ppo", normalize_value=True, normalize_value_eps=0.0)


# ---- 3. the runner: CLI, checkpoints, combinations ----------------------------------------------------------------------------------------------------------------
def _args(task="go2_flat", *flags, n=8, seed=5):
    return get_args(["--task", task, "--num_envs", str(n), "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", str(seed), *flags])


def _runner(emu, task="go2_flat", flags=(), log_root=None, train_cfg=None):
    args = _args(task, *flags)
    env, _ = task_registry.make_env(task, args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, None if train_cfg is not None else task, args, train_cfg=train_cfg, log_root=log_root)
    runner.alg.fused_rollout = True
    runner.alg.nn_lib = emu
    return env, runner


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_flag_sets_the_key_and_the_defaults(task):
    _, train_cfg = task_registry.get_cfgs(task)
    a = train_cfg.algorithm
    assert (a.normalize_value, a.normalize_value_eps, a.normalize_value_until, a.normalize_value_preserve) == (False, 1e-2, None, False)
    for flag in ((), ("--normalize_value",)):
        _, cfg = update_cfg_from_args(None, copy.deepcopy(train_cfg), _args(task, *flag))
        assert cfg.algorithm.normalize_value is bool(flag)


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_checkpoint_resumes_in_normalised_units(emu, tmp_path, task):
    """save with the switch on, load into a run WITHOUT the flag: the child is attached, the algorithm switched on, and the first rollout after the load runs on the
    loaded statistics; a checkpoint without the keys loaded into a run with the switch starts from the initial statistics"""
    env, runner = _runner(emu, task, ("--normalize_value",))
    torch.manual_seed(9)
    runner.learn(1, init_at_random_ep_len=True)
    vn = runner.alg.actor_critic.value_normalizer
    assert float(vn.count) == 8 * 24 and runner.alg.return_stats is not None
    path = str(tmp_path / "model.pt")
    runner.save(path)
    sd = {k: v.clone() for k, v in runner.alg.actor_critic.state_dict().items()}
    assert {"value_normalizer.state", "value_normalizer.stat32", "value_normalizer.hyper"} <= set(sd)
    env2, r2 = _runner(emu, task)
    assert r2.alg._vn is None and not hasattr(r2.alg.actor_critic, "value_normalizer")
    r2.learn(1)          # (it has stepped, and packed an unfolded critic, before the load)
    r2.load(path)
    ac2 = r2.alg.actor_critic
    sd2 = ac2.state_dict()
    assert set(sd2) == set(sd) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert r2.alg._vn is ac2.value_normalizer and ac2.value_normalizer.host_count() == 8 * 24
    used, inner = [], r2.alg._vn_after_gae

    def spy():
        used.append((r2.alg._vn.stat32.clone(), r2.alg.storage.values.clone()))
        return inner()
    r2.alg._vn_after_gae = spy
    r2.learn(1)
    assert len(used) == 1 and torch.equal(used[0][0], sd["value_normalizer.stat32"])
    pk = r2.alg._kernel()
    assert pk is None or pk.critic.fold is not None          # (the policy kernel was rebuilt around the folded critic)
    assert float(ac2.value_normalizer.count) == 2 * 8 * 24 and all(torch.isfinite(p).all() for p in ac2.parameters())
    # no keys in the checkpoint, switch on: the initial statistics
    plain = str(tmp_path / "plain.pt")
    env3, r3 = _runner(emu, task)
    r3.save(plain)
    runner.load(plain)
    assert vn.state.tolist() == [0.0, 0.0, 0.0] and np.array_equal(K.bits(vn.stat32.numpy()), K.bits(K.stat_of(0.0, 1.0)))
    r3.load(plain)
    assert not hasattr(r3.alg.actor_critic, "value_normalizer")
    for e in (env, env2, env3):
        e.close()


def test_play_evaluate_and_export_accept_the_checkpoint(emu, tmp_path, monkeypatch):
    import os
    from go2_rl_gym_amd.scripts import play as P
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils.exporter import export_policy_as_jit, export_policy_as_pkl
    train_cfg = copy.deepcopy(task_registry.train_cfgs["go2_flat"])
    e = train_cfg.evaluation
    e.num_envs, e.seconds, e.warmup_s = 24, 0.2, 0.1
    monkeypatch.setitem(task_registry.train_cfgs, "go2_flat", train_cfg)
    env, runner = _runner(emu, "go2_flat", ("--normalize_value",), log_root=str(tmp_path))
    runner.learn(1)
    env.close()
    ac = runner.alg.actor_critic
    obs = torch.randn(4, 45)
    mod = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "x")))
    with torch.no_grad():
        assert torch.allclose(torch.cat([mod(obs[i:i + 1]) for i in range(4)]), ac.act_inference(obs), atol=1e-6)
    assert "value_normalizer.state" in torch.load(export_policy_as_pkl(ac, str(tmp_path / "x")))
    base = ["--task", "go2_flat", "--num_envs", "8", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    out = evaluate(base, log_root=str(tmp_path), env_kwargs={"lib": load_oracle()}, evaluator_kwargs={"nn_lib": emu})
    assert all(np.isfinite(v) for v in out["checkpoints"][0]["overall"].values())
    real = task_registry.make_env
    monkeypatch.setattr(task_registry, "make_env", lambda name, args, env_cfg=None, **kw: real(name, args, env_cfg=env_cfg, lib=load_oracle()))
    env, exported = P.play(get_args(base), steps=2, log_root=str(tmp_path), export_policy=True)
    assert torch.isfinite(env.obs_buf).all() and os.path.exists(exported[0])
    env.close()


@pytest.mark.parametrize("task,flags", [("go2_flat", ("--normalize_value", "--symmetry", "--diagnostics")), ("go2_flat", ("--normalize_value", "--normalize_obs")),
                                        ("go2_flat_cts", ("--normalize_value", "--diagnostics"))])
def test_combinations_run_one_iteration(emu, task, flags):
    env, runner = _runner(emu, task, flags)
    torch.manual_seed(9)
    runner.learn(1, init_at_random_ep_len=True)
    ac = runner.alg.actor_critic
    assert float(ac.value_normalizer.count) == 8 * 24 and all(torch.isfinite(p).all() for p in ac.parameters())
    assert float(runner.alg.storage.returns.abs().max()) < 50.0          # normalised rows
    if "--diagnostics" in flags:
        d = runner.alg.diagnostics
        assert d is not None
    env.close()
