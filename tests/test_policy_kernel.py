"""include/go2nn.h: the rollout's policy evaluation (PPO.act, rsl_rl/algorithms/ppo.py:90-102) as one kernel — here the host build of the
same source (packing, padding, operand order, the sampling head, the Python side) against plain PyTorch fp32.  GPU twin (the MFMA kernel
itself): tests/test_gpu_policy_kernel.py."""
import math
import os

import numpy as np
import pytest
import torch

from helpers import load_nn_emu
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd.rsl_rl.modules.actor_critic import ActorCritic


def _ac(seed=0, dims=(512, 256, 128), n_obs=45, n_priv=263, A=12):
    torch.manual_seed(seed)
    ac = ActorCritic(n_obs, n_priv, A, actor_hidden_dims=list(dims), critic_hidden_dims=list(dims), activation="elu", init_noise_std=1.0)
    with torch.no_grad():
        ac.std.copy_(torch.rand(A) * 0.8 + 0.3)
    return ac


def reference_act(ac, obs, priv, eps):
    with torch.no_grad():
        mu, v = ac.actor(obs), ac.critic(priv)
        a = mu + ac.std * eps
        lp = torch.distributions.Normal(mu, mu * 0.0 + ac.std).log_prob(a).sum(-1)
    return a, mu, lp, v.view(-1)


@pytest.mark.parametrize("N", [1, 33, 200])
@pytest.mark.parametrize("dims", [(512, 256, 128), (40, 24)])
def test_policy_act_matches_torch(N, dims):
    lib = load_nn_emu()
    ac = _ac(dims=dims)
    assert _nn.PolicyKernel.supports(ac)
    pk = _nn.PolicyKernel(lib, ac); pk.pack()
    g = torch.Generator().manual_seed(1)
    obs, priv, eps = torch.randn(N, 45, generator=g), torch.randn(N, 263, generator=g) * 2, torch.randn(N, 12, generator=g)
    st = {k: torch.zeros(N, 12) for k in ("a", "mu", "sig")}; lp, v = torch.zeros(N), torch.zeros(N)
    actions = pk.act(obs, priv, eps, st["a"], st["mu"], st["sig"], lp, v)
    a_ref, mu_ref, lp_ref, v_ref = reference_act(ac, obs, priv, eps)
    np.testing.assert_allclose(st["mu"].numpy(), mu_ref.numpy(), atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(v.numpy(), v_ref.numpy(), atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(actions.numpy(), a_ref.numpy(), atol=2e-6, rtol=2e-6)
    assert torch.equal(actions, st["a"]) and torch.equal(st["sig"], ac.std.detach().expand(N, 12))
    np.testing.assert_allclose(lp.numpy(), lp_ref.numpy(), atol=2e-5, rtol=2e-6)
    # a = mu + std * eps exactly as the eager two-operation formulation on the kernel's own mu
    assert torch.equal(actions, st["mu"] + ac.std.detach() * eps)


def test_forward_and_repack_follow_the_parameters():
    lib = load_nn_emu()
    ac = _ac(seed=3)
    m = _nn.PackedMlp(lib, ac.critic); m.pack()
    x = torch.randn(70, 263)
    with torch.no_grad():
        np.testing.assert_allclose(m.forward(x).numpy(), ac.critic(x).numpy(), atol=2e-6, rtol=2e-6)
        for p in ac.critic.parameters():
            p.add_(torch.randn_like(p) * 0.05)          # an optimizer step, in place: same tensors, new values
        assert m.still_valid()
        assert np.abs(m.forward(x).numpy() - ac.critic(x).numpy()).max() > 1e-3      # stale until re-packed
        m.pack()
        np.testing.assert_allclose(m.forward(x).numpy(), ac.critic(x).numpy(), atol=2e-6, rtol=2e-6)


def test_unsupported_modules_are_rejected():
    lib = load_nn_emu()
    ac = _ac(dims=(600, 64))
    assert not _nn.PolicyKernel.supports(ac)                       # wider than GO2NN_MAX_WIDTH
    ac2 = ActorCritic(45, 263, 12, actor_hidden_dims=[64], critic_hidden_dims=[64], activation="relu")
    assert not _nn.PolicyKernel.supports(ac2)                      # not ELU
    with pytest.raises(ValueError):
        _nn.PackedMlp(lib, ac2.actor)
    d = _nn.Go2nnMlp(); d.num_layers = 9
    import ctypes as C
    assert lib.go2nn_packed_floats(C.byref(d)) < 0 and b"unsupported" in lib.go2nn_last_error()


def test_ppo_act_through_the_policy_kernel(tmp_path, monkeypatch):
    """PPO.act with the fused policy kernel (host build) inside the runner's rollout against the module-by-module path (ppo.py:90-102): the rows
    of the first step agree to fp32 round-off (later steps see different actions at the 1e-7 level, so only behaviour is compared), the
    weights are re-packed at the start of every rollout, checkpoints and state dicts are untouched."""
    from helpers import load_oracle
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    monkeypatch.setenv("GO2_FUSE_STEP", "1")
    res = {}
    for mode in ("modules", "kernel"):
        args = get_args(["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"])
        env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
        runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path / mode))
        alg = runner.alg
        alg.fused_rollout = True
        if mode == "kernel":
            alg.nn_lib = load_nn_emu()
        torch.manual_seed(4)
        runner._rollout(None)
        st = alg.storage
        assert (alg._policy_kernel() is not None) == (mode == "kernel")
        res[mode] = {k: getattr(st, k).clone() for k in ("actions", "mu", "sigma", "values", "actions_log_prob", "observations", "rewards")}
        if mode == "kernel":      # an optimizer step later the next rollout sees the new weights (pack at step 0)
            st.clear()
            with torch.no_grad():
                for p in alg.actor_critic.actor.parameters():
                    p.mul_(0.5)
            runner._rollout(None)
            with torch.no_grad():
                np.testing.assert_allclose(st.mu[3].numpy(), alg.actor_critic.actor(st.observations[3]).numpy(), atol=2e-6, rtol=2e-6)
        env.close()
    a, b = res["modules"], res["kernel"]
    assert torch.equal(a["observations"][0], b["observations"][0]) and torch.equal(a["sigma"], b["sigma"])
    for k in ("mu", "values", "actions"):
        np.testing.assert_allclose(a[k][0].numpy(), b[k][0].numpy(), atol=2e-6, rtol=2e-6, err_msg=k)
    np.testing.assert_allclose(a["actions_log_prob"][0].numpy(), b["actions_log_prob"][0].numpy(), atol=2e-5)
    assert torch.isfinite(b["rewards"]).all() and abs(float(a["rewards"].mean() - b["rewards"].mean())) < 0.05


def cts_policy_kernel_vs_modules(lib, device, kind="CTS", N=203, full=False, atol=3e-6):
    """_nn.PolicyKernelCTS (go2nn_mlp_forward_rows + go2nn_policy_act_latent: CTS.act of one rollout step, rsl_rl/algorithms/cts.py:112-149) against the modules:
    the env-ordered latent of both encoders on their env subsets, actor / critic on [latent | obs] / [latent | priv], the sampling head, the bootstrap value"""
    from go2_rl_gym_amd.rsl_rl.modules import ActorCriticCTS, ActorCriticMoECTS, fused, fused_cts
    torch.manual_seed(7)
    dims = (dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], teacher_encoder_hidden_dims=[512, 256], student_encoder_hidden_dims=[512, 256], latent_dim=32) if full else
            dict(actor_hidden_dims=[40, 24], critic_hidden_dims=[40, 24], teacher_encoder_hidden_dims=[48, 20], student_encoder_hidden_dims=[36, 28], latent_dim=8))
    if kind == "MoECTS":
        dims.update(student_encoder_hidden_dims=dims["student_encoder_hidden_dims"] + [16], expert_num=4)
    n_priv = 263 if full else 61
    model = (ActorCriticCTS if kind == "CTS" else ActorCriticMoECTS)(45, n_priv, 12, N, 5, init_noise_std=1.0, **dims).to(device)
    with torch.no_grad():
        model.std.copy_(torch.rand(12) * 0.8 + 0.3)
    saved = (fused._LIB, fused._NN)
    fused._LIB, fused._NN = object(), lib          # (cts_plan only asks whether the pair is there)
    try:
        plan = fused_cts.cts_plan(model)
    finally:
        fused._LIB, fused._NN = saved
    assert plan is not None and (plan.student is not None) == (kind == "CTS")
    ids = torch.arange(N, device=device)
    ti, si = ids[ids % 4 != 0], ids[ids % 4 == 0]
    pk = _nn.PolicyKernelCTS(lib, model, plan, ti, si); pk.pack()
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g).to(device)
    obs, priv, hist, eps = r(N, 45), r(N, n_priv) * 2, r(N, 225), r(N, 12)
    with torch.no_grad():
        lat_ref = torch.empty(N, plan.L, device=device)
        lat_ref[ti] = model.teacher_encoder(priv[ti]); lat_ref[si] = model.student_latent(hist[si])[0]
        mu_ref, v_ref = model.policy_mean(lat_ref, obs), model.evaluate_joint(priv, lat_ref, obs).view(-1)
        a_ref = mu_ref + model.std * eps
        lp_ref = torch.distributions.Normal(mu_ref, mu_ref * 0.0 + model.std).log_prob(a_ref).sum(-1)
    latent = torch.full((N, plan.L), 9.0, device=device)
    if pk.enc_s is None:
        latent[si] = lat_ref[si]          # (the MoE student encoder is the caller's)
    pk.latents(priv, hist, latent)
    np.testing.assert_allclose(latent.cpu().numpy(), lat_ref.cpu().numpy(), atol=atol)
    st = {k: torch.zeros(N, 12, device=device) for k in ("a", "mu", "sig")}; lp, v = torch.zeros(N, device=device), torch.zeros(N, device=device)
    actions = pk.act(latent, obs, priv, eps, st["a"], st["mu"], st["sig"], lp, v)
    np.testing.assert_allclose(st["mu"].cpu().numpy(), mu_ref.cpu().numpy(), atol=atol, rtol=2e-6)
    np.testing.assert_allclose(v.cpu().numpy(), v_ref.cpu().numpy(), atol=atol, rtol=2e-6)
    np.testing.assert_allclose(actions.cpu().numpy(), a_ref.cpu().numpy(), atol=atol, rtol=2e-6)
    np.testing.assert_allclose(lp.cpu().numpy(), lp_ref.cpu().numpy(), atol=10 * atol, rtol=2e-6)
    assert torch.equal(actions, st["a"]) and torch.equal(actions, st["mu"] + model.std.detach() * eps)
    np.testing.assert_allclose(pk.value(latent, priv).view(-1).cpu().numpy(), v_ref.cpu().numpy(), atol=atol, rtol=2e-6)


@pytest.mark.parametrize("kind,N,full", [("CTS", 203, False), ("MoECTS", 64, False), ("CTS", 5, False), ("CTS", 130, True)])
def test_cts_policy_kernel_matches_modules(kind, N, full):
    cts_policy_kernel_vs_modules(load_nn_emu(), "cpu", kind, N, full)


NO_GOAL_MASK = [True] * 6 + [False] * 3 + [True] * 36          # the observation without its three command entries (envs/go2/go2_config.py)


def cts_rollout_latent_vs_float64(sim_lib, nn_lib, device, kind="MoECTS", N=203, full=False):
    """CTS.act / CTS._rollout_latent of the two MoE students AT ALGORITHM LEVEL (which arm the algorithm picks, which buffers it hands over, when it rebuilds the split
    weight images) against the same model copied to float64: teacher rows of the env-ordered latent = teacher_encoder(priv[ti]) (its last module is the L2 normaliser),
    student rows = student_latent(hist[si])[0]; mu / values / actions = policy_mean / evaluate_joint / mu + std * eps on that latent.
      MoECTS   -> the soft mixture's tail as ONE launch (go2nn_moe_mix_forward) behind the experts / gate as torch modules under own_forward;
      MoENGCTS -> PolicyKernelCTS.moe_mix_ok is false (it asks for ActorCriticMoECTS.student_moe_parts): model.student_latent as torch modules under own_forward
                  (split images of the no-goal encoder, GroupedHeads' padded narrow batched product on cuda) + index_copy_ into the latent buffer.
    Bound — the project's rule for device arithmetic against float64 (tests/test_gpu_recurrent.py, test_split_operand_policy_kernel_is_as_close_to_float64_as_fp32): the error
    is at most 4 x the error of the same modules evaluated by torch in fp32 on the same device, + 2e-7; errors in units of max(1, largest |float64 value|) of the tensor
    (fp32 rounding is relative: the 2e-7 floor is ~2 ulp of the tensor's scale; the latent is normalised, |.| <= 1, and taken absolutely).
    -> [(what, error, fp32 torch error)] of every comparison made"""
    import copy
    from go2_rl_gym_amd.rsl_rl.algorithms import MoECTS, MoENGCTS
    from go2_rl_gym_amd.rsl_rl.modules import ActorCriticCTS, ActorCriticMoECTS, ActorCriticMoENGCTS, fused
    torch.manual_seed(7)
    E = 8 if full else 4          # (full: the widths and the expert count of go2_moe_cts / go2_moe_ng_cts)
    dims = (dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], teacher_encoder_hidden_dims=[512, 256], student_encoder_hidden_dims=[512, 256], latent_dim=32) if full else
            dict(actor_hidden_dims=[40, 24], critic_hidden_dims=[40, 24], teacher_encoder_hidden_dims=[48, 20], student_encoder_hidden_dims=[36, 28], latent_dim=8))
    if kind == "MoECTS":
        dims.update(student_encoder_hidden_dims=dims["student_encoder_hidden_dims"] + [256 if full else 16], expert_num=E)
    else:
        dims.update(student_expert_num=E, obs_no_goal_mask=NO_GOAL_MASK)
    n_priv, T = (263 if full else 61), 2
    model = (ActorCriticMoECTS if kind == "MoECTS" else ActorCriticMoENGCTS)(45, n_priv, 12, N, 5, init_noise_std=1.0, **dims).to(device)
    with torch.no_grad():
        model.std.copy_(torch.rand(12) * 0.8 + 0.3)
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g).to(device)
    obs, priv, hist, eps = r(N, 45), r(N, n_priv) * 2, r(N, 225), r(N, 12)
    ids = torch.arange(N, device=device)
    ti, si = ids[ids % 4 != 0], ids[ids % 4 == 0]          # (what CTS.__init__ must arrive at for teacher_env_ratio 0.75: computed here on its own)

    def modules(dt):
        """-> latent, mu, values, actions of the CURRENT parameters, by the modules in dtype dt (plain torch: no gradient and outside own_forward, FusedSequential runs as nn.Sequential)"""
        m = copy.deepcopy(model).to(dt)
        o, p, h = obs.to(dt), priv.to(dt), hist.to(dt)
        with torch.no_grad():
            lat = torch.empty(N, dims["latent_dim"], device=device, dtype=dt)
            lat[ti] = m.teacher_encoder(p[ti]); lat[si] = m.student_latent(h[si])[0]
            mu, v = m.policy_mean(lat, o), m.evaluate_joint(p, lat, o).view(-1)
            return {"latent": lat.double(), "mu": mu.double(), "values": v.double(), "actions": (mu + m.std * eps.to(dt)).double()}

    report = []

    def check(tag, got):
        r64, r32 = modules(torch.float64), modules(torch.float32)
        for k in ("latent", "mu", "values", "actions"):
            if k in got:
                scale = max(1.0, float(r64[k].abs().max()))
                e, e32 = float((got[k].double() - r64[k]).abs().max()) / scale, float((r32[k] - r64[k]).abs().max()) / scale
                print("[rollout latent %s N=%d full=%s] %s %s: error %.3g (torch fp32 %.3g)" % (kind, N, full, tag, k, e, e32))
                report.append((tag + " " + k, e, e32))
                assert e <= 4 * e32 + 2e-7, (tag, k, e, e32)
        return r64

    def perturb(seed, params):
        gp = torch.Generator().manual_seed(seed)
        with torch.no_grad():          # an optimizer step's worth and more, IN PLACE: same addresses (what the image cache is keyed by), new values
            for p in params:
                p.add_((torch.randn(p.shape, generator=gp) * 0.5 * float(p.abs().mean())).to(device))

    saved, saved_noise = (fused._LIB, fused._NN), ActorCriticCTS._noise
    try:
        if device == "cpu":
            fused._LIB, fused._NN = sim_lib, nn_lib
        alg = (MoECTS if kind == "MoECTS" else MoENGCTS)(model, N, 5, device=device, lib=sim_lib, use_graphs=False, fused_loss=True, fused_rollout=True)
        if device == "cpu":
            alg.nn_lib = nn_lib
        alg.init_storage(N, T, [45], [n_priv], [12])
        assert torch.equal(alg.teacher_env_idxs, ti) and torch.equal(alg.student_env_idxs, si) and alg.fused_rollout
        ActorCriticCTS._noise = lambda self, like: eps          # (the algorithm asks a module whose _noise is replaced per step: _RolloutHeads._rollout_noise)
        pk = alg._policy_kernel()
        assert pk is not None and pk.enc_s is None and pk.moe_mix_ok(model) == (kind == "MoECTS")          # which arm of CTS._rollout_latent runs
        st = alg.storage

        def act(s):
            st.step = s
            a = alg.act(obs, priv, hist)
            assert alg._pk_packed and a.shape == (N, 12)
            return {"latent": alg._latent_buf.clone(), "mu": st.mu[s].clone(), "values": st.values[s].view(-1).clone(), "actions": a.clone()}

        first = act(0)
        check("act", first)
        assert torch.equal(first["actions"], st.actions[0]) and torch.equal(first["actions"], first["mu"] + model.std.detach() * eps)
        # the latent alone, twice on the same inputs: the same bits (no atomics, no uninitialised padding read, nothing left over in the buffer)
        alg._latent_buf.fill_(9.0)
        l1 = alg._rollout_latent(pk, priv, hist).clone()
        alg._latent_buf.fill_(-9.0)
        l2 = alg._rollout_latent(pk, priv, hist).clone()
        assert torch.equal(l1, l2) and torch.equal(l1, first["latent"])
        # new student weights at the same addresses: the next rollout (step 0: act packs and empties the image cache itself) ...
        perturb(11, model.student_parameters())
        alg.parameters_changed()
        second = act(0)
        check("act after a weight change, step 0", second)
        assert float((second["latent"][si] - first["latent"][si]).abs().max()) > 1e-2, "the perturbation did not move the student latent: the check above would be empty"
        assert torch.equal(second["latent"][ti], first["latent"][ti])          # (the teacher encoder's weights did not change)
        # ... and in the middle of a rollout (a checkpoint loaded at step 1, OnPolicyRunnerCTS.load): only parameters_changed() tells act() that the packed weights and
        # the split images beside them are stale (every network changes there: the packed teacher encoder / actor / critic too)
        perturb(12, [p for n, p in model.named_parameters() if n != "std"])
        alg.parameters_changed()
        third = act(1)
        check("act after a weight change, step 1", third)
        assert float((third["latent"][si] - second["latent"][si]).abs().max()) > 1e-2
        # ... and _rollout_latent on its own (compute_returns calls it after the last step)
        perturb(13, model.student_parameters())
        alg.parameters_changed()
        check("_rollout_latent after a weight change", {"latent": alg._rollout_latent(pk, priv, hist).clone()})
    finally:
        fused._LIB, fused._NN = saved
        ActorCriticCTS._noise = saved_noise
    return report


@pytest.mark.parametrize("N", [5, 203])
@pytest.mark.parametrize("kind", ["MoECTS", "MoENGCTS"])
def test_cts_rollout_latent_matches_float64(kind, N):
    """host twin of tests/test_gpu_policy_kernel.py::test_cts_rollout_latent_on_gpu (the host builds of both libraries)"""
    from helpers import load_oracle
    cts_rollout_latent_vs_float64(load_oracle(), load_nn_emu(), "cpu", kind, N)


def test_forward_rows_refuses_bad_descriptions():
    import ctypes as C
    lib = load_nn_emu()
    ac = _ac(dims=(40, 24))
    m = _nn.PackedMlp(lib, ac.critic); m.pack()
    x, y = torch.zeros(4, 263), torch.zeros(4, 1)
    descs, packed = (C.POINTER(_nn.Go2nnMlp) * 1)(C.pointer(m.desc)), (C.c_void_p * 1)(m.packed.data_ptr())
    io = lambda **kw: (_nn.Go2nnMlpIO * 1)(_nn.Go2nnMlpIO(**dict(dict(x=x.data_ptr(), x2=None, rows=None, y=y.data_ptr(), ldx=263, ldx2=0, kx=263, nrows=4, ldy=1, normalize=0), **kw)))
    assert lib.go2nn_mlp_forward_rows(descs, packed, io(), 1, None) == 0
    assert lib.go2nn_mlp_forward_rows(descs, packed, io(kx=200), 1, None) < 0 and b"segments" in lib.go2nn_last_error()          # a second segment without x2
    assert lib.go2nn_mlp_forward_rows(descs, packed, io(ldx=100), 1, None) < 0 and lib.go2nn_mlp_forward_rows(descs, packed, io(nrows=0), 1, None) < 0
    assert lib.go2nn_mlp_forward_rows(descs, packed, io(), 3, None) < 0


def test_the_query_names_the_kernel_that_serves_a_network():
    """go2nn_mlp_arith (include/go2nn.h): the host test build answers 0; the HIP library — loaded here without a GPU, the query is host arithmetic — answers 3 (split-operand planes)
    for every network of the BASELINE tasks and 1 (fp32 MFMA) where two neighbouring 512-wide activations do not fit the LDS as planes."""
    import ctypes as C
    from go2_rl_gym_amd import _nn, build
    def desc(dims):
        d = _nn.Go2nnMlp(); d.num_layers = len(dims) - 1
        for i, v in enumerate(dims):
            d.dims[i] = v
        return d
    emu = load_nn_emu()
    assert emu.go2nn_mlp_arith(C.byref(desc((45, 512, 256, 128, 12)))) == 0
    hip = _nn.bind(build.build_nn())
    nets = [(45, 512, 256, 128, 12), (263, 512, 256, 128, 1),          # go2 / go2_flat: actor, critic
            (77, 512, 256, 128, 12), (295, 512, 256, 128, 1), (263, 512, 256, 32), (225, 512, 256, 32)]          # go2_cts: [latent | obs] actor, [latent | priv] critic, teacher / student encoder
    if os.environ.get("GO2_GEMM_SPLIT", "1") == "1":
        assert [hip.go2nn_mlp_arith(C.byref(desc(n))) for n in nets] == [3] * len(nets)
        assert hip.go2nn_mlp_arith(C.byref(desc((300, 512, 512, 12)))) == 1
    assert hip.go2nn_mlp_arith(C.byref(desc((45, 600, 12)))) < 0 and b"unsupported" in hip.go2nn_last_error()
