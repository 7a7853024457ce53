"""Value normalisation on the device (`algorithm.normalize_value`): go2nn_value_norm_apply / _update / go2nn_value_head_fold against numpy bit for bit, against the host
build and against the float64 restatements (the cases of value_norm_cases.py at the host tests' shapes); graph mode (folded critic, captured rollout and returns graphs)
against the eager mode (the torch statement) with the switch off and on in one run, for PPO, CTS and MoE-CTS; output preservation across a re-pack.  Run with -m gpu."""
import copy
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import obs_norm_cases as O  # noqa: E402
import value_norm_cases as K  # noqa: E402
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
@pytest.mark.parametrize("n", K.NS)
def test_values_and_returns_on_gpu_are_numpy_and_the_host_build_bit_for_bit(nn, n):
    """per n: aligned tensors and views offset by one float, with and without the partial table"""
    emu = load_nn_emu()
    for offset in (0, 1):
        for with_partials in (True, False):
            res = K.apply_case(nn, DEV, n, offset, with_partials)
            K.check_apply_case(res, with_partials)
            host = K.apply_case(emu, "cpu", n, offset, with_partials)
            assert np.array_equal(K.bits(res["got_v"]), K.bits(host["got_v"])) and np.array_equal(K.bits(res["got_r"]), K.bits(host["got_r"])), (n, offset)


def test_moments_on_gpu_equal_the_pooled_two_pass_statistics(nn):
    a = K.check_moments(nn, DEV, label=" gpu")
    assert K.check_moments(nn, DEV, label=" gpu") == a          # no atomics, a fixed order: two runs give the same bits


@pytest.mark.parametrize("Kw", [1, 37, 128])
def test_fold_and_preservation_on_gpu(nn, Kw):
    K.check_fold(nn, DEV, Kw)
    K.check_preservation(nn, DEV, Kw, label=" gpu")


def test_refusals_on_gpu_write_nothing(nn):
    K.check_refusals(nn, DEV)


# ---- 2. graph mode against the eager mode ----------------------------------------------------------------------------------------------------------------------
N_ENVS, ITERS = 64, 5          # (iteration 3 replays the captured rollout and warms the compute_returns step up, iteration 4 captures that one too, iteration 5 is replays only: its merge must not depend on a hook that ran through Python)
PRE = (2000.0, 0.8, 2.0)          # preloaded statistics: iteration 1 already runs on non-trivial ones


def _train_arm(hip, monkeypatch, task, normalize, graph, iters, preserve=False, before_last=None):
    """tests/test_gpu_obs_norm.py::_train_arm with this switch: `task` at 64 envs x 24 steps, the same seed and initial weights, a fixed learning rate, the smooth
    objective (CLIP_OFF), pre-drawn exploration noise and one fixed permutation (PPO: torch.randperm replaced; the CTS family: the keyed device permutation of graph mode
    handed to the eager arm, as tests/test_gpu_parity.py does).  -> env, runner, the weights after iteration 1, the state after iteration 1, the raw returns of iteration 1"""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic import ActorCritic
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic_cts import ActorCriticCTS
    from go2_rl_gym_amd.utils import get_args
    cts = task != "go2_flat"
    args = get_args(["--task", task, "--num_envs", str(N_ENVS), "--headless", "--seed", "3"] + (["--normalize_value"] if normalize else []))
    env, _ = task_registry.make_env(task, args)
    torch.manual_seed(3)
    _, train_cfg = task_registry.get_cfgs(task)
    a = train_cfg.algorithm
    keep = (a.schedule, a.clip_param, a.normalize_value, a.normalize_value_preserve)
    a.schedule, a.clip_param, a.normalize_value_preserve = "fixed", CLIP_OFF, preserve
    try:
        runner, _ = task_registry.make_alg_runner(env, task, args, train_cfg=train_cfg, log_root=None, use_graphs=graph)
    finally:
        a.schedule, a.clip_param, a.normalize_value, a.normalize_value_preserve = keep
    alg = runner.alg
    ac = alg.actor_critic
    assert alg.use_graphs == graph and hasattr(ac, "value_normalizer") == normalize and alg.fused_loss and alg.fused_rollout
    raw, snap = [], None
    if normalize:
        snap = copy.deepcopy(ac)          # the weights of iteration 1's rollout, for the magnitudes _raw_return_slack needs
        ac.value_normalizer.set_state(*PRE)
        inner = alg._vn_after_gae

        def spy():
            if not raw and not torch.cuda.is_current_stream_capturing():
                raw.append(alg.storage.returns.clone())
            return inner()
        alg._vn_after_gae = spy
    T, A = alg.storage.num_transitions_per_env, alg.storage.actions.shape[-1]
    gen, buf, calls = torch.Generator().manual_seed(17), torch.zeros(T, N_ENVS, A, device=alg.device), [0]

    def noise(self_, like):
        row = buf[calls[0] % T]; calls[0] += 1
        assert row.shape == like.shape
        return row
    monkeypatch.setattr(ActorCriticCTS if cts else ActorCritic, "_noise", noise)
    if not cts:
        perm = torch.randperm(N_ENVS * T, generator=torch.Generator().manual_seed(23)).to(alg.device)
        monkeypatch.setattr(torch, "randperm", lambda n, **kw: perm)
    elif not graph:
        assert alg._own_plan() is not None
        st = alg.storage
        key = torch.tensor([int((torch.initial_seed() * 0x9E3779B1 + 0x7F4A7C15) & 0x7FFFFFFF), 0, 0, 0], dtype=torch.int32, device=alg.device)          # _RolloutHeads._make_shuffle_key
        order = torch.empty(N_ENVS * T, dtype=torch.int64, device=alg.device)

        def keyed(nmb):
            nt, ns = st.teacher_num_envs * T, st.student_num_envs * T
            rc = hip.go2sim_cts_minibatch_indices(C.c_void_p(order.data_ptr()), nmb, nt, ns, C.c_void_p(st.ref2mine.data_ptr()), C.c_void_p(key.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream(alg.device).cuda_stream))
            assert rc == 0, hip.go2sim_last_error().decode()
            rows = nt // nmb + ns // nmb
            return [order[i * rows:(i + 1) * rows].clone() for i in range(nmb)]
        st.mini_batch_indices = keyed
    env.common_step_counter = 0
    first = state = None
    for it in range(iters):
        if before_last is not None and it == iters - 1:
            before_last(runner)
        buf.copy_(torch.randn(buf.shape, generator=gen))
        runner.learn(1, init_at_random_ep_len=(it == 0))
        if it == 0:
            first = {n: p.detach().cpu().numpy().copy() for n, p in ac.named_parameters()}
            if normalize:
                state = ac.value_normalizer.state.cpu().numpy().copy()
                runner._test_slack = _raw_return_slack(snap, alg, cts, raw[0])          # (the storage still holds iteration 1's rows)
    torch.cuda.synchronize()
    return env, runner, first, state, (raw[0].cpu().numpy().reshape(-1, 1) if raw else None)


def _raw_return_slack(snap, alg, cts, raw_returns):
    """How far the raw returns of the graph arm (folded critic) and of the eager arm (the kernel's v^, then v^ std32 + mean32 in torch) may lie apart, from the data's
    magnitudes and the number formats alone.  Per raw value: both arms run the same critic through the same kernel, each within the forward tolerance of
    tests/test_policy_kernel.py (FWD: 2e-6 + 2e-6 |x|) of the exact critic in its own units — v^ units, scaled by std32, in the eager arm, raw units in the graph arm —;
    the fold rounds every W_k std32 and b std32 + mean32 (2^-24 relative each: 2^-24 (std32 S + |mean32|) twice over, S = max over the rows of sum_k |W_k h_k| + |b|);
    torch's product and sum round twice at the raw value's magnitude V.  Through GAE: a lambda-return is a convex combination of n-step returns, each with ONE bootstrap
    value of weight gamma^n <= 1, and a time-out bootstrap gamma v ends its chain, so a return moves by at most 2 g_v; the recursion's own fp32 rounding (at most 6
    operations per step on magnitudes <= M = max |R| + V + max |r|, T steps, both arms) adds 12 T 2^-24 M."""
    import torch
    st = alg.storage
    T = st.num_transitions_per_env
    mu, sd = PRE[1], float(K.stat_of(PRE[1], PRE[2])[1])          # (iteration 1 ran on the preloaded statistics)
    priv = st.privileged_observations.flatten(0, 1)
    with torch.no_grad():
        if cts:
            hist, N = st.history.flatten(0, 1), st.num_envs
            teacher = torch.isin(torch.arange(priv.shape[0], device=priv.device) % N, alg.teacher_env_idxs)
            lt, ls = snap.teacher_encoder(priv[teacher]), snap.student_latent(hist[~teacher])[0]
            latent = torch.empty(priv.shape[0], lt.shape[1], device=priv.device)
            latent[teacher], latent[~teacher] = lt, ls
            x = torch.cat([latent, priv], dim=1)
        else:
            x = priv
        last = [m for m in snap.critic.modules() if isinstance(m, torch.nn.Linear)][-1]
        seen = []
        hook = last.register_forward_pre_hook(lambda m, inp: seen.append(inp[0]))
        vhat = snap.critic(x)
        hook.remove()
        S = float((seen[0].abs() @ last.weight.abs().t()).max() + last.bias.abs().max())
    Vh = float(vhat.abs().max())
    V = sd * Vh + abs(mu)
    u = 2.0 ** -24
    g_v = (2e-6 + 2e-6 * Vh) * sd + (2e-6 + 2e-6 * V) + 2.0 * u * (sd * S + abs(mu)) + 2.0 * u * V
    M = float(raw_returns.abs().max()) + V + float(st.rewards.abs().max())
    return 2.0 * g_v + 12.0 * T * u * M


def _close(env, *rest):
    import torch
    env.close()
    del env, rest          # (their HIP graphs, streams and events: collected here, with the device idle, not in the middle of the next arm's replay)
    torch.cuda.synchronize()
    gc.collect()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts", "go2_flat_moe_cts"])
def test_graph_mode_matches_the_eager_mode_with_the_switch_off_and_on(hip, nn, monkeypatch, task):
    """After iteration 1 the per-tensor median weight gap between graph mode (the folded critic, the three launches) and the eager mode (the torch statement) with the
    switch ON is at most 4 x the gap with the switch OFF measured in this same run, plus the floor of tests/test_gpu_parity.py (GAP1_MED = 2e-6): the rule of
    tests/test_gpu_obs_norm.py.  The two arms' merged states agree — and agree with the pooled two-pass statistics of the rollout's raw returns — within the derived
    moment bound.  With the switch on under GO2_STRICT_GRAPHS=1 the rollout and the update are captured and the weights stay finite over five iterations, the last of which only replays graphs (the statistics still take its rollout in)."""
    import torch
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    gaps, states, raws, slack = {}, {}, {}, 0.0
    pre_state, pre_stat = np.array([PRE[0], PRE[1], PRE[2] * PRE[0]]), K.stat_of(PRE[1], PRE[2])
    for normalize in (False, True):
        first = {}
        for graph in (False, True):
            env, runner, first[graph], state, raw = _train_arm(hip, monkeypatch, task, normalize, graph, ITERS if (graph and normalize) else 1)
            alg = runner.alg
            if normalize:
                states[graph], raws[graph] = state, raw
                slack = max(slack, runner._test_slack)
                tot, mean, var, e_mean, e_var = O.pooled((pre_state, pre_stat[:1], None), raw, 1)
                got_mean, got_var = state[1], state[2] / state[0]
                print("[value norm %s, %s] state after iteration 1: |mean err| %.3e (bound %.3e), |var err| %.3e (bound %.3e); raw returns mean %.3f std %.3f"
                      % (task, "graph" if graph else "eager", abs(got_mean - mean[0]), e_mean[0], abs(got_var - var[0]), e_var[0], raw.mean(), raw.std()))
                assert state[0] == tot == PRE[0] + N_ENVS * 24
                assert abs(got_mean - mean[0]) <= e_mean[0] and abs(got_var - var[0]) <= e_var[0], (graph,)
                pk = alg._kernel()
                assert pk is not None and (pk.critic.fold is not None) == graph and (alg._vn_state["lib"] is not None) == graph          # eager: the torch statement
            if graph and normalize:
                caps = runner.graphs_captured()
                assert caps["rollout"] and caps["update"] and runner._returns_graph is not None and runner._returns_graph.graph is not None, caps
                assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
                vn = alg.actor_critic.value_normalizer
                assert float(vn.count) == PRE[0] + ITERS * N_ENVS * 24 and vn.host_count() == float(vn.count) and bool(torch.isfinite(vn.stat32).all())
                assert alg.return_stats == tuple(vn.stat32[:2].tolist())
            elif graph:
                assert alg._vn is None and alg._vn_state is None and alg._kernel().critic.fold is None
            _close(env, runner, alg)
        gaps[normalize] = {n: float(np.median(np.abs(first[True][n] - first[False][n]))) for n in first[True]}
        peak = {n: float(np.abs(first[True][n] - first[False][n]).max()) for n in first[True]}
        print("[value norm %s, %s] graph vs eager after iteration 1: largest per-tensor median gap %.2e (%s), largest element gap %.2e"
              % (task, "on" if normalize else "off", max(gaps[normalize].values()), max(gaps[normalize], key=gaps[normalize].get), max(peak.values())))
    # the two arms' rollouts of iteration 1 differ only by the fold's rounding in the stored raw values: their merged states agree within the moment bound
    _, _, _, e_mean, e_var = O.pooled((pre_state, pre_stat[:1], None), raws[True], 1)
    sg, se = states[True], states[False]
    d_mean, d_var = abs(sg[1] - se[1]), abs(sg[2] / sg[0] - se[2] / se[0])
    gap_raw = float(np.abs(raws[True] - raws[False]).max())
    print("[value norm %s] state graph vs eager after iteration 1: |mean difference| %.3e (bound %.3e), |var difference| %.3e (bound %.3e); largest raw-return difference %.3e (derived slack %.3e)"
          % (task, d_mean, e_mean[0], d_var, e_var[0], gap_raw, slack))
    # The moment bound is the summation's.  The arms' inputs differ — the graph arm's raw values come from the folded critic, the eager arm's from torch's product — by at
    # most `slack` per return (_raw_return_slack: derived from the data's magnitudes and the number formats, not from the two arms' difference): that much of the mean,
    # and 2 (std + |mean - preloaded mean|) slack + slack^2 of the pooled variance, is the data's, not the merge's.
    assert gap_raw <= slack, (gap_raw, slack)
    sd = float(raws[True].std()) + abs(float(raws[True].mean()) - PRE[1])
    assert sg[0] == se[0] and d_mean <= e_mean[0] + slack and d_var <= e_var[0] + 2.0 * sd * slack + slack ** 2
    ratio = max(gaps[True][n] / (gaps[False][n] + GAP1_MED) for n in gaps[True])
    print("[value norm %s] largest gap_on / (gap_off + 2e-6) over the tensors: %.3f (allowed: gap_on <= 4 gap_off + 2e-6)" % (task, ratio))
    for n in gaps[True]:
        assert gaps[True][n] <= 4.0 * gaps[False][n] + GAP1_MED, (n, gaps[True][n], gaps[False][n])


def test_preservation_and_the_repack_in_graph_mode(hip, nn, monkeypatch):
    """normalize_value_preserve on, graph mode, one iteration more than the capture needs: the LAST rollout — replayed, packed inside the graph behind the rewrite of the
    iteration before — stored raw values of the rewritten layer: the stored normalised values are the critic's answer (as it stood in front of that iteration) on the
    stored rows, within the forward tolerance plus the round trip's rounding"""
    import torch
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    snap = {}

    def before_last(runner):
        ac = runner.alg.actor_critic
        torch.cuda.synchronize()
        snap["critic"], snap["stat"] = copy.deepcopy(ac.critic), ac.value_normalizer.stat32.clone()
        snap["replayed"] = runner._rollout_graph is not None
    env, runner, _, _, _ = _train_arm(hip, monkeypatch, "go2_flat", True, True, ITERS + 1, preserve=True, before_last=before_last)
    alg = runner.alg
    vn = alg.actor_critic.value_normalizer
    assert snap["replayed"] and runner.graphs_captured() == {"rollout": True, "update": True}
    assert float((vn.stat32.cpu() - torch.from_numpy(K.stat_of(PRE[1], PRE[2]))).abs().max()) > 1e-4          # the statistics moved
    with torch.no_grad():
        want = snap["critic"](alg.storage.privileged_observations.flatten(0, 1)).view(-1)
    got = alg.storage.values.view(-1)
    mu, sd = float(snap["stat"][0]), float(snap["stat"][1])
    tol = 2e-6 + 8.0 * 2.0 ** -24 * (abs(mu) + sd * float(want.abs().max())) / sd
    gap = float((got - want).abs().max())
    print("[value norm] preservation in graph mode: stored normalised values vs the rewritten critic on the stored rows: max gap %.3e (allowed %.3e + 2e-6 relative)" % (gap, tol))
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=tol, rtol=2e-6)
    assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
    _close(env, runner, alg)
