"""The recurrent actor-critic on the MI355X: the memory kernels (include/go2nn.h ABI 7) at the rollout's and the update's sizes against float64, with the rule of
test_split_operand_policy_kernel_is_as_close_to_float64_as_fp32 (error <= 4 x the fp32 torch evaluation's + 2e-7), split-operand and fp32-MFMA products; the two
golden iterations on the GPU; task go2_flat_rnn at 4096 envs (rollout and update replayed from HIP graphs, 30 iterations, play + export) and its GRU / 2-layer
variants through the replayed update graph; the cell kernels called directly and the memory at small, ragged and stacked shapes (the checks of
tests/test_recurrent_host.py on the HIP kernels).  Run with -m gpu."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402


@pytest.fixture(scope="module")
def kernels():
    from go2_rl_gym_amd.rsl_rl.modules import fused
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1
    was = (fused._LIB, fused._NN)
    fused.set_library(lib)
    assert fused._NN.go2nn_is_device_library() == 1
    yield lib
    fused._LIB, fused._NN = was


def _mem(typ, K, H, L=1, seed=0):
    from go2_rl_gym_amd.rsl_rl.modules import Memory
    torch.manual_seed(seed)
    return Memory(K, type=typ, num_layers=L, hidden_size=H)


def _errs(got, f32, f64):
    return (got.double() - f64).abs().max().item(), (f32.double() - f64).abs().max().item()


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("typ,H", [("lstm", 256), ("gru", 256), ("lstm", 512), ("gru", 512)])
def test_rollout_steps_are_as_close_to_float64_as_fp32(kernels, monkeypatch, typ, H, split):
    """24 chained steps of both memories at 4096 envs with resets (RolloutMemory.step / .reset) vs nn.LSTM / nn.GRU in float64 and in fp32"""
    from go2_rl_gym_amd.rsl_rl.modules import ActorCriticRecurrent, fused, fused_rnn
    monkeypatch.setattr(fused, "_SPLIT", split)
    N, T = 4096, 24
    torch.manual_seed(0)
    ac = ActorCriticRecurrent(45, 263, 12, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], rnn_type=typ, rnn_hidden_size=H).cuda()
    ac.init_hidden_states(N, "cuda")
    rm = fused_rnn.RolloutMemory(ac)
    rm.images()
    assert (rm._imgs[0] is not None) == split
    lstm = typ == "lstm"
    refs = {}
    for dt in (torch.float64, torch.float32):
        refs[dt] = [type(m.rnn)(m.rnn.input_size, H, 1).to("cuda", dt) for m in (ac.memory_a, ac.memory_c)]
        for r, m in zip(refs[dt], (ac.memory_a, ac.memory_c)):
            r.load_state_dict({k: v.to(dt) for k, v in m.rnn.state_dict().items()})
    z = lambda dt: torch.zeros(1, N, H, device="cuda", dtype=dt)
    st = {dt: [(z(dt), z(dt)) if lstm else z(dt) for _ in range(2)] for dt in refs}
    g = torch.Generator(device="cuda").manual_seed(1)
    worst = [0.0, 0.0]
    with torch.no_grad():
        for s in range(T):
            xs = [torch.randn(N, 45, device="cuda", generator=g), torch.randn(N, 263, device="cuda", generator=g)]
            hs = rm.step(xs)
            for j in range(2):
                outs = {}
                for dt in refs:
                    outs[dt], st[dt][j] = refs[dt][j](xs[j].to(dt).unsqueeze(0), st[dt][j])
                e, e32 = _errs(hs[j], outs[torch.float32][0], outs[torch.float64][0])
                worst = [max(worst[0], e), max(worst[1], e32)]
                assert e <= 4 * e32 + 2e-7, (s, j, e, e32)
            done = (torch.rand(N, device="cuda", generator=g) < 0.05).to(torch.uint8)
            rm.reset(done)
            keep = (done == 0).view(1, N, 1)
            for dt in refs:
                st[dt] = [tuple(x * keep for x in p) if lstm else p * keep for p in st[dt]]
    torch.cuda.synchronize()
    print("rollout %s H=%d split=%s: max |err| vs float64 %.3g (fp32 torch %.3g)" % (typ, H, split, worst[0], worst[1]))


def _reference_sequence(rnn, x, saved, dones):
    lstm = isinstance(rnn, nn.LSTM)
    saved = [s.to(x.dtype) for s in saved]
    st = (saved[0][0], saved[1][0]) if lstm else saved[0][0]
    ys = []
    for t in range(x.shape[0]):
        if t > 0:
            d = dones[t - 1].bool().view(1, -1, 1)
            st = tuple(torch.where(d, s[t], c) for s, c in zip(saved, st)) if lstm else torch.where(d, saved[0][t], st)
        y, st = rnn(x[t:t + 1], st)
        ys.append(y[0])
    return torch.stack(ys)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("typ", ["lstm", "gru"])
def test_update_recurrence_is_as_close_to_float64_as_fp32(kernels, monkeypatch, typ, split):
    """RnnFunction at B = 1024, T = 24, H = 256 (forward output and every parameter gradient) vs float64 and fp32 autograd through nn.LSTM / nn.GRU"""
    from go2_rl_gym_amd.rsl_rl.modules import fused, fused_rnn
    monkeypatch.setattr(fused, "_SPLIT", split)
    T, B, K, H = 24, 1024, 45, 256
    mem = _mem(typ, K, H).cuda()
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(T, B, K, device="cuda", generator=g)
    dones = (torch.rand(T, B, device="cuda", generator=g) < 0.05).to(torch.uint8)
    saved = [torch.randn(T, 1, B, H, device="cuda", generator=g) * 0.3 for _ in range(2 if typ == "lstm" else 1)]
    gy = torch.randn(T, B, H, device="cuda", generator=g) / (T * B)
    y = fused_rnn.memory_sequence(mem, x, saved, dones)
    (y * gy).sum().backward()
    res = {}
    for dt in (torch.float64, torch.float32):
        r = type(mem.rnn)(K, H, 1).to("cuda", dt)
        r.load_state_dict({k: v.to(dt) for k, v in mem.rnn.state_dict().items()})
        yr = _reference_sequence(r, x.to(dt), saved, dones)
        (yr * gy.to(dt)).sum().backward()
        res[dt] = (yr.detach(), {n: p.grad for n, p in r.named_parameters()})
    e, e32 = _errs(y.detach(), res[torch.float32][0], res[torch.float64][0])
    print("update %s split=%s: y %.3g (fp32 %.3g)" % (typ, split, e, e32))
    assert e <= 4 * e32 + 2e-7
    for n, p in mem.rnn.named_parameters():
        e, e32 = _errs(p.grad, res[torch.float32][1][n], res[torch.float64][1][n])
        print("  d%s %.3g (fp32 %.3g)" % (n, e, e32))
        assert e <= 4 * e32 + 2e-7, n


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("graphs", [False, True])
def test_two_golden_iterations_on_the_gpu(kernels, monkeypatch, typ, graphs):
    """tests/golden/ppo_recurrent_iterations.npz on the device: the policy kernel on the memories' output, the fixed-shape update; eager and as a HIP graph
    (update captured after the first one: the second iteration replays it)"""
    from go2_rl_gym_amd.rsl_rl.algorithms import PPO
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic, ActorCriticRecurrent
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_recurrent_iterations.npz"))
    p = typ + "_"
    T, N = g[p + "it0_rew"].shape
    ac = ActorCriticRecurrent(45, 60, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type=typ, rnn_hidden_size=16)
    ac.load_state_dict({k[len(p) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p + "w0_")})
    alg = PPO(ac, num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3,
              max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01, device="cuda", lib=kernels, use_graphs=True if graphs else "uncaptured")
    alg.init_storage(N, T, [45], [60], [12])
    worst = 0.0
    for it in range(2):
        q = p + "it%d_" % it
        obs, cobs, noise = (torch.from_numpy(g[q + k]).cuda() for k in ("obs", "cobs", "noise"))
        with torch.inference_mode():
            for t in range(T):
                monkeypatch.setattr(ActorCritic, "_noise", lambda self, like, _t=t: noise[_t])
                a = alg.act(obs[t], cobs[t])
                np.testing.assert_allclose(a.cpu().numpy(), g[q + "actions"][t], atol=1e-6)
                np.testing.assert_allclose(alg.storage.actions_log_prob[t].view(-1).cpu().numpy(), g[q + "logp"][t], atol=1e-5)
                alg.process_env_step(torch.from_numpy(g[q + "rew"][t]).cuda(), torch.from_numpy(g[q + "dones"][t]).bool().cuda(),
                                     {"time_outs": torch.from_numpy(g[q + "time_outs"][t]).bool().cuda()})
            alg.compute_returns(cobs[T])
        np.testing.assert_allclose(alg.storage.returns.cpu().numpy(), g[q + "returns"], atol=2e-6)
        alg.update()
        lr, want = alg.learning_rate, float(g[q + "lr"])
        assert abs(lr - want) <= 2e-7 * want, (lr, want)          # (the rate lives in an fp32 device tensor: the fp32 representation of the reference's float)
        for k, v in ac.state_dict().items():
            d = np.abs(v.cpu().numpy() - g[q + "w_" + k])
            worst = max(worst, float(d.max()))
            np.testing.assert_allclose(v.cpu().numpy(), g[q + "w_" + k], atol=2e-6, rtol=1e-5, err_msg="iteration %d: %s" % (it, k))
    assert alg.graphs_captured() == graphs
    print("golden %s graphs=%s: max |dw| %.3g" % (typ, graphs, worst))


def _runner(task, N, tmp=None, seed=1):
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", task, "--num_envs", str(N), "--headless", "--seed", str(seed)])
    env, _ = task_registry.make_env(task, args)
    torch.manual_seed(seed)
    runner, _ = task_registry.make_alg_runner(env, task, args, log_root=str(tmp) if tmp else None)
    return env, runner, args


def test_go2_flat_rnn_trains_in_graph_mode_and_plays(kernels, tmp_path):
    """task go2_flat_rnn at 4096 envs: 30 iterations, rollout and update replayed from HIP graphs, finite weights and losses; the checkpoint plays and exports"""
    env, runner, args = _runner("go2_flat_rnn", 4096, tmp_path)
    runner.save_interval = 1000
    losses, update = [], runner.alg.update
    runner.alg.update = lambda: losses.append(update()) or losses[-1]
    for _ in range(30):
        runner.learn(1)
    assert len(losses) == 30 and np.isfinite(np.array(losses, dtype=np.float64)).all(), losses
    caps = runner.graphs_captured()
    assert caps == {"rollout": True, "update": True}, caps
    for k, v in runner.alg.actor_critic.state_dict().items():
        assert torch.isfinite(v).all(), k
    env.close()
    from go2_rl_gym_amd.scripts.play import play
    args.num_envs = None
    env2, exported = play(args, steps=20, log_root=str(tmp_path), export_policy=True)
    env2.close()
    assert exported and os.path.exists(exported[0])
    jit = torch.jit.load(exported[0])
    out = jit(torch.zeros(1, 45))
    assert out.shape == (1, 12) and torch.isfinite(out).all()


def _graph_and_eager_snapshots(monkeypatch, N, rnn_type=None, layers=None, ITERS=2):
    """task go2_flat_rnn (rnn_type / layers: its GRU / stacked variants, set as tests/test_recurrent_host.py:test_runner_builds_the_recurrent_policy sets them) trained
    ITERS iterations on identical rollouts, eager and with the update replayed from a HIP graph -> {use_graphs: [parameters after each iteration]}"""
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    from go2_rl_gym_amd.utils import get_args
    out = {}
    for mode in (False, True):
        args = get_args(["--task", "go2_flat_rnn", "--num_envs", str(N), "--headless", "--seed", "3"])
        env, _ = task_registry.make_env("go2_flat_rnn", args)
        torch.manual_seed(3)
        _, train_cfg = task_registry.get_cfgs("go2_flat_rnn")
        sched0, clip0, type0, layers0 = train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param, train_cfg.policy.rnn_type, train_cfg.policy.rnn_num_layers
        train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param = "fixed", 1.0e6
        if rnn_type is not None:
            train_cfg.policy.rnn_type, train_cfg.policy.rnn_num_layers = rnn_type, layers
        try:
            runner, _ = task_registry.make_alg_runner(env, "go2_flat_rnn", args, train_cfg=train_cfg, log_root=None, use_graphs=mode)
        finally:
            train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param = sched0, clip0
            train_cfg.policy.rnn_type, train_cfg.policy.rnn_num_layers = type0, layers0
        alg = runner.alg
        assert alg.use_graphs == mode and alg.clip_param == 1.0e6 and alg._rnn_memory() is not None
        if rnn_type is not None:
            rnn = alg.actor_critic.memory_a.rnn
            assert isinstance(rnn, nn.LSTM if rnn_type == "lstm" else nn.GRU) and rnn.num_layers == layers == alg.actor_critic.memory_c.rnn.num_layers
        T, A = alg.storage.num_transitions_per_env, alg.storage.actions.shape[-1]
        gen, buf, calls = torch.Generator().manual_seed(17), torch.zeros(T, N, A, device=alg.device), [0]

        def noise(self_, like, buf=buf, calls=calls, T=T):
            row = buf[calls[0] % T]; calls[0] += 1
            return row
        monkeypatch.setattr(ActorCritic, "_noise", noise)
        snaps = []
        for it in range(ITERS):
            buf.copy_(torch.randn(buf.shape, generator=gen))
            runner.learn(1, init_at_random_ep_len=(it == 0))
            snaps.append({n: p.detach().cpu().numpy().copy() for n, p in alg.actor_critic.named_parameters()})
        torch.cuda.synchronize()
        assert alg.graphs_captured() == mode
        out[mode] = snaps
        env.close()
    return out


def _graph_vs_eager_gaps(out, label, bounds):
    """bounds: per iteration (largest per-tensor median gap or None, largest element gap or None) -> the largest per-tensor median gap of every iteration"""
    meds = []
    for it, (med_bound, max_bound) in enumerate(bounds):
        g, e = out[True][it], out[False][it]
        med = {n: float(np.median(np.abs(g[n] - e[n]))) for n in g}
        big = {n: float(np.abs(g[n] - e[n]).max()) for n in g}
        print("[graph vs eager %s] after iteration %d: largest per-tensor median gap %.1e (%s), largest element gap %.1e (%s)"
              % (label, it + 1, max(med.values()), max(med, key=med.get), max(big.values()), max(big, key=big.get)))
        assert all(np.isfinite(v).all() for v in g.values()) and all(np.isfinite(v).all() for v in e.values())
        assert med_bound is None or max(med.values()) <= med_bound, med
        assert max_bound is None or max(big.values()) <= max_bound, big
        meds.append(max(med.values()))
    return meds


def test_go2_flat_rnn_graph_update_equals_eager_update(kernels, monkeypatch):
    """task go2_flat_rnn at 4096 envs, 2 iterations on identical rollouts (same env seed, the same injected sampling noise), clip far away and a fixed rate: the
    update replayed from a HIP graph (fused clip + Adam) against the eager update (autograd over the same kernels, torch's clip and Adam), held as the CTS twin
    (tests/test_gpu_parity.py:test_cts_training_graph_vs_eager_on_gpu) holds them.  After iteration 1 the two arms have seen the same data: the median gap of every
    parameter tensor within 2e-6 (a dropped, doubled or mis-fed launch moves its tensor by ~1e-3 per Adam step), single elements within 2e-3 (Adam turns the sign of a
    near-zero gradient into a full 1e-3 step).  After iteration 2 (the graph arm's update replayed; the rounding differences have been through 24 env steps) the
    per-tensor median within 1e-3, an order of magnitude under what a stale replay does."""
    out = _graph_and_eager_snapshots(monkeypatch, 4096)
    _graph_vs_eager_gaps(out, "go2_flat_rnn", ((2e-6, 2e-3), (1e-3, None)))


# After iteration 2 the parent's 1e-3 holds a variant only where its measured gap is under a third of it.  Measured on an MI355X at 256 envs (largest per-tensor
# median gap after iteration 2): GRU x 1 8.5e-5, LSTM x 2 1.5e-7, GRU x 2 2.8e-6 — all three under 3.3e-4, so all three are held; None would mean finiteness only.
IT2_MEDIAN_BOUND = {("gru", 1): 1e-3, ("lstm", 2): 1e-3, ("gru", 2): 1e-3}


@pytest.mark.parametrize("rnn_type,layers", [("gru", 1), ("lstm", 2), ("gru", 2)])
def test_gru_and_stacked_graph_update_equals_eager_update(kernels, monkeypatch, rnn_type, layers):
    """the GRU and the 2-layer memories through the replayed update graph, at 256 envs: after iteration 1 (both arms have seen the same data) the bounds of
    test_go2_flat_rnn_graph_update_equals_eager_update, for the reason given there; after iteration 2 finite parameters, the gap printed, and the parent's 1e-3
    where IT2_MEDIAN_BOUND says the variant's measured gap leaves a factor of three"""
    out = _graph_and_eager_snapshots(monkeypatch, 256, rnn_type, layers)
    _graph_vs_eager_gaps(out, "go2_flat_rnn %s x %d, 256 envs" % (rnn_type, layers), ((2e-6, 2e-3), (IT2_MEDIAN_BOUND[(rnn_type, layers)], None)))


# ---- the memory at small, ragged and stacked shapes: the checks of tests/test_recurrent_host.py (there on the host build) on the HIP kernels -----------------
# What only the __global__ functions of csrc/go2nn_rnn.h contain — the flat index split k / H, k % H, the reset's row (k / H) % B over L > 1 layers, the grid sized by
# the larger of two jobs with the smaller job's guard, the k < B H tail of the last workgroup — at 255 / 256 / 257 elements, H odd and up to 512, unequal job pairs.
from test_recurrent_host import (CELL_SHAPES, RESET_SHAPES, ROLLOUT_CASES, TWO_JOBS, UPDATE_CASES, check_cell_backward, check_cell_forward,  # noqa: E402
                                 check_cell_two_jobs, check_refusals, check_reset, check_shape_refusal, rollout_steps, update_sequence)

DEV = "cuda:0"


def _nn_lib():
    from go2_rl_gym_amd.rsl_rl.modules import fused
    assert fused._NN.go2nn_is_device_library() == 1
    return fused._NN


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_forward_on_gpu(kernels, typ, B, H):
    """go2nn_rnn_cell_forward alone: h, c and the saved blocks under the fp32 rule, slots / carries / aliases bit for bit, nothing written past any output"""
    check_cell_forward(_nn_lib(), DEV, typ, B, H)


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_backward_on_gpu(kernels, typ, B, H):
    """go2nn_rnn_cell_backward on the forward kernel's own gates against autograd through the float64 restatement: last step, no done, random done"""
    check_cell_backward(_nn_lib(), DEV, typ, B, H)


@pytest.mark.parametrize("specs", TWO_JOBS, ids=["small-first", "large-first"])
def test_two_unequal_cell_jobs_in_one_launch_on_gpu(kernels, specs):
    """the grid is sized by the larger job and the smaller one is guarded, whichever comes first: each job bit-equal to itself launched alone, every element written"""
    check_cell_two_jobs(_nn_lib(), DEV, specs)


@pytest.mark.parametrize("B,H", RESET_SHAPES)
def test_reset_on_gpu(kernels, B, H):
    """go2nn_rnn_reset over 1 .. 4 states and 1 .. 3 layers: the row of flat element k is (k / H) % B"""
    check_reset(_nn_lib(), DEV, B, H)


def test_refusals_on_gpu(kernels):
    check_refusals(_nn_lib(), DEV)
    check_shape_refusal(kernels, DEV)
    torch.cuda.synchronize()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L,N", ROLLOUT_CASES)
def test_stacked_ragged_rollout_on_gpu(kernels, monkeypatch, typ, H, L, N, split):
    """RolloutMemory.step / .reset with up to three layers at ragged sizes and one env (layer l fed from layer l - 1's in-place state), the critic-only step;
    bit-reproducible from run to run"""
    from go2_rl_gym_amd.rsl_rl.modules import fused
    monkeypatch.setattr(fused, "_SPLIT", split)
    a = rollout_steps(DEV, typ, H, L, N, rule=True)
    b = rollout_steps(DEV, typ, H, L, N, rule=True)
    torch.cuda.synchronize()
    assert _same(a, b)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L,T,B,K", UPDATE_CASES)
def test_stacked_ragged_update_on_gpu(kernels, monkeypatch, typ, H, L, T, B, K, split):
    """memory_sequence with up to three layers (RnnFunction.backward hands dgi W_ih down), states and dones as the strided views of recurrent_fixed_batches: the
    output and all 4 L parameter gradients under the fp32 rule; bit-reproducible from run to run"""
    from go2_rl_gym_amd.rsl_rl.modules import fused
    monkeypatch.setattr(fused, "_SPLIT", split)
    a = update_sequence(DEV, typ, H, L, T, B, K, rule=True)
    b = update_sequence(DEV, typ, H, L, T, B, K, rule=True)
    torch.cuda.synchronize()
    assert _same(a, b)
