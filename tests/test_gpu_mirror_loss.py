"""The mirror (equivariance) loss of symmetry-augmented PPO on the device (`algorithm.mirror_loss_coef`): go2nn_mirror_loss against float64 with the torch fp32
formulation on the GPU as the yardstick of the error, its refusals, the swap invariance, an equivariant network reading zero, the graph-mode PPO update against the
eager formulation (coefficient 0 and 0.5 in one run: 0 is the code as it was, the yardstick), and the term lowering what it penalises.  Run with -m gpu."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_mirror_loss_host as mh  # noqa: E402
from test_gpu_parity import CLIP_OFF, GAP1_MED  # noqa: E402
from go2_rl_gym_amd import _nn  # noqa: E402
from go2_rl_gym_amd.envs.go2.go2_config import GO2Cfg  # noqa: E402
from go2_rl_gym_amd.utils.symmetry import mirror_tables  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1
    return lib


@pytest.fixture(scope="module")
def nn():
    lib = _nn.load_nn()
    assert lib.go2nn_is_device_library() == 1
    return lib


@pytest.fixture(scope="module")
def tables():
    return mirror_tables(GO2Cfg())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("B,A,K", mh.SHAPES)
def test_entry_point_on_gpu_against_float64(nn, tables, B, A, K):
    """tests/test_mirror_loss_host.py::test_entry_point_against_float64 on the device: the kernel's largest error against the float64 restatement, per quantity, is at
    most 4 x that of torch autograd in fp32 on the GPU; sentinels untouched, two launches bit-identical, coef 0 adds nothing.  Measured on one MI355X, kernel / torch
    fp32 (the run prints every shape): at (1000, 12, 128) loss 5.3e-8 / 5.3e-8, gz_a 2.4e-10 / 2.4e-10, dW_mu 7.2e-9 / 2.3e-8, gb_a 5.8e-9 / 7.6e-9, db_mu 2.1e-8 /
    2.3e-8; at (257, 1, 4) loss 1.6e-8 / 1.6e-8, gz_a 1.4e-9 / 1.4e-9, dW_mu 5.5e-8 / 6.4e-8, gb_a 2.9e-8 / 2.9e-8, db_mu 6.2e-9 / 6.2e-9.  The largest ratio over the 13
    shapes is 2.1 (dW_mu at (3, 1, 4): 1.6e-7 / 7.7e-8); the loss's is 1.3 ((3, 16, 256): 6.7e-8 / 5.3e-8).  The loss is a single number, and torch's mean often lands on
    the fp32 number nearest the float64 value: the kernel adds the workgroups' sums of e^2 in fp64 and rounds once for that reason (with an fp32 sum of per-workgroup
    fp32 losses the cases (257, 1, 4) and (257, 16, 256) read 7.6e-8 and 1.4e-7, one fp32 step off, against torch's 1.6e-8 and 1.8e-8)."""
    mh.check_entry_point(nn, mh.make_case(B, A, K, tables), DEV, _stream(), "device")


def test_refusals_on_gpu_write_nothing(nn, tables):
    mh.check_refusals(nn, tables, DEV, _stream())
    mh.check_table_refusals(nn, tables)


def test_swapping_the_halves_on_gpu(nn, tables):
    mh.check_swap(nn, tables, DEV, _stream())


def test_equivariant_network_reads_zero_on_gpu(nn):
    mh.check_equivariant_reads_zero(nn, DEV, _stream(), "device")


# ---- graph mode against the eager formulation ---------------------------------------------------------------------------------------------------------------
N_ENVS, ITERS = 64, 3


def _train_arm(monkeypatch, coef, graph, iters):
    """One arm of go2_flat at 64 envs x 24 steps with symmetry on, pinned as tests/test_gpu_symmetry.py pins its arms: the same seed and initial weights, a fixed
    learning rate, the smooth objective (CLIP_OFF), pre-drawn exploration noise, ONE fixed permutation.  -> (env, runner, weights after iteration 1, alg.mirror_loss
    after iteration 1)"""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic import ActorCritic
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", str(N_ENVS), "--headless", "--seed", "3"])
    env, _ = task_registry.make_env("go2_flat", args)
    torch.manual_seed(3)
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    a = train_cfg.algorithm
    a.schedule, a.clip_param, a.symmetry, a.mirror_loss_coef = "fixed", CLIP_OFF, True, coef
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, train_cfg=train_cfg, log_root=None, use_graphs=graph)
    alg = runner.alg
    assert alg.use_graphs == graph and alg._sym is not None and alg.mirror_loss_coef == coef and alg.fused_loss and alg.fused_rollout
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
    first = ml = None
    for it in range(iters):
        buf.copy_(torch.randn(buf.shape, generator=gen))
        runner.learn(1, init_at_random_ep_len=(it == 0))
        if it == 0:
            first, ml = {n: p.detach().cpu().numpy().copy() for n, p in alg.actor_critic.named_parameters()}, alg.mirror_loss
    torch.cuda.synchronize()
    return env, runner, first, ml


def test_graph_mode_matches_the_eager_formulation_with_the_coefficient_0_and_on(hip, nn, monkeypatch):
    """After iteration 1 (20 Adam steps of 1e-3 from the same weights on the same rollout in the same order, symmetry on) the per-tensor median gap between graph mode
    and the eager formulation with mirror_loss_coef = 0.5 is at most twice the gap with the coefficient 0 measured in this same run (0 is the code as it was: the
    yardstick; the factor 2 for the added term's different summation order on the two paths), plus the floor of tests/test_gpu_parity.py (GAP1_MED).  Graph mode with
    the term is captured and finite over three iterations, alg.mirror_loss agrees between the two formulations to 1e-5 relative, and the term changes the weights."""
    import torch
    gaps, graph_weights, mls = {}, {}, {}
    for coef in (0.0, 0.5):
        first = {}
        for graph in (False, True):
            env, runner, first[graph], mls[(coef, graph)] = _train_arm(monkeypatch, coef, graph, ITERS if (graph and coef) else 1)
            alg = runner.alg
            if graph:
                assert alg.graphs_captured() or not coef          # (the first update runs eagerly: the one-iteration arm has not captured yet)
                assert alg._aug is not None and alg._acc.numel() == (3 if coef else 2) and (alg._ml_dev is not None) == bool(coef)
                assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
            env.close()
            del env, runner, alg          # (their HIP graphs, streams and events: collected here, with the device idle)
            torch.cuda.synchronize()
            gc.collect()
        graph_weights[coef] = first[True]
        gaps[coef] = {n: float(np.median(np.abs(first[True][n] - first[False][n]))) for n in first[True]}
        print("[mirror loss, coef %s] graph vs eager after iteration 1: largest per-tensor median gap %.2e (%s); alg.mirror_loss eager %.6e, graph %.6e"
              % (coef, max(gaps[coef].values()), max(gaps[coef], key=gaps[coef].get), mls[(coef, False)], mls[(coef, True)]))
    for n in gaps[0.5]:
        assert gaps[0.5][n] <= 2.0 * gaps[0.0][n] + GAP1_MED, (n, gaps[0.5][n], gaps[0.0][n])
    e, g = mls[(0.5, False)], mls[(0.5, True)]
    assert e > 0 and abs(g - e) <= 1e-5 * e, (e, g)
    assert mls[(0.0, False)] == 0.0 and mls[(0.0, True)] == 0.0
    last = [n for n in graph_weights[0.5] if n.startswith("actor.") and n.endswith(".weight")][-1]
    assert float(np.median(np.abs(graph_weights[0.5][last] - graph_weights[0.0][last]))) > 1e-5


def test_term_lowers_what_it_penalises_on_gpu(hip, nn, tables):
    """tests/test_mirror_loss_host.py::test_term_lowers_what_it_penalises through the captured device path (go2nn_mirror_loss behind go2nn_ppo_heads)"""
    alg = mh.check_term_lowers_the_gap(tables, DEV, hip, "graph mode on the device")
    assert alg.use_graphs and alg._acc.numel() == 3 and alg._ml_dev is not None and alg._aug is not None
