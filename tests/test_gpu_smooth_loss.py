"""The temporal action-smoothness loss of PPO on env-block mini-batches on the device (`algorithm.smooth_loss_coef`): go2nn_smooth_loss against float64 with the torch
fp32 formulation on the GPU as the yardstick of the error (every time-segment count the shape allows), go2nn_smooth_indices, the refusals, the closed forms, the
graph-mode PPO update against the eager formulation (coefficient 0 and 0.5 in one run: 0 is the code as it was, the yardstick), and the term lowering what it
penalises.  Run with -m gpu."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import load_hip, load_oracle  # noqa: E402
import test_smooth_loss_host as sh  # noqa: E402
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
    lib = _nn.load_nn()
    assert lib.go2nn_is_device_library() == 1
    return lib


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("blocks,T,n,A,K", sh.SHAPES)
def test_entry_point_on_gpu_against_float64(nn, blocks, T, n, A, K):
    """tests/test_smooth_loss_host.py::test_entry_point_against_float64 on the device, for the five patterns of pair weights: the kernel's largest error against the
    float64 restatement, per quantity, is at most 4 x that of torch autograd in fp32 on the GPU in the same run; sentinels untouched, two launches bit-identical, coef 0
    adds nothing.  At these sizes the launch's own choice is the largest segment count (T / 2 segments of two or three rows, every one with its halo); one segment — the
    plain walk — is forced as well for the all-pairs and the 30 % patterns, under the same bound.  Measured on one MI355X, kernel / torch fp32 (the run prints every
    case): at (2, 24, 9, 12, 128), all pairs, loss 2.3e-8 / 3.7e-8, gz_a 2.2e-10 / 2.8e-10, dW_mu 4.8e-9 / 3.4e-8, gb_a 1.2e-9 / 1.1e-9, db_mu 1.9e-9 / 2.8e-9; the largest
    ratio over the 66 cases is 3.1 (db_mu — rounding noise around 0, it telescopes — at (2, 25, 3, 1, 4), one segment: 1.2e-8 / 3.7e-9); the loss's largest is 1.0."""
    try:
        for pattern in sh.PATTERNS:
            sh.check_entry_point(nn, sh.make_case(blocks, T, n, A, K, pattern), DEV, _stream(), "device", pattern)
        assert nn.go2nn_smooth_loss_set_segments(1) == 0
        for pattern in ("ones", "random"):
            sh.check_entry_point(nn, sh.make_case(blocks, T, n, A, K, pattern), DEV, _stream(), "device, one segment", pattern)
    finally:
        nn.go2nn_smooth_loss_set_segments(0)


def test_segment_counts_agree_on_gpu(nn):
    """T = 25 (no count divides it) at 1, 2, 3, 5 and 12 segments: the loss is the same number (an fp64 sum of the same fp32 terms), gz_a the same bytes (a row's
    gradient does not depend on who owns its neighbours), and the partial-row count follows the setting"""
    c = sh.make_case(2, 25, 9, 12, 128, "random")
    seen = {}
    try:
        for S in (1, 2, 3, 5, 12):
            assert nn.go2nn_smooth_loss_set_segments(S) == 0
            assert nn.go2nn_smooth_loss_rows(2, 25, 9, 12, 128) == 2 * 2 * S
            rc, got, gz, _ = sh.run_kernel(nn, c, DEV, _stream())
            assert rc == 0
            seen[S] = (got["loss"].tobytes(), gz.tobytes())
    finally:
        nn.go2nn_smooth_loss_set_segments(0)
    assert all(v == seen[1] for v in seen.values())


def test_indices_on_gpu(nn):
    sh.check_indices(nn, load_oracle(), DEV, _stream())


def test_refusals_on_gpu_write_nothing(nn):
    sh.check_refusals(nn, DEV, _stream())


def test_closed_forms_on_gpu(nn):
    sh.check_closed_forms(nn, DEV, _stream(), "device")


# ---- graph mode against the eager formulation ---------------------------------------------------------------------------------------------------------------
N_ENVS, ITERS = 64, 3


def _train_arm(monkeypatch, coef, graph, iters):
    """One arm of go2_flat at 64 envs x 24 steps, pinned as tests/test_gpu_mirror_loss.py pins its arms: the same seed and initial weights, a fixed learning rate, the
    smooth objective (CLIP_OFF), pre-drawn exploration noise, ONE fixed order through the randperm hook (the row permutation with the coefficient 0, the env permutation
    with it on).  -> (env, runner, weights after iteration 1, alg.smooth_loss after iteration 1)"""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic import ActorCritic
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", str(N_ENVS), "--headless", "--seed", "3"])
    env, _ = task_registry.make_env("go2_flat", args)
    torch.manual_seed(3)
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    a = train_cfg.algorithm
    a.schedule, a.clip_param, a.smooth_loss_coef = "fixed", CLIP_OFF, coef
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, train_cfg=train_cfg, log_root=None, use_graphs=graph)
    alg = runner.alg
    assert alg.use_graphs == graph and alg.smooth_loss_coef == coef and alg.fused_loss and alg.fused_rollout
    T, A = alg.storage.num_transitions_per_env, alg.storage.actions.shape[-1]
    gen, buf, calls = torch.Generator().manual_seed(17), torch.zeros(T, N_ENVS, A, device=alg.device), [0]

    def noise(self_, like):
        row = buf[calls[0] % T]; calls[0] += 1
        assert row.shape == like.shape
        return row
    monkeypatch.setattr(ActorCritic, "_noise", noise)
    g = torch.Generator().manual_seed(23)
    perms = {N_ENVS * T: torch.randperm(N_ENVS * T, generator=g).to(alg.device), N_ENVS: torch.randperm(N_ENVS, generator=g).to(alg.device)}
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: perms[n])
    env.common_step_counter = 0
    first = sl = None
    for it in range(iters):
        buf.copy_(torch.randn(buf.shape, generator=gen))
        runner.learn(1, init_at_random_ep_len=(it == 0))
        if it == 0:
            first, sl = {n: p.detach().cpu().numpy().copy() for n, p in alg.actor_critic.named_parameters()}, alg.smooth_loss
    torch.cuda.synchronize()
    return env, runner, first, sl


def test_graph_mode_matches_the_eager_formulation_with_the_coefficient_0_and_on(hip, nn, monkeypatch):
    """After iteration 1 (20 Adam steps of 1e-3 from the same weights on the same rollout in the same order) the per-tensor median gap between graph mode and the eager
    formulation with smooth_loss_coef = 0.5 is at most twice the gap with the coefficient 0 measured in this same run (0 is the code as it was: the yardstick; the factor
    2 for the added term's different summation order on the two paths), plus the floor of tests/test_gpu_parity.py (GAP1_MED).  Graph mode with the term is captured and
    finite over three iterations, alg.smooth_loss agrees between the two formulations to 1e-5 relative, and the term changes the weights."""
    import torch
    gaps, graph_weights, sls = {}, {}, {}
    for coef in (0.0, 0.5):
        first = {}
        for graph in (False, True):
            env, runner, first[graph], sls[(coef, graph)] = _train_arm(monkeypatch, coef, graph, ITERS if (graph and coef) else 1)
            alg = runner.alg
            if graph:
                assert alg.graphs_captured() or not coef          # (the first update runs eagerly: the one-iteration arm has not captured yet)
                assert alg._acc.numel() == (3 if coef else 2) and (alg._sw_all is not None) == bool(coef)
                assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
            env.close()
            del env, runner, alg          # (their HIP graphs, streams and events: collected here, with the device idle)
            torch.cuda.synchronize()
            gc.collect()
        graph_weights[coef] = first[True]
        gaps[coef] = {n: float(np.median(np.abs(first[True][n] - first[False][n]))) for n in first[True]}
        print("[smooth loss, coef %s] graph vs eager after iteration 1: largest per-tensor median gap %.2e (%s); alg.smooth_loss eager %.6e, graph %.6e"
              % (coef, max(gaps[coef].values()), max(gaps[coef], key=gaps[coef].get), sls[(coef, False)], sls[(coef, True)]))
    for n in gaps[0.5]:
        print("[smooth loss] %s: median gap with the coefficient on %.3e, with 0 %.3e" % (n, gaps[0.5][n], gaps[0.0][n]))
    for n in gaps[0.5]:
        assert gaps[0.5][n] <= 2.0 * gaps[0.0][n] + GAP1_MED, (n, gaps[0.5][n], gaps[0.0][n])
    e, g = sls[(0.5, False)], sls[(0.5, True)]
    assert e > 0 and abs(g - e) <= 1e-5 * e, (e, g)
    assert sls[(0.0, False)] == 0.0 and sls[(0.0, True)] == 0.0
    last = [n for n in graph_weights[0.5] if n.startswith("actor.") and n.endswith(".weight")][-1]
    assert float(np.median(np.abs(graph_weights[0.5][last] - graph_weights[0.0][last]))) > 1e-5


def test_term_lowers_what_it_penalises_on_gpu(hip, nn):
    """tests/test_smooth_loss_host.py::test_term_lowers_what_it_penalises through the captured device path (go2nn_smooth_indices in the permutation step, go2nn_smooth_loss
    behind go2nn_ppo_heads)"""
    alg = sh.check_term_lowers_the_loss(DEV, hip, "graph mode on the device")
    assert alg.use_graphs and alg._acc.numel() == 3 and alg._sw_all is not None and alg.graphs_captured()


# ---- the combinations, captured ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["normalisers+diagnostics", "mirror+sensors+collectives"])
def test_combinations_replay_captured_on_gpu(hip, nn, monkeypatch, combo):
    """go2_flat at 64 envs, four iterations in graph mode with the term next to (a) observation normalisation, value normalisation and the diagnostics, (b) symmetry
    augmentation (two blocks), the mirror loss and randomised sensors in the multi-rank step shape (a 1-rank RCCL group, GO2_FORCE_COLLECTIVES=1): every step is replayed
    from its graph, the weights are finite and both reported losses positive."""
    import socket
    import torch
    import torch.distributed as dist
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    forced = combo.endswith("collectives")
    flags = ["--mirror_loss", "0.5"] if forced else ["--normalize_obs", "--normalize_value", "--diagnostics"]
    if forced:
        monkeypatch.setenv("GO2_FORCE_COLLECTIVES", "1")
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        args = get_args(["--task", "go2_flat", "--num_envs", "64", "--headless", "--seed", "3", "--smooth_loss", "0.25", *flags])
        env_cfg, _ = task_registry.get_cfgs("go2_flat")
        env_cfg.domain_rand.randomize_sensors = forced
        env, _ = task_registry.make_env("go2_flat", args, env_cfg=env_cfg)
        torch.manual_seed(3)
        runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
        runner.learn(4, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        alg = runner.alg
        assert alg.use_graphs and alg.graphs_captured() and alg._acc.numel() == (4 if forced else 3)
        assert np.isfinite(alg.smooth_loss) and alg.smooth_loss > 0.0 and all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
        if forced:
            assert alg.mirror_loss > 0.0 and alg._aug is not None
        else:
            assert alg.diagnostics
        env.close()
    finally:
        if forced:
            dist.destroy_process_group()
