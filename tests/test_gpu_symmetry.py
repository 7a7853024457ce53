"""Left-right symmetry augmentation on the device (`algorithm.symmetry`): go2nn_mirror_rows against numpy bit for bit, the graph-mode PPO update against the eager
formulation (flag off and on in one run: flag off is the yardstick), the mirror launch inside the captured permutation step, and the invariance of the augmented
mini-batch under mirroring the whole rollout.  Run with -m gpu."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
from test_symmetry_host import GO2NN_EINVAL, SENTINEL, SHAPES, fill_storage, mirror_case, mirror_expected  # noqa: E402
from test_gpu_parity import CLIP_OFF, GAP1_MED  # noqa: E402
from go2_rl_gym_amd import _nn  # noqa: E402
from go2_rl_gym_amd.envs.go2.go2_config import GO2Cfg  # noqa: E402
from go2_rl_gym_amd.utils.symmetry import mirror_rows, mirror_tables  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1
    return lib


@pytest.fixture(scope="module")
def nn():
    return _nn.load_nn()


@pytest.fixture(scope="module")
def tables():
    return mirror_tables(GO2Cfg())


def _device_jobs(nn, jobs, dev="cuda:0"):
    """-> (pairs for _nn.mirror_jobs, the padded destination buffers): every dst is followed by SENTINEL floats of 7.25"""
    import torch
    pairs, bufs = [], []
    for src, tab in jobs:
        s = torch.from_numpy(src).to(dev)
        buf = torch.full((2 * src.size + SENTINEL,), 7.25, device=dev)
        pairs.append((s, buf[:2 * src.size].view(2 * src.shape[0], src.shape[1]), None if tab is None else _nn.mirror_table_tensors(nn, tab, dev)))
        bufs.append(buf)
    return pairs, bufs


@pytest.mark.parametrize("chunks,chunk_rows", SHAPES)
def test_mirror_rows_on_gpu_is_numpy_bit_for_bit(nn, tables, chunks, chunk_rows):
    import torch
    jobs = mirror_case(chunks, chunk_rows, tables)
    pairs, bufs = _device_jobs(nn, jobs)
    _nn.mirror_rows(nn, _nn.mirror_jobs(pairs), chunks, chunk_rows, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for (src, tab), buf in zip(jobs, bufs):
        got = buf.cpu().numpy()
        want = mirror_expected(src, tab, chunks, chunk_rows).reshape(-1)
        assert np.array_equal(got[:-SENTINEL].view(np.uint32), want.view(np.uint32))          # the BITS: -0.0 and denormals included
        assert (got[-SENTINEL:] == 7.25).all()


def test_mirror_rows_on_gpu_refuses_bad_arguments_and_writes_nothing(nn, tables):
    import torch
    src = np.ones((6, 12), np.float32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(n_jobs=None, chunks=2, chunk_rows=3, patch=None, count=2):
        pairs, bufs = _device_jobs(nn, [(src, tables.action)] * count)
        arr = _nn.mirror_jobs(pairs)
        if patch:
            patch(arr)
        assert nn.go2nn_mirror_rows(arr, count if n_jobs is None else n_jobs, chunks, chunk_rows, stream) == GO2NN_EINVAL and nn.go2nn_last_error().decode() != ""
        torch.cuda.synchronize()
        assert all(bool((b == 7.25).all()) for b in bufs)

    assert nn.go2nn_mirror_rows(None, 1, 2, 3, stream) == GO2NN_EINVAL
    refused(n_jobs=0)
    refused(n_jobs=17)
    refused(chunks=0)
    refused(chunk_rows=0)
    refused(chunk_rows=-3)
    refused(patch=lambda a: setattr(a[1], "src", None))
    refused(patch=lambda a: setattr(a[1], "dst", None))
    refused(patch=lambda a: setattr(a[1], "width", 0))
    refused(patch=lambda a: setattr(a[1], "perm", None))
    refused(patch=lambda a: setattr(a[1], "sign", None))
    # an index outside the row cannot be reported by the launch: the table is refused on the host, before the upload
    perm, sign = tables.action
    for bad in (12, -1):
        p = perm.copy(); p[7] = bad
        with pytest.raises(ValueError, match="perm"):
            _nn.mirror_table_tensors(nn, (p, sign), "cuda:0")


# ---- graph mode against the eager formulation ---------------------------------------------------------------------------------------------------------------
N_ENVS, ITERS = 64, 3


def _train_arm(monkeypatch, symmetry, graph, iters):
    """One arm of go2_flat at 64 envs x 24 steps through the product path, pinned the way tests/test_gpu_parity.py pins its graph-vs-eager arms: the same seed and initial
    weights, a fixed learning rate, the smooth objective (CLIP_OFF), the exploration noise from one pre-drawn buffer and ONE fixed permutation for every update."""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic import ActorCritic
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", str(N_ENVS), "--headless", "--seed", "3"])
    env, _ = task_registry.make_env("go2_flat", args)
    torch.manual_seed(3)
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    keep = (train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param, train_cfg.algorithm.symmetry)
    train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param, train_cfg.algorithm.symmetry = "fixed", CLIP_OFF, symmetry
    try:
        runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, train_cfg=train_cfg, log_root=None, use_graphs=graph)
    finally:
        train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param, train_cfg.algorithm.symmetry = keep
    alg = runner.alg
    assert alg.use_graphs == graph and (alg._sym is not None) == symmetry and alg.fused_loss and alg.fused_rollout
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
    first = None
    for it in range(iters):
        buf.copy_(torch.randn(buf.shape, generator=gen))
        runner.learn(1, init_at_random_ep_len=(it == 0))
        if it == 0:
            first = {n: p.detach().cpu().numpy().copy() for n, p in alg.actor_critic.named_parameters()}
    torch.cuda.synchronize()
    return env, runner, first, perm


def test_graph_mode_matches_the_eager_formulation_with_the_flag_off_and_on(hip, nn, tables, monkeypatch):
    """After iteration 1 (20 Adam steps of 1e-3 from the same weights on the same rollout in the same order) the per-tensor gap between graph mode and the eager
    formulation with the flag ON is at most twice the gap with the flag OFF measured in this same run (flag off is the code as it was: the yardstick; the factor 2 is
    for sums over twice the rows), plus the floor of tests/test_gpu_parity.py (GAP1_MED).  Graph mode with the flag on is captured, stays finite over three
    iterations, and its mirror launch sits inside the captured permutation step: a replay after the storage changed fills _aug like a fresh eager build."""
    import torch
    gaps, graph_weights = {}, {}
    for symmetry in (False, True):
        first = {}
        for graph in (False, True):
            env, runner, first[graph], perm = _train_arm(monkeypatch, symmetry, graph, ITERS if (graph and symmetry) else 1)
            alg = runner.alg
            if graph and symmetry:
                assert alg.graphs_captured() and alg._permute.graph is not None and alg._aug is not None
                assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
                st, mb, nmb = alg.storage, alg._mb, alg.num_mini_batches
                assert alg._aug["obs"].shape == (nmb, 2 * mb, 45) and alg._aug["cobs"].shape == (nmb, 2 * mb, 263) and alg._aug["logp"].shape == (nmb, 2 * mb, 1)
                fill_storage_device(alg, 41)
                before = alg._aug["obs"].clone()
                alg._permute()          # a REPLAY of the captured step: gather + mirror
                torch.cuda.synchronize()
                assert not torch.equal(before, alg._aug["obs"])
                for k in alg._KEYS:
                    x = alg._flat[k][perm].reshape((nmb, mb) + tuple(alg._flat[k].shape[1:])).cpu().numpy()
                    tab = alg._sym_table(k)
                    want = np.concatenate([x, x if tab is None else mirror_rows(x, tab)], 1)
                    assert np.array_equal(alg._aug[k].cpu().numpy().view(np.uint32), want.view(np.uint32)), k
            elif graph:
                assert alg._aug is None and alg._sym is None
            env.close()
            del env, runner, alg          # (their HIP graphs, streams and events: collected here, with the device idle, not in the middle of the next arm's replay)
            torch.cuda.synchronize()
            gc.collect()
        graph_weights[symmetry] = first[True]
        gaps[symmetry] = {n: float(np.median(np.abs(first[True][n] - first[False][n]))) for n in first[True]}
        peak = {n: float(np.abs(first[True][n] - first[False][n]).max()) for n in first[True]}
        print("[symmetry %s] graph vs eager after iteration 1: largest per-tensor median gap %.2e (%s), largest element gap %.2e"
              % ("on" if symmetry else "off", max(gaps[symmetry].values()), max(gaps[symmetry], key=gaps[symmetry].get), max(peak.values())))
    for n in gaps[True]:
        assert gaps[True][n] <= 2.0 * gaps[False][n] + GAP1_MED, (n, gaps[True][n], gaps[False][n])
    # the flag does something: the two settings have trained on different mini-batches (20 Adam steps of 1e-3 each)
    assert max(float(np.median(np.abs(graph_weights[True][n] - graph_weights[False][n]))) for n in graph_weights[True]) > 1e-4


def fill_storage_device(alg, seed):
    """new contents for the rollout tensors the update reads (the addresses stay: the captured steps read them in place)"""
    import torch
    st = alg.storage
    g = torch.Generator().manual_seed(seed)
    for k in ("observations", "privileged_observations", "actions", "mu", "values", "returns", "advantages", "actions_log_prob"):
        t = getattr(st, k)
        t.copy_(torch.randn(t.shape, generator=g))
    st.sigma.copy_(0.5 + torch.rand(st.sigma.shape, generator=g))


# ---- the storage-mirroring invariance on the device path ------------------------------------------------------------------------------------------------------
def test_mirrored_storage_gives_the_same_minibatch_gradients_on_gpu(hip, nn, tables, monkeypatch):
    """tests/test_symmetry_host.py::test_mirrored_storage_gives_the_same_first_minibatch through the device path (go2sim_shuffle_gather, go2nn_mirror_rows, the
    no-autograd mini-batch): ONE mini-batch of 16 x 24 rows at learning rate 0, so the update leaves the weights alone and every parameter's .grad is that mini-batch's
    gradient.  The augmented mini-batch of the mirrored rollout is the same multiset of rows in another order: same loss sums and gradients within fp32 summation
    order — the bounds of the host test (2e-6 on the loss terms: means over 768 rows of terms of size ~0.3, i.e. ~100 ulp of the result; 2e-7 + 2e-4 relative on the
    gradients)."""
    import torch
    from go2_rl_gym_amd.rsl_rl.algorithms import PPO
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    N, T = 16, 24
    perm = torch.randperm(N * T, generator=torch.Generator().manual_seed(5)).to("cuda:0")
    monkeypatch.setattr(torch, "randperm", lambda n, **kw: perm)
    res = []
    for mirrored in (False, True):
        torch.manual_seed(0)
        ac = ActorCritic(45, 263, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=0.8)
        alg = PPO(ac, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=0.0, max_grad_norm=1e9,
                  use_clipped_value_loss=True, schedule="fixed", device="cuda:0", lib=hip, symmetry=tables)
        alg.init_storage(N, T, [45], [263], [12])
        w0 = torch.cat([p.detach().reshape(-1) for p in ac.parameters()]).clone()
        fill_storage(alg, 3, tables if mirrored else None, scale=0.3)
        value_loss, surrogate_loss = alg.update()
        torch.cuda.synchronize()
        assert alg.use_graphs and alg._aug is not None and alg._aug["obs"].shape == (1, 2 * N * T, 45)
        assert torch.equal(w0, torch.cat([p.detach().reshape(-1) for p in ac.parameters()]))
        res.append(((value_loss, surrogate_loss), {n: p.grad.detach().cpu().numpy().copy() for n, p in ac.named_parameters()}, alg._aug["obs"][0].cpu()))
    (l0, g0, o0), (l1, g1, o1) = res
    B = N * T
    assert torch.equal(o0[:B], o1[B:]) and torch.equal(o0[B:], o1[:B]) and not torch.equal(o0[:B], o0[B:])
    print("[symmetry] mirrored rollout on the device path: loss terms %s / %s; largest gradient gap %.2e" % (l0, l1, max(float(np.abs(g0[n] - g1[n]).max()) for n in g0)))
    assert all(abs(a - b) < 2e-6 for a, b in zip(l0, l1)), (l0, l1)
    assert all(np.abs(g).max() > 0 for g in g0.values())
    for n in g0:
        np.testing.assert_allclose(g1[n], g0[n], atol=2e-7, rtol=2e-4, err_msg=n)
