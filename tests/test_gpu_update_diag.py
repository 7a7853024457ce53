"""The update's diagnostics on the device (`algorithm.diagnostics`): go2nn_ppo_diag against float64 at the shapes and with the rule of tests/test_update_diag_host.py,
also from inside a captured and twice-replayed graph; go2nn_grad_sqnorm; go2_flat and go2_flat_cts through the product path with the key off and on (bit-identical
weights, captured graphs, step-0 ratios of 1); graph mode against the eager mode per slot.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_update_diag_host as dh  # noqa: E402
from test_gpu_parity import GAP1_MED  # noqa: E402
from go2_rl_gym_amd import _nn  # noqa: E402
from go2_rl_gym_amd.rsl_rl.algorithms import _diag  # noqa: E402

DEV = "cuda:0"
COL = _diag.COL


@pytest.fixture(scope="module")
def nn():
    lib = _nn.load_nn()
    assert lib.go2nn_is_device_library() == 1
    return lib


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the kernel against float64, plain and from a replayed graph ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(7))
def test_kernel_on_gpu_matches_float64(nn, i):
    import torch
    B, A, K, split = dh.shapes(nn)[i]
    c = dh.make_case(B, A, K, split)
    call = dh.DiagCall(nn, c, DEV)
    assert call(stream=_stream()) == 0, nn.go2nn_last_error()
    torch.cuda.synchronize()
    assert int(call.cursor.cpu()[0]) == 1 and bool((call.partials[-8:] == dh.SENT).all()) and bool((call.table[call.segs * dh.NUM:] == dh.SENT).all())
    dh.check_against_float64(call.slot(0), c, "device, B %d A %d K %d split %d" % (B, A, K, split), DEV)
    again = dh.DiagCall(nn, c, DEV)
    assert again(stream=_stream()) == 0
    torch.cuda.synchronize()
    assert again.bits() == call.bits()          # fixed order: two launches give the same bits


@pytest.mark.parametrize("i", range(7))
def test_captured_pair_advances_the_slot_on_every_replay(nn, i):
    """the two launches captured ONCE, replayed twice with other inputs in the same buffers: slots 0 and 1 hold their inputs' rows, the cursor reads 2"""
    import torch
    B, A, K, split = dh.shapes(nn)[i]
    cases = [dh.make_case(B, A, K, split, seed=s) for s in (0, 1)]
    call = dh.DiagCall(nn, cases[0], DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # (a warm-up call outside the capture, as CapturedStep does)
        assert call(stream=C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    call.cursor.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call(stream=_stream()) == 0
    for c in cases:
        for k in dh.DiagCall.KEYS:
            call.t[k].copy_(torch.from_numpy(c[k]))
        g.replay()
    torch.cuda.synchronize()
    assert int(call.cursor.cpu()[0]) == 2
    for s, c in enumerate(cases):
        dh.check_against_float64(call.slot(s), c, "device, replay %d, B %d" % (s, B), DEV)
    assert not np.array_equal(call.slot(0), call.slot(1)) and bool((call.table[2 * call.segs * dh.NUM:] == dh.SENT).all())


def test_refusals_on_gpu_write_nothing(nn):
    import torch
    B, A, K, split = dh.shapes(nn)[4]
    call = dh.DiagCall(nn, dh.make_case(B, A, K, split), DEV)
    clean = call.bits()
    for kw in (dict(B=0), dict(A=17), dict(K=126), dict(surrogate_split=B), dict(slots=0), dict(table=None), dict(cursor=None), dict(y_a=None)):
        assert call(patch=lambda d, kw=kw: [setattr(d, k, v) for k, v in kw.items()], stream=_stream()) == dh.GO2NN_EINVAL
    torch.cuda.synchronize()
    assert call.bits() == clean
    call.cursor.fill_(3)          # a full table: the launches run, the pass leaves its partial rows, the table and the cursor stay
    table = call.table.cpu().numpy().tobytes()
    assert call(stream=_stream()) == 0
    torch.cuda.synchronize()
    assert call.table.cpu().numpy().tobytes() == table and int(call.cursor.cpu()[0]) == 3 and bool((call.table == dh.SENT).all())


# ---- 2. go2nn_grad_sqnorm ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 48])
def test_grad_sqnorm_on_gpu_matches_float64(nn, count):
    arrays = dh.grad_case(count)
    rcs, out, part, cur, _ = dh.run_grad_sqnorm(nn, arrays, DEV, stream=_stream())
    want = sum(float((a.astype(np.float64) ** 2).sum()) for a in arrays)
    print("[update diag, grad sqnorm, device] %d tensors: %.15e against float64 %.15e (relative gap %.2e)" % (count, out[0], want, abs(out[0] - want) / want))
    assert rcs == [0, 0] and cur == 2 and abs(out[0] - want) <= 1e-9 * want
    assert out[0].tobytes() == out[1].tobytes() and out[2] == dh.SENT and (part[-8:] == dh.SENT).all()


# ---- 3 / 4. the product path ----------------------------------------------------------------------------------------------------------------------------------
N_ENVS = 64


def train_arm(mp, task, graph, key, iters):
    """One arm of `task` at 64 envs x 24 steps through the product path, pinned as tests/test_gpu_symmetry.py:_train_arm pins its arms — the same seed and initial weights,
    a fixed learning rate, the exploration noise from one pre-drawn buffer, ONE fixed permutation (PPO; the CTS update's is keyed by the seed) — with the task's own
    clip.  -> dict(weights per iteration, tables per iteration, alg, boundary rows per slot of the first update (eager arms))"""
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic import ActorCritic
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic_cts import ActorCriticCTS
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", task, "--num_envs", str(N_ENVS), "--headless", "--seed", "3"] + (["--diagnostics"] if key else []))
    env, _ = task_registry.make_env(task, args)
    torch.manual_seed(3)
    _, train_cfg = task_registry.get_cfgs(task)
    keep = train_cfg.algorithm.schedule
    train_cfg.algorithm.schedule = "fixed"
    try:
        runner, _ = task_registry.make_alg_runner(env, task, args, train_cfg=train_cfg, log_root=None, use_graphs=graph)
    finally:
        train_cfg.algorithm.schedule = keep
        if key:
            train_cfg.algorithm.diagnostics = False
    alg = runner.alg
    assert alg.use_graphs == graph and (alg._diag is not None) == key and alg.fused_loss and alg.fused_rollout and alg.clip_param == 0.2
    T, A = alg.storage.num_transitions_per_env, alg.storage.actions.shape[-1]
    gen, buf, calls = torch.Generator().manual_seed(17), torch.zeros(T, N_ENVS, A, device=alg.device), [0]

    def noise(self_, like):
        row = buf[calls[0] % T]; calls[0] += 1
        assert row.shape == like.shape
        return row
    cts = task.endswith("cts")
    mp.setattr(ActorCriticCTS if cts else ActorCritic, "_noise", noise)
    if not cts:
        perm = torch.randperm(N_ENVS * T, generator=torch.Generator().manual_seed(23)).to(alg.device)
        mp.setattr(torch, "randperm", lambda n, **kw: perm)
    boundary, vboundary, real_terms = [], [], _diag.diag_terms_torch
    if key and not graph:          # the eager arm's own fp32 rows: per slot and segment, the rows within 1e-4 of a count's threshold (the ratio's, the value step's)
        split = alg._teacher_rows() if cts else 0

        def counting(*a):
            t = real_terms(*a)
            rho, dv, clip = t[:, COL["ratio_max"]], (a[2].detach().float().reshape(-1) - a[8].detach().float().reshape(-1)), a[-1]
            segs = [(0, len(rho))] if not split else [(0, split), (split, len(rho))]
            boundary.append([int((((rho[lo:hi] - 1.0).abs() - clip).abs() < 1e-4).sum()) for lo, hi in segs])
            vboundary.append([int(((dv[lo:hi].abs() - clip).abs() < 1e-4).sum()) for lo, hi in segs])
            return t
        mp.setattr(_diag, "diag_terms_torch", counting)
    if cts and not graph:
        # the eager CTS arm draws its mini-batches with the keyed device-side permutation the graph arm's update head uses, under the same key (tests/test_gpu_parity.py)
        import ctypes
        from helpers import load_hip
        hip, st = load_hip(), alg.storage
        skey = torch.tensor([int((torch.initial_seed() * 0x9E3779B1 + 0x7F4A7C15) & 0x7FFFFFFF), 0, 0, 0], dtype=torch.int32, device=alg.device)
        order = torch.empty(N_ENVS * T, dtype=torch.int64, device=alg.device)

        def keyed(nmb):
            nt, ns = st.teacher_num_envs * T, st.student_num_envs * T
            rc = hip.go2sim_cts_minibatch_indices(ctypes.c_void_p(order.data_ptr()), nmb, nt, ns, ctypes.c_void_p(st.ref2mine.data_ptr()), ctypes.c_void_p(skey.data_ptr()),
                                                  ctypes.c_void_p(torch.cuda.current_stream(alg.device).cuda_stream))
            assert rc == 0, hip.go2sim_last_error().decode()
            rows = nt // nmb + ns // nmb
            return [order[i * rows:(i + 1) * rows].clone() for i in range(nmb)]
        st.mini_batch_indices = keyed
    env.common_step_counter = 0
    out = dict(weights=[], tables=[], grad_sq=[], alg=alg, boundary=boundary, vboundary=vboundary)
    for it in range(iters):
        buf.copy_(torch.randn(buf.shape, generator=gen))
        runner.learn(1, init_at_random_ep_len=(it == 0))
        out["weights"].append({n: p.detach().cpu().numpy().copy() for n, p in alg.actor_critic.named_parameters()})
        if key:
            out["tables"].append(alg.diagnostics_table.copy()); out["grad_sq"].append(alg.diagnostics_grad_sq.copy())
    torch.cuda.synchronize()
    out["captured"] = bool(alg.graphs_captured()) if graph else None
    out["logp_min"], out["actions"] = float(alg.storage.actions_log_prob.abs().min()), A          # (the last rollout's rows: clear() leaves them)
    out["figures"] = alg.diagnostics
    mp.undo()
    env.close()
    return out


@pytest.fixture(scope="module")
def arms():
    """every arm once: (task, graph mode, key) -> train_arm's result; graph arms run three iterations (the update's warm-up call, its capture, and the third, by which the
    permutation step with its two warm-up calls is captured too), eager arms one"""
    mp = pytest.MonkeyPatch()
    cache = {}

    def get(task, graph, key):
        if (task, graph, key) not in cache:
            cache[(task, graph, key)] = train_arm(mp, task, graph, key, 3 if graph else 1)
        return cache[(task, graph, key)]
    yield get
    mp.undo()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_key_on_leaves_graph_mode_training_bit_identical(arms, task):
    """Three iterations in graph mode (the last replays every captured step) with the key off and on: every weight bit-identical after each, graphs captured, the
    tables finite, step 0 of each update reads the rollout's own policy (ratios of 1 within 1e-5), and the clip fraction does not fall from the first epoch to the last."""
    off, on = arms(task, True, False), arms(task, True, True)
    assert off["captured"] and on["captured"]
    for it in range(3):
        for n in off["weights"][it]:
            assert off["weights"][it][n].tobytes() == on["weights"][it][n].tobytes(), (it, n)
    alg = on["alg"]
    segs = 1 if task == "go2_flat" else 2
    for it, (tab, gsq) in enumerate(zip(on["tables"], on["grad_sq"])):
        assert tab.shape == (alg.num_learning_epochs * alg.num_mini_batches, segs, dh.NUM) and gsq.shape == (tab.shape[0], segs)
        assert np.isfinite(tab).all() and np.isfinite(gsq).all() and (gsq > 0).all() and (tab[..., COL["rows"]] > 0).all()
        step0 = _diag.pool_rows(tab[0])
        print("[update diag, %s, iteration %d] step 0 ratio in [%.8f, %.8f]; clip fraction per step %s" % (task, it, step0[COL["ratio_min"]], step0[COL["ratio_max"]],
              np.round(tab[..., COL["ratio_clipped"]].sum(-1) / tab[..., COL["rows"]].sum(-1), 4).tolist()))
        assert abs(step0[COL["ratio_max"]] - 1.0) <= 1e-5 and abs(step0[COL["ratio_min"]] - 1.0) <= 1e-5
    d = on["figures"] if segs == 1 else on["figures"]["all"]
    assert d["clip_fraction/last_epoch"] >= d["clip_fraction/first_epoch"] and d["grad_norm"] > 0
    assert alg._diag._partials is not None and all(p is not None for p in alg._diag._gpart)          # the kernels ran, not the torch statement


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_graph_mode_tables_match_the_eager_mode_per_slot(arms, task):
    """Iteration 1, graph mode (go2nn_ppo_diag) against the eager mode (the torch statement) slot by slot and segment by segment.  ROWS and ADV_POS are equal.
    RATIO_CLIPPED may differ by at most the segment's rows whose eager fp32 ratio lies within 1e-4 of the clip boundary, VALUE_CLIPPED by at most those whose eager
    |v - old value| lies within 1e-4 of the clip; both are counted here per slot and printed, and are at most 1 % of the slot's rows.  Sum columns differ by at most
    (4 x the key-off graph-vs-eager weight gap of this run + GAP1_MED) x the column's magnitude (its own absolute value, at least one unit per row).  An extremum column
    is ONE row's fp32 value: no sum averages its rounding, so on top of that rule it gets the floor of the kernel-vs-float64 test, 1e-6 x the magnitude of the term's
    fp32 operands, taken at a lower bound that needs no per-row data — kl: 1 / 2 per action (one of its addends); the ratio: rho x the smallest |old log-prob| of the
    rollout (rho = exp(lp - old lp)); |returns - v|: half of itself (the larger of |returns| and |v| is at least that)."""
    g_off, e_off, g_on, e_on = arms(task, True, False), arms(task, False, False), arms(task, True, True), arms(task, False, True)
    wgap = max(float(np.median(np.abs(g_off["weights"][0][n] - e_off["weights"][0][n]))) for n in g_off["weights"][0])
    g, e, boundary, vboundary = g_on["tables"][0], e_on["tables"][0], np.asarray(e_on["boundary"]), np.asarray(e_on["vboundary"])
    rows = e[..., COL["rows"]]
    print("[update diag, graph vs eager on the device, %s] key-off weight gap (largest per-tensor median) %.2e; rows per segment %s; ratio-boundary rows per slot %s; "
          "value-boundary rows per slot %s; smallest |old log-prob| %.2f" % (task, wgap, rows[0].astype(int).tolist(), boundary.tolist(), vboundary.tolist(), e_on["logp_min"]))
    assert g.shape == e.shape and boundary.shape == vboundary.shape == rows.shape and np.array_equal(g[..., COL["rows"]], rows)
    assert (boundary.sum(1) <= 0.01 * rows.sum(1)).all() and (vboundary.sum(1) <= 0.01 * rows.sum(1)).all()
    assert np.array_equal(g[..., COL["adv_pos"]], e[..., COL["adv_pos"]])
    for k, allowed in (("ratio_clipped", boundary), ("value_clipped", vboundary)):
        gap = np.abs(g[..., COL[k]] - e[..., COL[k]])
        print("[update diag, graph vs eager on the device, %s] %-14s eager counts %s, largest difference %d" % (task, k, e[..., COL[k]].astype(int).tolist(), int(gap.max())))
        assert (gap <= allowed).all(), (k, gap, allowed)
    assert e[..., COL["ratio_clipped"]].sum() > 0 and e[..., COL["value_clipped"]].sum() > 0          # (the counts are not trivially zero)
    tol = 4.0 * wgap + GAP1_MED
    operands = {"kl_max": 0.5 * e_on["actions"] * np.ones_like(rows), "ratio_max": e[..., COL["ratio_max"]] * max(1.0, e_on["logp_min"]),
                "ratio_min": e[..., COL["ratio_min"]] * max(1.0, e_on["logp_min"]), "verr_abs_max": 0.5 * e[..., COL["verr_abs_max"]]}
    for k, j in COL.items():
        if k in dh.COUNT_COLS:
            continue
        allowed = tol * np.maximum(np.abs(e[..., j]), rows if _diag._KIND[j] == 0 else 1.0) + (1e-6 * operands[k] if k in operands else 0.0)
        gap = np.abs(g[..., j] - e[..., j])
        print("[update diag, graph vs eager on the device, %s] %-14s largest gap / allowed %.3f (gap %.2e)" % (task, k, (gap / allowed).max(), gap.max()))
        assert (gap <= allowed).all(), (k, gap, allowed)
