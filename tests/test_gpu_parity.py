"""Parity tests proper: the HIP library on a real MI355X against the oracle, the reference's golden vectors and
size-independent properties.  Everything goes through the C ABI (include/go2sim.h).  Run with -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import ROOT, STEP_STATE, DeviceSim, HostSim, load_hip, load_oracle  # noqa: E402
import test_oracle_golden as tg  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.mark.parametrize("terrain", tg.SEQUENCES)
def test_golden_sequence_on_gpu(hip, terrain):
    """post_physics_step of the reference (golden vectors, injected uniforms) reproduced by the HIP kernel:
    obs / priv obs <= 2e-5, rewards <= 2e-6 (fp32, tolerances in test_oracle_golden.TOL).  heightfield: + the 187-point
    height scan, terrain curriculum and per-terrain-kind command ranges; control_v / control_t:
    the other two control types of _compute_torques; cmd_curriculum: commands.curriculum across a command_range_curriculum stage start.  Each
    sequence ends with a reset_idx(subset) from outside a step (go2sim_reset_idx) against the reference's."""
    g = dict(np.load(os.path.join(G, "go2_%s_sequence.npz" % terrain)))
    s = tg._mk(hip, g, sim=DeviceSim)
    n = 0
    def check(name, t_, got, want):      # torques of all 4 substeps from the kernel's own pd() + delay select vs the reference's (2e-5)
        np.testing.assert_allclose(got, want, atol=tg.TOL[name], rtol=1e-5, err_msg="%s at step %d" % (name, t_))
    for t in tg.run_sequence(s, hip, g, check):
        s.torch.cuda.synchronize()
        tg.compare_step(s, g, t)
        n += 1
    assert n == g["actions"].shape[0]
    tg.compare_reset_idx(s, g)
    s.close()


def test_strict_ops_on_gpu(hip):
    """The individually rounded fp32 operations under the height-scan index arithmetic equal IEEE on the device build (-ffast-math)."""
    tg.check_strict_ops(hip, "cuda:0")


def test_reset_all_golden_on_gpu(hip):
    g = dict(np.load(os.path.join(G, "go2_plane_sequence.npz")))
    s = DeviceSim(hip, num_envs=g["actions"].shape[1])
    hip.go2sim_set_common_step_counter(s.h, int(g["start_counter"]))
    s.inject(g["U_reset_all"]); s.reset_all(); s.torch.cuda.synchronize()
    np.testing.assert_allclose(s.root_states, g["reset_all_root"], atol=1e-6)
    np.testing.assert_allclose(s.dof_state, g["reset_all_dof"], atol=1e-6)
    np.testing.assert_allclose(s.commands, g["reset_all_commands"], atol=1e-6)
    s.close()


def test_one_step_parity_vs_oracle(hip):
    """Each step starts from the oracle's state: 4 substeps (PD, dynamics, contact PGS) + post-physics on the GPU vs the independent CPU
    derivation.  ONE fp32 bound per tensor for every env of every step (helpers.PLANE_BOUND, round 4: root 3e-4, dof 5e-3, torque 3e-3, obs 3e-4,
    reward 2e-5) and a 10x tighter one for 99 % of them — the size of the fp32 oracle's own error against the fp64 oracle on the same
    inputs (profiles/r2_parity_probe.txt).
    This is go2sim_default_cfg only (4 substeps, 8 sweeps, no armature, vertical gravity; hardly an env-step at a joint stop, none at the twist clamp): the other
    settings and those rows are in tests/test_gpu_step_configs.py (cases and gates: tests/step_config_cases.py)."""
    from helpers import PLANE_BOUND, StepErrors, check_plane_errors, ill_conditioned_envs
    N = 64
    so = HostSim(load_oracle(), num_envs=N)
    s64 = HostSim(load_oracle(f64=True), num_envs=N)      # the fp64 oracle from the same state: tells an ill-conditioned step from an error
    sd = DeviceSim(hip, num_envs=N)
    np.testing.assert_array_equal(so.peek(), sd.peek())
    so.reset_all(); sd.reset_all(); s64.reset_all()
    rng = np.random.default_rng(0)
    contact_seen = 0
    err = StepErrors(PLANE_BOUND)
    for it in range(100):
        a = rng.normal(0, 1, (N, 12)).astype(np.float32)
        for k in STEP_STATE:
            v = np.asarray(getattr(so, k))
            getattr(sd, k)[...] = v; getattr(s64, k)[...] = v
        so.step(a); sd.step(a); s64.step(a.astype(np.float64))
        contact_seen += int((so.contact_forces[:, [6, 10, 14, 18], 2] > 1).sum())
        err.add(so, sd, N, ref64=s64)
        ok = ~ill_conditioned_envs(so, s64)
        fo, fd = np.asarray(so.contact_forces, np.float64)[ok], np.asarray(sd.contact_forces, np.float64)[ok]
        de = np.abs(fo - fd).reshape(int(ok.sum()), -1).max(1)
        assert np.median(de) < 5e-3 and de.max() < 2e-3 * max(1.0, np.abs(fo).max()) + 0.5, (it, np.sort(de)[-3:])      # forces are impulse / 5 ms: fp32 noise x200
        np.testing.assert_array_equal(np.asarray(so.reset_buf), np.asarray(sd.reset_buf))
        # feet rows of rigid_body_states (pos, lin vel) - the only rows the reference reads (:1252,1407-1408)
        ro, rd = np.asarray(so.rigid_body_states)[ok][:, [6, 10, 14, 18]][..., [0, 1, 2, 7, 8, 9]], np.asarray(sd.rigid_body_states)[ok][:, [6, 10, 14, 18]][..., [0, 1, 2, 7, 8, 9]]
        assert np.abs(ro - rd).max() < 2e-2, (it, float(np.abs(ro - rd).max()))
    check_plane_errors(err)
    assert contact_seen > 1000
    so.close(); sd.close()


@pytest.mark.parametrize("mesh_type", ["heightfield", "trimesh"])
def test_heightfield_one_step_parity_vs_oracle(hip, mesh_type):
    """Same protocol on the rough curriculum map (all 20 terrain columns): contact against sloped / stepped facets,
    height scan, terrain curriculum.  trimesh: the displaced mesh with its vertical faces (the registered tasks' default mesh type)."""
    from helpers import heightfield_overrides
    N = 80
    t, ov = heightfield_overrides(N, mesh_type=mesh_type)
    from helpers import ROUGH_BOUND, StepErrors, check_relative_to_conditioning, check_rough_errors
    so, s64 = HostSim(load_oracle(), num_envs=N, **ov), HostSim(load_oracle(f64=True), num_envs=N, **ov)
    sd = DeviceSim(hip, num_envs=N, **ov)
    so.reset_all(); sd.reset_all(); s64.reset_all()
    rng = np.random.default_rng(2)
    contact_seen = 0
    floors = {"root_states": 2e-5, "dof_state": 2e-4, "torques": 2e-4, "obs_buf": 2e-5, "privileged_obs_buf": 2e-5, "rew_buf": 2e-7}
    err, cond, abs_err = StepErrors(floors), StepErrors(floors), StepErrors(ROUGH_BOUND, bounds=ROUGH_BOUND)
    for it in range(100):
        a = rng.normal(0, 0.6, (N, 12)).astype(np.float32)
        for k in STEP_STATE:
            v = np.asarray(getattr(so, k))
            getattr(sd, k)[...] = v; getattr(s64, k)[...] = v
        so.step(a); sd.step(a); s64.step(a.astype(np.float64))
        contact_seen += int((so.contact_forces[:, [6, 10, 14, 18], 2] > 1).sum())
        err.add(so, sd, N); cond.add(so, s64, N); abs_err.add(so, sd, N, ref64=s64)
        np.testing.assert_array_equal(np.asarray(so.reset_buf), np.asarray(sd.reset_buf))
        np.testing.assert_array_equal(np.asarray(so.terrain_levels), np.asarray(sd.terrain_levels))
        # the height scan is taken at the pose each library integrated to (1e-5 apart): a point within that of a cell boundary may read the
        # neighbouring cell; the index arithmetic itself is pinned bit-exactly by the golden sequences (test_golden_sequence_on_gpu)
        # (<= 2 of the 14960 samples of a step until round 5; with 8 solver sweeps the two integrated poses are a little further apart — up to 4 samples seen)
        assert (np.abs(np.asarray(so.measured_heights) - np.asarray(sd.measured_heights)) > 1e-6).sum() <= 6
    # a facet edge / stair face under a sphere makes the step ill-conditioned in fp32 for ANY evaluation order: the kernel's error stays
    # within 3x of the fp32 oracle's own error against the fp64 oracle on the same inputs (median, 99th percentile, far tail)
    check_relative_to_conditioning(err, cond, floors)
    # ... and every WELL-conditioned env-step (fp32-vs-fp64 oracle gap below half the bound) meets the plane's absolute per-tensor bound;
    # the ill-conditioned rest is capped at 0.5 % of env-steps (VERDICT r2 "weak" 1)
    check_rough_errors(abs_err)
    assert contact_seen > 2000 and np.abs(np.asarray(so.measured_heights)).max() > 0.05
    so.close(); sd.close(); s64.close()


def test_train_rough_terrain_on_gpu(hip):
    """task=go2 (trimesh -> height field, terrain curriculum, height scan in the privileged obs) through the product path."""
    import tempfile
    import torch
    from go2_rl_gym_amd.envs import task_registry  # noqa: F401
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2", "--num_envs", "400", "--headless", "--max_iterations", "3"])
    env, _ = task_registry.make_env("go2", args)
    assert env.height_samples.shape == (1345, 2195) and env.custom_origins and env.terrain_ids.shape == (400,)
    runner, _ = task_registry.make_alg_runner(env, "go2", args, log_root=tempfile.mkdtemp())
    env.common_step_counter = 0
    runner.learn(3, init_at_random_ep_len=True)
    assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.privileged_obs_buf).all() and runner.last_fps > 0
    assert env.measured_heights.abs().max() > 0.02 and "terrain_level_all" in env.extras["episode"]
    assert any(k.startswith("terrain_level_") and k != "terrain_level_all" for k in env.extras["episode"])
    env.close()


def test_full_size_properties(hip):
    """BASELINE size (4096 envs): finite outputs, determinism (same seed -> bit-identical), different seed -> different,
    physical sanity (robots stand: mean base height, total foot force ~ weight), per-step reward bounded."""
    import torch
    N = 4096
    outs = []
    for seed in (1, 1, 2):
        s = DeviceSim(hip, num_envs=N, seed=seed, push_robots=0)
        s.reset_all()
        a = torch.zeros(N, 12, device="cuda:0")
        for _ in range(60):
            hip.go2sim_step(s.h, C.c_void_p(a.data_ptr()), s._st())
        torch.cuda.synchronize()
        outs.append({k: np.asarray(s.buf[k]).copy() for k in ("obs_buf", "privileged_obs_buf", "root_states", "rew_buf", "contact_forces", "added_base_mass")})
        s.close()
    a, b, c = outs
    for k in a:
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg="non-deterministic " + k)
    assert np.abs(a["obs_buf"] - c["obs_buf"]).max() > 1e-3
    z = a["root_states"][:, 2]
    assert 0.15 < np.median(z) < 0.40
    fz = a["contact_forces"][:, :, 2].sum(1)
    w = (15.019 + a["added_base_mass"]) * 9.81
    assert abs(np.median(fz / w) - 1.0) < 0.15       # standing robots carry their weight
    assert np.abs(a["rew_buf"]).max() < 1.0


def test_gae_kernel_matches_reference(hip):
    import torch
    g = dict(np.load(os.path.join(G, "gae.npz")))
    T, N = g["rewards"].shape
    d = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    rew, dones, val, last = d(g["rewards"]), d(g["dones"]), d(g["values"]), d(g["last_values"])
    ret, adv, part = torch.zeros(T, N, device="cuda:0"), torch.zeros(T, N, device="cuda:0"), torch.zeros(3, dtype=torch.float64, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert hip.go2sim_gae(p(rew), p(dones), p(val), p(last), p(ret), p(adv), p(part), T, N, float(g["gamma"]), float(g["lam"]), st) == 0
    assert hip.go2sim_normalize_advantages(p(adv), p(part), T * N, st) == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(ret.cpu().numpy(), g["returns"], atol=2e-6, rtol=1e-6)
    np.testing.assert_allclose(adv.cpu().numpy(), g["advantages"], atol=2e-5, rtol=1e-5)
    assert part.cpu().numpy()[2] == T * N


def test_train_two_iterations_on_gpu(hip):
    """task=go2_flat through the product path (LeggedRobot -> HIP kernel, OnPolicyRunner -> PPO on PyTorch-ROCm)."""
    import tempfile
    import torch
    from go2_rl_gym_amd.envs import task_registry  # noqa: F401
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", "256", "--headless", "--max_iterations", "2"])
    env, _ = task_registry.make_env("go2_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=tempfile.mkdtemp())
    env.common_step_counter = 0
    runner.learn(2, init_at_random_ep_len=True)
    assert torch.isfinite(env.obs_buf).all() and runner.last_fps > 0
    env.close()


def test_fused_ppo_loss_kernel_on_gpu(hip):
    """go2sim_ppo_loss: HIP kernel vs the oracle on the same inputs at the real mini-batch size (24576 x 12): loss terms, KL and
    the three gradients.  (The oracle itself is pinned against torch autograd in tests/test_ppo_golden.py.)"""
    import torch
    rng = np.random.default_rng(0)
    B, A = 24576, 12
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    mu, std, value, acts = f(B, A), (0.6 + 0.3 * rng.uniform(size=A)).astype(np.float32), f(B), f(B, A)
    old_mu, old_sig = mu + 0.1 * f(B, A), (0.7 + 0.2 * rng.uniform(size=(B, A))).astype(np.float32)
    lp = (-((acts - mu) ** 2) / (2 * std ** 2) - np.log(std) - 0.9189385).sum(1).astype(np.float32)
    old_lp, adv, tv, ret = lp + 0.3 * f(B), f(B), value + 0.3 * f(B), value + f(B)
    ins = [mu, std, value, acts, old_mu, old_sig, old_lp, adv, tv, ret]
    lo = load_oracle()
    res = {}
    for name, lib, dev in (("oracle", lo, "cpu"), ("hip", hip, "cuda:0")):
        t = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in ins]
        gmu, gstd, gval, stats, ws = (torch.zeros(B, A, device=dev), torch.zeros(A, device=dev), torch.zeros(B, device=dev), torch.zeros(5, device=dev), torch.zeros(24 * ((B + 63) // 64), device=dev))
        p = lambda x: C.c_void_p(x.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if dev != "cpu" else None
        assert lib.go2sim_ppo_loss(*[p(x) for x in t], p(gmu), p(gstd), p(gval), p(stats), p(ws), B, A, 0.2, 1.0, 0.01, 1, 0, st) == 0
        if dev != "cpu":
            torch.cuda.synchronize()
        res[name] = [x.cpu().numpy() for x in (gmu, gstd, gval, stats)]
    for a, b, tol in zip(res["oracle"], res["hip"], (2e-8, 2e-6, 2e-9, 2e-5)):
        np.testing.assert_allclose(b, a, atol=tol, rtol=2e-3)


def test_graph_rollout_and_update_match_eager(hip):
    """The HIP-graph execution mode of the runner (rollout replay + captured mini-batch update + fused loss) trains like the
    eager mode: same seeds -> same learning-rate trajectory and near-identical policy after 5 iterations."""
    import tempfile
    import torch
    from go2_rl_gym_amd.envs import task_registry  # noqa: F401
    from go2_rl_gym_amd.utils import get_args
    out = {}
    for mode in (False, True):
        args = get_args(["--task", "go2_flat", "--num_envs", "512", "--headless", "--seed", "3"])
        env, _ = task_registry.make_env("go2_flat", args)
        torch.manual_seed(3)
        runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None, use_graphs=mode)
        assert runner.use_graphs == mode and runner.alg.use_graphs == mode
        env.common_step_counter = 0
        runner.learn(5, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        out[mode] = (runner.alg.learning_rate, torch.cat([p.detach().reshape(-1) for p in runner.alg.actor_critic.parameters()]).cpu().numpy(),
                     env.common_step_counter, float(env.rew_buf.mean()))
        env.close()
    assert out[True][2] == out[False][2] == 5 * 24              # host mirror of the device-resident counter follows the replays
    assert np.isfinite(out[True][1]).all()
    # sampling noise differs between the modes (different RNG consumption), so compare behaviour, not bits
    assert 1.5 ** -8 < out[True][0] / out[False][0] < 1.5 ** 8        # the adaptive rate moves by x1.5 per mini-batch (100 of them); different sampling noise
    assert abs(out[True][3] - out[False][3]) < 0.05


def test_cts_kernels_on_gpu(hip):
    """go2sim_history_push and the split-surrogate loss head: HIP kernels vs numpy / the oracle."""
    import torch
    rng = np.random.default_rng(0)
    N, H, D = 4096, 5, 45
    hist = rng.normal(size=(N, H, D)).astype(np.float32)
    want = hist.copy()
    dh = torch.as_tensor(hist, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for it in range(5):
        obs = rng.normal(size=(N, D)).astype(np.float32)
        dones = (rng.uniform(size=N) < 0.2).astype(np.uint8) if it else None
        if dones is not None:
            want[dones > 0] = 0.0
        want = np.concatenate([want[:, 1:], obs[:, None]], axis=1)
        do, dd = torch.as_tensor(obs, device="cuda:0"), (torch.as_tensor(dones, device="cuda:0") if dones is not None else None)
        assert hip.go2sim_history_push(C.c_void_p(dh.data_ptr()), C.c_void_p(do.data_ptr()), C.c_void_p(dd.data_ptr()) if dd is not None else None, N, H, D, st) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dh.cpu().numpy(), want)
    B, A, split = 24576, 12, 18432
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    mu, std, value, acts = f(B, A), (0.6 + 0.3 * rng.uniform(size=A)).astype(np.float32), f(B), f(B, A)
    old_mu, old_sig = mu + 0.1 * f(B, A), (0.7 + 0.2 * rng.uniform(size=(B, A))).astype(np.float32)
    lp = (-((acts - mu) ** 2) / (2 * std ** 2) - np.log(std) - 0.9189385).sum(1).astype(np.float32)
    ins = [mu, std, value, acts, old_mu, old_sig, lp + 0.3 * f(B), f(B), value + 0.3 * f(B), value + f(B)]
    res = {}
    for name, lib, dev in (("oracle", load_oracle(), "cpu"), ("hip", hip, "cuda:0")):
        t = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in ins]
        gmu, gstd, gval, stats, ws = (torch.zeros(B, A, device=dev), torch.zeros(A, device=dev), torch.zeros(B, device=dev), torch.zeros(5, device=dev), torch.zeros(24 * ((B + 63) // 64), device=dev))
        p = lambda x: C.c_void_p(x.data_ptr())
        assert lib.go2sim_ppo_loss(*[p(x) for x in t], p(gmu), p(gstd), p(gval), p(stats), p(ws), B, A, 0.2, 1.0, 0.01, 1, split, st if dev != "cpu" else None) == 0
        if dev != "cpu":
            torch.cuda.synchronize()
        res[name] = [x.cpu().numpy() for x in (gmu, gstd, gval, stats)]
    for a, b, tol in zip(res["oracle"], res["hip"], (2e-8, 2e-6, 2e-9, 2e-5)):
        np.testing.assert_allclose(b, a, atol=tol, rtol=2e-3)
    # teacher rows weigh 1/split, student rows 1/(B-split): 3x larger gradients per student row at this 75/25 split
    assert abs(np.abs(res["hip"][0][split:]).mean() / np.abs(res["hip"][0][:split]).mean() - 3.0) < 0.5




# The clipped PPO objective is DISCONTINUOUS in the weights: a row whose probability ratio sits on 1 +- clip switches its whole per-row gradient on or off, and one
# row can be several per cent of a mini-batch's gradient (per-row terms mostly cancel).  Round 6's "open finding" (go2_moe_cts graph vs eager 1.2e-4 apart after one
# update; the same on go2_flat_cts as soon as the physics produced other data) was exactly that — tools/debug_cts_gap.py, profiles/r6_cts_gap_clip_boundary.txt: the two
# arms agree to 1e-8 for 19 policy steps, then row 415's ratio is 1.2000013 under the eager arm's weights and 1.1999980 under the graph arm's (advantage +1.7), its
# gradient is dropped by one arm and kept by the other, and each arm's gradient equals the float64 gradient AT ITS OWN WEIGHTS to 1e-6.  So the two formulations are
# compared on the smooth objective (clip far away: both branches of the surrogate and of the value loss coincide); the clip branches themselves are pinned by the
# reference's update fixtures (tests/test_gpu_update_golden.py, tests/test_cts_golden.py).
CLIP_OFF = 1.0e6
GAP1_MED = 2e-6          # measured (round 6): 2.2e-8 / 1.1e-7 / 1.9e-8 — a tensor whose launch is dropped or fed other rows sits at ~1e-3 after one step


# tasks whose algorithm takes the no-autograd mini-batch of modules/fused_cts.py (CTS._own_plan) and the policy kernel; the others (AC-MoE / Dual-MoE heads, the MCP actor)
# keep the autograd formulation, in graph mode as one CapturedStep per mini-batch slot
OWN_PLAN_TASKS = ("go2_flat_cts", "go2_cts", "go2_moe_cts", "go2_flat_moe_cts", "go2_moe_ng_cts")


def _cts_graph_vs_eager(hip, task, monkeypatch, N, ITERS, drift):
    """The body of the two tests below: three arms (eager, eager with reordered mini-batch rows, graph) of `task` at N envs; the bounds after iteration 1 always, the
    drift bounds after iteration ITERS where `drift` (they were measured for the parent test's tasks at 512 envs x 5 iterations only)."""
    import ctypes as C
    import torch
    from go2_rl_gym_amd.envs import task_registry  # noqa: F401
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic_cts import ActorCriticCTS
    from go2_rl_gym_amd.utils import get_args
    out = {}
    # third arm, "reordered": the EAGER formulation once more with the rows of every mini-batch in reverse order (teacher rows and student rows each within their part) —
    # the same sums in another order, i.e. what rounding alone does to the first update on THIS data (one iteration is all it is needed for)
    for arm in ("eager", "reordered", "graph"):
        mode, iters = arm == "graph", (1 if arm == "reordered" else ITERS)
        args = get_args(["--task", task, "--num_envs", str(N), "--headless", "--seed", "3"])
        env, _ = task_registry.make_env(task, args)
        torch.manual_seed(3)
        _, train_cfg = task_registry.get_cfgs(task)
        sched0, clip0 = train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param
        train_cfg.algorithm.schedule = "fixed"      # the adaptive rate at 512 envs is chaotic (x1.5 per mini-batch): compare the two modes at a fixed rate
        train_cfg.algorithm.clip_param = CLIP_OFF   # (see CLIP_OFF)
        try:
            runner, _ = task_registry.make_alg_runner(env, task, args, train_cfg=train_cfg, log_root=None, use_graphs=mode)
        finally:
            train_cfg.algorithm.schedule, train_cfg.algorithm.clip_param = sched0, clip0
        alg = runner.alg
        assert runner.use_graphs == mode and alg.use_graphs == mode and alg.clip_param == CLIP_OFF
        assert alg.fused_loss == alg.fused_rollout == (task != "go2_mcp_cts")          # (MCP-CTS: a state-dependent std keeps it off the fused heads, on a GPU too)
        own = alg._own_plan() is not None
        assert own == (task in OWN_PLAN_TASKS)
        T, A = alg.storage.num_transitions_per_env, alg.storage.actions.shape[-1]
        gen, buf, calls = torch.Generator().manual_seed(17), torch.zeros(T, N, A, device=alg.device), [0]

        def noise(self_, like, buf=buf, calls=calls, T=T):
            row = buf[calls[0] % T]; calls[0] += 1
            assert row.shape == like.shape
            return row
        monkeypatch.setattr(ActorCriticCTS, "_noise", noise)
        draws = []
        if not own:
            # no own plan (AC-MoE, Dual-MoE, MCP): graph mode gathers by storage.mini_batch_indices (torch.randperm on the device) exactly as eager mode does, so the
            # arms draw the same permutations when torch's generator is seeded alike before every draw: update u of every arm under torch.manual_seed(1000 + u)
            real = alg.storage.mini_batch_indices

            def seeded(nmb, real=real, draws=draws, T=T, st=alg.storage, flip=(arm == "reordered")):
                torch.manual_seed(1000 + len(draws))
                mbs = real(nmb)
                draws.append(torch.cat(mbs).cpu())
                nt = st.teacher_num_envs * T // nmb
                return [torch.cat([b[:nt].flip(0), b[nt:].flip(0)]) for b in mbs] if flip else mbs
            alg.storage.mini_batch_indices = seeded
        elif not mode:
            st = alg.storage
            key = torch.tensor([int((torch.initial_seed() * 0x9E3779B1 + 0x7F4A7C15) & 0x7FFFFFFF), 0, 0, 0], dtype=torch.int32, device=alg.device)          # _RolloutHeads._make_shuffle_key
            order = torch.empty(N * T, dtype=torch.int64, device=alg.device)

            def keyed(nmb, st=st, key=key, order=order, T=T, flip=(arm == "reordered")):
                nt, ns = st.teacher_num_envs * T, st.student_num_envs * T
                rc = hip.go2sim_cts_minibatch_indices(C.c_void_p(order.data_ptr()), nmb, nt, ns, C.c_void_p(st.ref2mine.data_ptr()), C.c_void_p(key.data_ptr()),
                                                      C.c_void_p(torch.cuda.current_stream(alg.device).cuda_stream))
                assert rc == 0, hip.go2sim_last_error().decode()
                rows = (nt // nmb + ns // nmb)
                mbs = [order[i * rows:(i + 1) * rows].clone() for i in range(nmb)]
                return [torch.cat([b[:nt // nmb].flip(0), b[nt // nmb:].flip(0)]) for b in mbs] if flip else mbs
            st.mini_batch_indices = keyed
        env.common_step_counter = 0
        first, trail = None, []
        for it in range(iters):
            buf.copy_(torch.randn(buf.shape, generator=gen))
            runner.learn(1, init_at_random_ep_len=(it == 0))
            trail.append(torch.cat([p.detach().reshape(-1) for p in alg.model.parameters()]).clone())
            if it == 0:
                first = {n: p.detach().cpu().numpy().copy() for n, p in alg.model.named_parameters()}
        torch.cuda.synchronize()
        assert calls[0] % T == 0 and calls[0] >= T
        if mode:
            assert runner._rollout_graph is not None and all(s.graph is not None for grp in alg._steps for s in grp)
            assert runner.graphs_captured() == {"rollout": True, "update": True} and alg.graphs_captured()
        if not own:
            assert len(draws) == iters                                                 # one permutation per update, from the seeded generator
        elif mode:
            assert alg._head_step.graph is not None                                   # the keyed permutation + gather ran as a graph, not through the eager fall-back
            assert int(alg._shuffle_key[1]) == ITERS                                   # one counter step per update
        else:
            assert int(key[1]) == iters
        out[{"eager": False, "graph": True}.get(arm, arm)] = (alg.learning_rate, torch.cat([p.detach().reshape(-1) for p in alg.model.parameters()]).cpu().numpy(),
                     env.common_step_counter, float(env.rew_buf.mean()), runner.history.abs().mean().item(), {n: p.detach().cpu().numpy().copy() for n, p in alg.model.named_parameters()}, first, draws, [t.cpu().numpy() for t in trail])
        env.close()
    assert out[True][2] == out[False][2] == ITERS * 24
    assert len(out[True][7]) == len(out[False][7]) and all(torch.equal(a, b) for a, b in zip(out[True][7], out[False][7]))          # (no own plan) both arms gathered by the same index lists
    assert all(np.isfinite(out[True][5][n]).all() and np.isfinite(out[False][5][n]).all() for n in out[True][5])
    assert np.isfinite(out[True][1]).all() and out[True][4] > 0
    assert abs(out[True][0] - 1e-3) < 1e-9 and abs(out[False][0] - 1e-3) < 1e-9
    d = np.abs(out[True][1] - out[False][1])
    print("[graph vs eager %s] weight gap median %.2e p99 %.2e max %.2e, reward %.4f / %.4f" % (task, np.median(d), np.quantile(d, 0.99), d.max(), out[True][3], out[False][3]))
    # (1) after the FIRST iteration — same weights, same noise, same permutation, the same rollout kernels: the two arms have seen the same data, what differs is
    # the update's formulation (explicit launches against autograd over the same GEMM kernels), i.e. summation orders.  20 + 20 Adam steps of 1e-3: a launch that is
    # dropped, doubled or fed another mini-batch moves the weights it touches by ~1e-3 PER STEP; every parameter tensor is held on its own so that one layer's launch
    # cannot hide among a million other weights.  (Graphs are not captured yet in iteration 1: the warm-up calls run the same launches through Python.)
    # (Adam turns the SIGN of a near-zero gradient into a full +-1e-3 step, so single weights can sit an order of magnitude above the rest: the median of a tensor is
    #  the sharp statistic, its largest element the loose one)
    per1 = {n: float(np.abs(out[True][6][n] - out[False][6][n]).max()) for n in out[True][6]}
    med1 = {n: float(np.median(np.abs(out[True][6][n] - out[False][6][n]))) for n in out[True][6]}
    print("   after iteration 1, per tensor: largest median gap %.1e (%s), largest element gap %.1e (%s)" % (max(med1.values()), max(med1, key=med1.get), max(per1.values()), max(per1, key=per1.get)))
    # What rounding alone does on this data: the eager formulation against ITSELF with every mini-batch's rows in reverse order (identical sums, another order).
    # Adam's step is lr * m / (sqrt(v) + eps): a gradient element that is a small difference of large per-row terms carries the summation order's rounding at full
    # relative size, and 20 + 20 steps pass it on — how much depends on the data (gate layers, whose gradients sum to zero over the experts, and encoders near a flat
    # spot of the latent loss most), not on the formulation.
    medn = {n: float(np.median(np.abs(out["reordered"][6][n] - out[False][6][n]))) for n in out[True][6]}
    pern = {n: float(np.abs(out["reordered"][6][n] - out[False][6][n]).max()) for n in out[True][6]}
    print("   eager vs eager with reordered rows, after iteration 1: largest median gap %.1e (%s), largest element gap %.1e (%s)" % (max(medn.values()), max(medn, key=medn.get), max(pern.values()), max(pern, key=pern.get)))
    # the two formulations may differ by what a reordering of the same formulation does (x 4), floor GAP1_MED; a dropped launch moves its tensor by ~1e-3 per step
    bound1 = max(GAP1_MED, 4.0 * max(medn.values()))
    assert bound1 < 3e-4, medn
    assert max(med1.values()) < bound1 and max(per1.values()) < max(2e-3, 4.0 * max(pern.values())), (med1, per1, medn)
    # (2) after the last iteration (5: 100 + 100 steps, the last three replayed from HIP graphs): the rounding differences have been fed back through the simulator for 120 env
    # steps (contacts make the trajectories of the two arms drift apart: rough terrain more than the plane), so this bound is looser — measured (round 6) medians 3.0e-4
    # (plane) / 6.4e-4 / 7.7e-4 (rough) over all weights, 1.1e-3 / 2.4e-3 / 3.1e-3 for the worst tensor; a replay that reads stale memory or skips a launch is off by 1e-2 and more
    per = {n: float(np.median(np.abs(out[True][5][n] - out[False][5][n]))) for n in out[True][5]}
    print("   after iteration %d, median gap per tensor: max %.1e (%s)" % (ITERS, max(per.values()), max(per, key=per.get)))
    print("   median gap over all weights after iteration 1..%d: %s" % (ITERS, " ".join("%.1e" % np.median(np.abs(a - b)) for a, b in zip(out[True][8], out[False][8]))))
    if drift:
        assert np.median(d) < 2e-3 and np.quantile(d, 0.99) < 2e-2, (np.median(d), np.quantile(d, 0.99), d.max())
        assert max(per.values()) < 8e-3, per
    assert abs(out[True][3] - out[False][3]) < 0.02


@pytest.mark.parametrize("task", ["go2_flat_cts", "go2_cts", "go2_moe_cts"])
def test_cts_training_graph_vs_eager_on_gpu(hip, task, monkeypatch):
    """CTS / MoE-CTS through the product path: HIP-graph mode (the no-autograd mini-batch steps, the keyed device-side permutation, the captured rollout) against eager
    mode (autograd over the same kernels) fed the SAME mini-batch permutations and the SAME exploration noise, so the two runs differ by rounding only and the weights
    after 5 iterations (100 policy + 100 student Adam steps) are held to a bound a dropped or reordered launch breaks by orders of magnitude:
      * permutations: the eager arm's storage.mini_batch_indices asks go2sim_cts_minibatch_indices (the kernel graph mode's update head launches) under the key
        graph mode derives from torch.manual_seed — same (seed, counter) sequence, so also a check of the counter's advance per update;
      * noise: both arms' modules hand out rows of one pre-drawn [T, N, A] buffer, refilled from a CPU generator before every iteration (a static address: the
        captured rollout reads the refreshed values on replay).
    (Round 5 bounded the median weight gap of two differently-shuffled, differently-perturbed runs by 7e-3 — a statistic that could not tell an arithmetic change
    from noise.)  The eager arithmetic is pinned to the reference in tests/test_cts_golden.py, graph mode's in tests/test_gpu_update_golden.py."""
    _cts_graph_vs_eager(hip, task, monkeypatch, 512, 5, drift=True)


@pytest.mark.parametrize("task", ["go2_flat_moe_cts", "go2_moe_ng_cts", "go2_ac_moe_cts", "go2_dual_moe_cts", "go2_mcp_cts"])
def test_cts_variant_training_graph_vs_eager_on_gpu(hip, task, monkeypatch):
    """The other five registered CTS tasks through the product path, graph mode against eager mode, at 256 envs x 4 iterations — the smallest run whose last iteration
    replays both the captured rollout (2 eager + capture) and the captured update steps: MoE-CTS on the plane and MoE-NG-CTS (own plan: the keyed device-side permutation,
    as above; MoE-NG-CTS's rollout latent as torch modules inside the captured rollout), AC-MoE / Dual-MoE / MCP-CTS (no own plan: autograd over the fused nodes captured per
    mini-batch slot, both arms fed the same torch.manual_seed per update and the gathered index lists compared; MCP-CTS samples with its state-dependent std from the same
    injected noise, through ActorCriticCTS._noise like the others).  The iteration-1 bounds are the parent test's; after iteration 4 only finiteness and the reward means
    (no drift bound has been measured for these tasks: the per-tensor medians are printed, DESIGN.md records them)."""
    _cts_graph_vs_eager(hip, task, monkeypatch, 256, 4, drift=False)


@pytest.mark.parametrize("terrain", ["plane", "heightfield"])
def test_pretrained_policy_walks_on_gpu(hip, terrain):
    """The reference's pretrained CTS student (weights committed as fixture data, loaded through this build's ActorCriticCTS) tracks
    a 1 m/s command on the HIP simulator: on the plane, and on the rough curriculum map it was trained for."""
    from helpers import heightfield_overrides
    from test_export import run_pretrained_walk
    N = 80
    ov = heightfield_overrides(N)[1] if terrain == "heightfield" else {}
    s = DeviceSim(hip, num_envs=N, push_robots=0, add_noise=0, **ov)
    v, zmin, resets = run_pretrained_walk(s, seconds=8.0)
    if terrain == "plane":
        assert 0.8 < v < 1.1 and zmin > 0.25 and resets == 0, (v, zmin, resets)
    else:
        assert 0.5 < v < 1.1 and resets <= N // 2, (v, zmin, resets)       # levels 0-5 of slopes, stairs, obstacles: mostly walks, may trip
    s.close()


def test_train_save_play_export_on_gpu(hip, tmp_path):
    """train.py -> checkpoint -> play.py (resume through the runner, export, roll out) for the CTS task."""
    import torch
    from go2_rl_gym_amd.envs import task_registry  # noqa: F401
    from go2_rl_gym_amd.scripts.play import play
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat_cts", "--num_envs", "256", "--headless"])
    env, _ = task_registry.make_env("go2_flat_cts", args)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat_cts", args, log_root=str(tmp_path))
    runner.learn(2, init_at_random_ep_len=True)
    env.close()
    args = get_args(["--task", "go2_flat_cts", "--num_envs", "64", "--headless"])
    env, exported = play(args, steps=20, log_root=str(tmp_path), export_policy=True)
    assert torch.isfinite(env.obs_buf).all() and os.path.exists(exported[0]) and os.path.exists(exported[1])
    jit = torch.jit.load(exported[0])
    a, (none, lat) = jit(torch.zeros(1, 45))
    assert a.shape == (1, 12) and lat.shape == (1, 32)
    env.close()


def test_rollout_head_kernels_on_gpu(hip):
    """go2sim_act_head / go2sim_store_transition: HIP vs torch's own formulation (Normal.log_prob, ppo.py:104-114) at 4096 x 12."""
    import torch
    torch.manual_seed(0)
    N, A = 4096, 12
    dev = "cuda:0"
    mu, eps, value = torch.randn(N, A, device=dev), torch.randn(N, A, device=dev), torch.randn(N, 1, device=dev)
    std = (0.3 + torch.rand(A, device=dev))
    out = [torch.zeros(N, A, device=dev) for _ in range(4)] + [torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev)]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip.go2sim_act_head(p(mu), p(std), p(eps), p(value), *[p(o) for o in out], N, A, st) == 0
    torch.cuda.synchronize()
    a = mu + std * eps
    d = torch.distributions.Normal(mu, mu * 0 + std)
    assert torch.equal(out[0], a) and torch.equal(out[1], a) and torch.equal(out[2], mu) and torch.equal(out[3], (mu * 0 + std)) and torch.equal(out[5], value)
    np.testing.assert_allclose(out[4].view(-1).cpu().numpy(), d.log_prob(a).sum(-1).cpu().numpy(), atol=2e-5, rtol=1e-5)
    rew, dones, touts = torch.randn(N, device=dev), torch.rand(N, device=dev) < 0.1, torch.rand(N, device=dev) < 0.05
    rst, dst = torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev, dtype=torch.uint8)
    assert hip.go2sim_store_transition(p(rew), p(dones.view(torch.uint8)), p(touts.view(torch.uint8)), p(value), p(rst), p(dst), 0.99, N, st) == 0
    torch.cuda.synchronize()
    want = rew + 0.99 * torch.squeeze(value * touts.unsqueeze(1), 1)
    np.testing.assert_allclose(rst.view(-1).cpu().numpy(), want.cpu().numpy(), atol=1e-6)
    assert torch.equal(dst.view(-1).bool(), dones)
    assert hip.go2sim_store_transition(p(rew), p(dones.view(torch.uint8)), None, None, p(rst), p(dst), 0.99, N, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(rst.view(-1), rew)


def test_fused_linear_elu_on_gpu(hip):
    """go2sim_elu_backward_bias (HIP) inside modules/fused.py against plain autograd on the GPU at the real mini-batch shape."""
    import torch
    from go2_rl_gym_amd.rsl_rl.modules import fused
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic import _mlp
    torch.manual_seed(0)
    net = _mlp(263, [512, 256, 128], 1, "elu").cuda()
    x, tgt = torch.randn(24576, 263, device="cuda:0"), torch.randn(24576, 1, device="cuda:0")
    res = []
    for lib in (None, hip):
        fused.set_library(lib)
        try:
            net.zero_grad()
            out = net(x)
            ((out - tgt) ** 2).mean().backward()
            torch.cuda.synchronize()
            res.append((out.detach().clone(), [p.grad.clone() for p in net.parameters()]))
        finally:
            fused.set_library(None)
    np.testing.assert_allclose(res[1][0].cpu().numpy(), res[0][0].cpu().numpy(), atol=1e-5)
    for a, b in zip(res[0][1], res[1][1]):
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), atol=2e-6, rtol=2e-3)


@pytest.mark.parametrize("B,Cn", [(1, 4), (63, 12), (70, 260), (1000, 512), (24576, 128), (4099, 32)])
def test_elu_backward_bias_kernel_shapes_on_gpu(hip, B, Cn):
    """go2sim_elu_backward_bias at ragged shapes (rows not a multiple of the 64-row tile / of the 16-row trip, columns not a multiple of
    the 256-column block): every element of gz and the deterministic column sums against torch; gz may alias gy."""
    import torch
    torch.manual_seed(B + Cn)
    gy, y = torch.randn(B, Cn, device="cuda"), torch.randn(B, Cn, device="cuda")
    gz, gb = torch.empty_like(y), torch.empty(Cn, device="cuda")
    ws = torch.full((Cn * ((B + 63) // 64),), float("nan"), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = gy * torch.where(y > 0, torch.ones_like(y), y + 1.0)
    assert hip.go2sim_elu_backward_bias(p(gy), p(y), p(gz), p(gb), p(ws), B, Cn, st) == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(gz.cpu().numpy(), ref.cpu().numpy(), atol=1e-6)
    np.testing.assert_allclose(gb.cpu().numpy(), ref.double().sum(0).float().cpu().numpy(), atol=2e-5 * max(1.0, B ** 0.5), rtol=1e-5)
    gb1 = gb.clone()
    g2 = gy.clone()
    assert hip.go2sim_elu_backward_bias(p(g2), p(y), p(g2), p(gb), p(ws), B, Cn, st) == 0       # in place, and bit-reproducible
    torch.cuda.synchronize()
    assert torch.equal(g2, gz) and torch.equal(gb, gb1)
    assert hip.go2sim_elu_backward_bias(p(gy), p(y), p(gz), p(gb), p(ws), B, 6, st) != 0           # C must be a multiple of 4


@pytest.mark.parametrize("N", [1, 17, 4097])
def test_ragged_batches_on_gpu(hip, N):
    """Smallest, ragged (one full 16-env workgroup + 1) and just-over-BASELINE batches: the partially filled last workgroup
    computes the same as the oracle, env by env, and touches nothing outside its N envs."""
    from helpers import ill_conditioned_envs
    so = HostSim(load_oracle(), num_envs=N, seed=9)
    s64 = HostSim(load_oracle(f64=True), num_envs=N, seed=9)
    sd = DeviceSim(hip, num_envs=N, seed=9)
    so.reset_all(); sd.reset_all(); s64.reset_all()
    rng = np.random.default_rng(4)
    skipped = 0
    for it in range(6 if N > 1000 else 20):
        a = rng.normal(0, 1, (N, 12)).astype(np.float32)
        for k in STEP_STATE:
            v = np.asarray(getattr(so, k))
            getattr(sd, k)[...] = v; getattr(s64, k)[...] = v
        so.step(a); sd.step(a); s64.step(a.astype(np.float64))
        ok = ~ill_conditioned_envs(so, s64); skipped += int((~ok).sum())
        d = np.abs(np.asarray(so.obs_buf, np.float64) - np.asarray(sd.obs_buf, np.float64)).max(1)[ok]
        from helpers import PLANE_BOUND
        assert d.max() < PLANE_BOUND["obs_buf"], (it, np.sort(d)[-3:])                  # every (well-conditioned) env
        np.testing.assert_array_equal(np.asarray(so.reset_buf)[ok], np.asarray(sd.reset_buf)[ok])
    assert skipped <= max(2, N // 500)
    so.close(); sd.close(); s64.close()


def test_error_codes_on_gpu(hip):
    abi = hip.abi
    cfg = abi.Cfg(); hip.go2sim_default_cfg(C.byref(cfg))
    h = C.c_void_p()
    cfg.num_envs = 0
    assert hip.go2sim_create(C.byref(cfg), 0, C.byref(h)) == abi.GO2SIM_EINVAL
    cfg.num_envs = 16; cfg.terrain_mode = 1
    assert hip.go2sim_create(C.byref(cfg), 0, C.byref(h)) == abi.GO2SIM_EINVAL and b"heightfield" in hip.go2sim_last_error()
    cfg.terrain_mode = 0; cfg.struct_size += 8
    assert hip.go2sim_create(C.byref(cfg), 0, C.byref(h)) == abi.GO2SIM_EINVAL and b"mismatch" in hip.go2sim_last_error()
    assert hip.go2sim_step(None, None, None) != 0 and hip.go2sim_act_head(*([None] * 10), 4, 12, None) != 0


def test_train_script_entry_point_on_gpu(hip, tmp_path, monkeypatch):
    """scripts/train.py's train(args) — the reference's legged_gym/scripts/train.py:11-16 — for two iterations."""
    import torch
    from go2_rl_gym_amd.scripts import train as train_script
    import sys
    from go2_rl_gym_amd.utils import get_args
    monkeypatch.setattr(sys.modules["go2_rl_gym_amd.utils.task_registry"], "ROOT_DIR", str(tmp_path))     # logs/<experiment>/... under the temp dir
    args = get_args(["--task", "go2_flat", "--num_envs", "256", "--headless", "--max_iterations", "2"])
    train_script.train(args)
    runs = list((tmp_path / "logs" / "go2_flat_ppo").iterdir())
    assert len(runs) == 1 and any(f.name.startswith("model_") for f in runs[0].iterdir())
    torch.cuda.synchronize()


def test_fine_grained_calls_equal_the_fused_step_on_gpu(hip):
    """go2sim_simulate + go2sim_post_physics (two launches, the Isaac-Gym-shaped path) against go2sim_step (one fused launch) from the
    same state.  They are different instantiations of the kernel template, so under -ffast-math the results agree to fp32 round-off,
    not bit for bit (on the host builds they are identical: tests/test_lane_emulation.py)."""
    N = 128
    a_, b_ = DeviceSim(hip, num_envs=N, seed=4), DeviceSim(hip, num_envs=N, seed=4)
    a_.reset_all(); b_.reset_all()
    rng = np.random.default_rng(3)
    for it in range(10):
        act = rng.normal(0, 1, (N, 12)).astype(np.float32)
        for k in STEP_STATE:
            getattr(b_, k)[...] = np.asarray(getattr(a_, k))
        a_.step(act)
        b_.actions[:] = act; b_.simulate(); b_.post_physics(); b_.torch.cuda.synchronize()
        from helpers import PLANE_BOUND
        for k in ("root_states", "dof_state", "obs_buf", "privileged_obs_buf", "rew_buf"):
            d = np.abs(np.asarray(getattr(a_, k), np.float64) - np.asarray(getattr(b_, k), np.float64)).reshape(N, -1).max(1)
            assert d.max() < PLANE_BOUND[k], (k, it, np.sort(d)[-4:])
        np.testing.assert_array_equal(np.asarray(a_.reset_buf), np.asarray(b_.reset_buf))
    assert hip.go2sim_get_common_step_counter(a_.h) == hip.go2sim_get_common_step_counter(b_.h) == 10
    a_.close(); b_.close()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_multi_rank_update_shape_on_one_gpu(hip, task, monkeypatch):
    """The update as it runs with more than one rank — per mini-batch slot two captured halves and the RCCL all-reduce of the gradient
    bucket issued eagerly between their replays (algorithms/_graph.py) — exercised on one GPU with a 1-rank RCCL group
    (GO2_FORCE_COLLECTIVES=1): both halves were captured, training behaves like the single-graph mode."""
    import socket
    import torch
    import torch.distributed as dist
    from go2_rl_gym_amd.envs import task_registry  # noqa: F401
    from go2_rl_gym_amd.rsl_rl.algorithms._graph import ReducedStep
    from go2_rl_gym_amd.utils import get_args
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = {}
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("GO2_FORCE_COLLECTIVES", "1")
            s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
            dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda:0"))
        try:
            args = get_args(["--task", task, "--num_envs", "512", "--headless", "--seed", "3"])
            env, _ = task_registry.make_env(task, args)
            torch.manual_seed(3)
            runner, _ = task_registry.make_alg_runner(env, task, args, log_root=None)
            env.common_step_counter = 0
            runner.learn(6, init_at_random_ep_len=True)
            torch.cuda.synchronize()
            alg = runner.alg
            steps = alg._graph if task == "go2_flat" else alg._steps[0] + alg._steps[1]
            if forced:
                assert all(isinstance(g, ReducedStep) and g.front.graph is not None and g.back.graph is not None for g in steps)
            else:
                assert all(not isinstance(g, ReducedStep) and g.graph is not None for g in steps)
            model = alg.actor_critic if task == "go2_flat" else alg.model
            out[forced] = (alg.learning_rate, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy(), float(env.rew_buf.mean()))
            env.close()
        finally:
            if forced:
                dist.destroy_process_group()
    # the arithmetic of the split update is pinned on the CPU (tests/test_distributed.py: equal to the eager update, identical replicas);
    # here: it runs captured with RCCL between the halves and trains like the single-graph mode.  The adaptive rate at 512 envs is
    # chaotic (x1.5 per mini-batch), so the two runs are compared by behaviour, not by weights.
    assert np.isfinite(out[True][1]).all() and 1e-5 - 1e-12 <= out[True][0] <= 1e-2 + 1e-12
    assert abs(out[True][2] - out[False][2]) < 0.05


@pytest.mark.parametrize("terrain", ["plane", "heightfield"])
def test_env_shards_equal_slices_of_one_sim_on_gpu(hip, terrain):
    """Multi-GPU sharding on the real library (the oracle-side twin is tests/test_distributed.py): two HIP simulators with
    env_offset 0 / 2048 of num_envs_global = 4096 are rows [0, 2048) / [2048, 4096) of ONE 4096-env HIP simulator, bit for bit, after
    creation, reset and 20 steps — Philox key, plane grid origin, terrain level / type round robin, friction buckets and every
    creation-time draw depend on the GLOBAL env index only (go2sim_impl.cpp create / lane programs)."""
    import torch
    from helpers import heightfield_overrides
    Ng, n = 4096, 2048
    ov = heightfield_overrides(Ng)[1] if terrain == "heightfield" else {}
    whole = DeviceSim(hip, num_envs=Ng, seed=5, **ov)
    parts = [DeviceSim(hip, num_envs=n, env_offset=r * n, num_envs_global=Ng, seed=5, **ov) for r in range(2)]
    keys = ("root_states", "dof_state", "obs_buf", "privileged_obs_buf", "rew_buf", "reset_buf", "commands", "env_origins", "friction_coeffs", "link_mass_ratio",
            "added_base_mass", "motor_strengths", "episode_length_buf", "terrain_levels", "terrain_types", "contact_forces", "measured_heights", "episode_sums")

    def same(tag):
        for k in keys:
            w = whole.t[k]
            for r, prt in enumerate(parts):
                sl = w[:, r * n:(r + 1) * n] if k == "episode_sums" else w[r * n:(r + 1) * n]
                assert torch.equal(sl, prt.t[k]), "%s: %s differs between shard %d and the slice of the single simulator" % (tag, k, r)
    same("create")
    for s_ in [whole] + parts:
        s_.reset_all()
    torch.cuda.synchronize()
    same("reset")
    g = torch.Generator(device="cuda:0"); g.manual_seed(0)
    for it in range(20):
        a = torch.randn(Ng, 12, device="cuda:0", generator=g)
        hip.go2sim_step(whole.h, C.c_void_p(a.data_ptr()), whole._st())
        for r, prt in enumerate(parts):
            ar = a[r * n:(r + 1) * n].contiguous()
            hip.go2sim_step(prt.h, C.c_void_p(ar.data_ptr()), prt._st())
        torch.cuda.synchronize()
        same("step %d" % it)
    assert int(whole.t["reset_buf"].sum()) >= 0 and float(whole.t["contact_forces"].abs().max()) > 1.0
    for s_ in [whole] + parts:
        s_.close()


def test_parity_outliers_are_conditioning_not_fast_math(hip):
    """What the one-step parity bounds stand on, measured instead of asserted:
      * the device library built WITHOUT -ffast-math (tests/emu/libgo2sim_hip_precise.so, IEEE division / sqrt) has the same error
        distribution against the fp32 oracle as the shipped -ffast-math build => the differences are not fast-math artefacts;
      * the fp32 oracle itself differs from the fp64 oracle on the same inputs by the same amounts => they are the fp32 conditioning of the
        step (a contact row switching at gap = contact_offset, a friction-cone boundary, a joint-limit row), which ANY two fp32 evaluation
        orders share.  Both builds pass the plane bounds and the conditioning-relative gate; the report is written to gpurun_out/."""
    import json
    from helpers import PLANE_BOUND, StepErrors, check_plane_errors, check_relative_to_conditioning, load_hip_precise
    N, steps = 256, 60
    so, s64 = HostSim(load_oracle(), num_envs=N), HostSim(load_oracle(f64=True), num_envs=N)
    sims = {"fast_math": DeviceSim(hip, num_envs=N), "precise": DeviceSim(load_hip_precise(), num_envs=N)}
    for s_ in [so, s64] + list(sims.values()):
        s_.reset_all()
    rng = np.random.default_rng(0)
    errs = {b: StepErrors(PLANE_BOUND) for b in sims}
    cond = StepErrors(PLANE_BOUND)
    for it in range(steps):
        a = rng.normal(0, 1, (N, 12)).astype(np.float32)
        for k in STEP_STATE:
            v = np.asarray(getattr(so, k))
            getattr(s64, k)[...] = v
            for sd in sims.values():
                getattr(sd, k)[...] = v
        so.step(a); s64.step(a.astype(np.float64))
        for sd in sims.values():
            sd.step(a)
        cond.add(so, s64, N)
        for b, sd in sims.items():
            errs[b].add(so, sd, N, ref64=s64)
    q = lambda e, k: {"p50": float(np.quantile(e.all(k), 0.5)), "p99": float(np.quantile(e.all(k), 0.99)), "max": float(e.all(k).max())}
    report = {"envs": N, "steps": steps, "bounds": PLANE_BOUND, "oracle32_vs_oracle64": {k: q(cond, k) for k in PLANE_BOUND},
              **{b: {k: q(e, k) for k in PLANE_BOUND} for b, e in errs.items()}}
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    json.dump(report, open(os.path.join(ROOT, "gpurun_out", "parity_outliers.json"), "w"), indent=1)
    print(json.dumps(report))
    floors = {k: v / 500 for k, v in PLANE_BOUND.items()}
    for b, e in errs.items():
        check_plane_errors(e)
        check_relative_to_conditioning(e, cond, floors)
    for k in PLANE_BOUND:      # the two builds' distributions agree with each other
        assert 0.5 < np.quantile(errs["fast_math"].all(k), 0.99) / np.quantile(errs["precise"].all(k), 0.99) < 2.0, k
    for s_ in [so, s64] + list(sims.values()):
        s_.close()


def test_trimesh_walls_on_gpu(hip):
    """Row f4 on the device: the contact query against the trimesh's vertical faces equals the oracle's on random spheres over a staircase,
    and the known-answer behaviour of tests/test_trimesh_walls.py (feet pressed into a riser end up resting against its face; a foot pressed into the
    outside corner of a block is pushed out along the diagonal)."""
    import torch
    import test_trimesh_walls as tw
    from go2_rl_gym_amd.utils.terrain import SubTerrain, displaced_cell_heights, pyramid_stairs_terrain
    t = SubTerrain("t", width=60, length=60, vertical_scale=tw.VS, horizontal_scale=tw.HS)
    pyramid_stairs_terrain(t, step_width=0.31, step_height=0.15, platform_size=2.0)
    hf = np.ascontiguousarray(t.height_field_raw)
    ov = dict(terrain_mode=1, hf_rows=60, hf_cols=60, hf_hscale=tw.HS, hf_vscale=tw.VS, hf_border=0.0, hf_samples=hf,
              terrain_origins=np.zeros((1, 1, 3), np.float32), terrain_type_id=np.zeros(1, np.int32), terrain_num_levels=1, terrain_num_types=1,
              terrain_curriculum=0, max_init_terrain_level=0, hf_cells=np.ascontiguousarray(displaced_cell_heights(hf, tw.HS, tw.VS, 0.75)), hf_walls=1)
    so, sd = HostSim(load_oracle(), num_envs=1, **ov), DeviceSim(hip, num_envs=1, **ov)
    rng = np.random.default_rng(2)
    n = 20000
    pts = np.stack([rng.uniform(0.3, 5.6, n), rng.uniform(0.3, 5.6, n), rng.uniform(-0.05, 1.3, n), rng.uniform(0.0, 0.05, n)], 1).astype(np.float32)
    want = tw.query(load_oracle(), so, pts)
    dp, do = torch.as_tensor(pts, device="cuda:0"), torch.zeros(n, 4, device="cuda:0")
    assert hip.go2sim_debug_contact_query(sd.h, C.c_void_p(dp.data_ptr()), C.c_void_p(do.data_ptr()), n, sd._st()) == 0
    torch.cuda.synchronize()
    got = do.cpu().numpy()
    d = np.abs(got - want).max(1)
    # fp32 on both sides; a sphere centre within rounding of a cell boundary or of the two facets' diagonal may be assigned to the other side
    assert np.quantile(d, 0.999) < 2e-5 and (d > 1e-3).mean() < 2e-3, (float(np.quantile(d, 0.999)), float((d > 1e-3).mean()))
    assert (want[:, 3] < 0.5).mean() > 0.02           # the sample did hit vertical faces
    assert ((np.abs(want[:, 1]) > 0.1) & (np.abs(want[:, 2]) > 0.1)).sum() >= 5       # ... and the rings' outside corners (vertical edges of a diagonal-neighbour cell; round 6)
    so.close(); sd.close()
    tri = tw.settle_against_riser(hip, DeviceSim, "trimesh")
    assert np.all(np.abs(tri[:, 0] + 0.022 - 6.0) < 0.006) and np.all(np.abs(tri[:, 2] - 0.022) < 0.006), tri
    assert np.all(tw.settle_against_riser(hip, DeviceSim, "heightfield")[:, 0] < 5.93)

    # the outside corner of a block (tests/test_trimesh_walls.py): the query's known answers and the foot that is pushed out along the diagonal
    def device_query(lib, s, pts):
        dp, do = torch.as_tensor(np.ascontiguousarray(pts, np.float32), device="cuda:0"), torch.zeros(len(pts), 4, device="cuda:0")
        assert lib.go2sim_debug_contact_query(s.h, C.c_void_p(dp.data_ptr()), C.c_void_p(do.data_ptr()), len(pts), s._st()) == 0
        torch.cuda.synchronize()
        return do.cpu().numpy()
    got, exp = tw.corner_queries(hip, DeviceSim, query=device_query)
    np.testing.assert_allclose(got, exp, atol=3e-5)
    # the device's one-record-per-cell query against the oracle's direct neighbour reads on a map of independent random cells (grid borders included)
    ov_r, pts_r = tw.random_cells_world()
    so_r, sd_r = HostSim(load_oracle(), num_envs=1, **ov_r), DeviceSim(hip, num_envs=1, **ov_r)
    want_r, got_r = tw.query(load_oracle(), so_r, pts_r), device_query(hip, sd_r, pts_r)
    so_r.close(); sd_r.close()
    tw.check_against_oracle_on_random_cells(got_r, want_r)
    first, forces, off, z = tw.foot_pressed_into_corner(hip, DeviceSim)
    first_o, forces_o, off_o, z_o = tw.foot_pressed_into_corner(load_oracle(), HostSim)
    assert (forces[:, 0] < -1.0).all() and (forces[:, 1] < -1.0).all() and abs(np.hypot(*off) - 0.022) < 0.003, (forces, off)
    assert np.abs(first - first_o).max() < 2e-3 and np.abs(off - off_o).max() < 2e-3 and abs(z - z_o) < 2e-3, (first, first_o, off, off_o)


def test_calf_across_a_nosing_reports_a_calf_force_on_gpu(hip):
    """The known-answer case of the capsule flank samples (tests/test_trimesh_walls.py::calf_across_nosing) on the HIP kernel: only the middle of the
    FL calf touches the riser's edge; the calf body reports the force, equal to the oracle's."""
    import test_trimesh_walls as tw
    gaps_o, f_o, _ = tw.calf_across_nosing(load_oracle(), HostSim)
    import torch

    def device_query(lib, s, pts):
        dp, do = torch.as_tensor(np.ascontiguousarray(pts, np.float32), device="cuda:0"), torch.zeros(len(pts), 4, device="cuda:0")
        assert lib.go2sim_debug_contact_query(s.h, C.c_void_p(dp.data_ptr()), C.c_void_p(do.data_ptr()), len(pts), s._st()) == 0
        torch.cuda.synchronize()
        return do.cpu().numpy()
    gaps, f, others = tw.calf_across_nosing(hip, DeviceSim, query=device_query)
    assert gaps[0] > 0.0105 and gaps[1] > 0.03 and abs(gaps[2] + 0.004) < 2e-4, gaps
    assert f[1] > 1.0 and others == 0.0, (f, others)
    assert abs(f[1] - f_o[1]) < 2e-3 * f_o[1], (f, f_o)


def test_step_rollout_on_gpu(hip):
    """go2sim_step_rollout on the device: redirected observation rows, fused transition store, extras copy == go2sim_step + those operations."""
    from test_lane_emulation import check_step_rollout
    check_step_rollout(hip, DeviceSim, 200)


def test_fused_clip_adam_matches_torch_on_gpu(hip):
    """go2sim_adam_clip_step (adaptive-KL learning rate + clip_grad_norm_ + Adam, two kernels) against torch.nn.utils.clip_grad_norm_ +
    torch.optim.Adam on the same gradients over several steps (ppo.py:140-155,178-181): parameters, both moments, step counters, learning rate."""
    import torch
    from go2_rl_gym_amd.rsl_rl.algorithms._graph import FusedClipAdam
    torch.manual_seed(0)
    shapes = [(512, 45), (512,), (256, 512), (256,), (128, 256), (128,), (12, 128), (12,), (12,), (5000, 33)]
    pa = [torch.nn.Parameter(torch.randn(s, device="cuda:0") * 0.1) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    lra, lrb = torch.tensor(1e-3, device="cuda:0"), 1e-3
    oa = torch.optim.Adam(pa, lr=lra, capturable=True, fused=True)
    ob = torch.optim.Adam(pb, lr=lrb)
    fa = FusedClipAdam(hip, oa, pa, 1.0)
    assert fa.usable
    for it in range(6):
        scale = [3.0, 0.01, 1.0, 30.0, 0.3, 1.0][it]              # clipped and unclipped steps
        kl = [0.05, 0.001, 0.011, 0.0, 0.004, 0.03][it]           # lr down, up, keep, keep (kl == 0), up, down
        for a, b in zip(pa, pb):
            g = torch.randn_like(a) * scale * 1e-2
            a.grad, b.grad = g.clone(), g.clone()
        assert fa.step(torch.tensor(kl, device="cuda:0"), 0.01)
        if kl > 0.02: lrb = max(1e-5, lrb / 1.5)
        elif kl < 0.005 and kl > 0.0: lrb = min(1e-2, lrb * 1.5)
        for gr in ob.param_groups: gr["lr"] = lrb
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        ob.step()
        assert abs(float(lra) - lrb) < 1e-9 + 2e-7 * lrb
        for a, b in zip(pa, pb):
            np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), atol=2e-7, rtol=2e-6)
            np.testing.assert_allclose(oa.state[a]["exp_avg"].cpu().numpy(), ob.state[b]["exp_avg"].cpu().numpy(), atol=1e-9, rtol=2e-6)
            np.testing.assert_allclose(oa.state[a]["exp_avg_sq"].cpu().numpy(), ob.state[b]["exp_avg_sq"].cpu().numpy(), atol=1e-12, rtol=2e-6)
            assert float(oa.state[a]["step"]) == it + 1
    sd = oa.state_dict()                                          # the torch optimizer's own state: checkpoints are unchanged
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("launch", ["torchrun", "plain"])
def test_two_rank_bench_rehearsal_on_one_gpu(hip, launch):
    """`bench.py --gpus 2` exactly as the driver launches it (torch.distributed.run, one process per rank) and started PLAINLY (`python bench.py --gpus 2`: bench.py
    then launches its own ranks — the driver's N = 1 command line has no launcher in front of it), rehearsed on the ONE GPU of a test
    box: GO2_DIST_BACKEND=gloo lets both ranks share cuda:0 (RCCL refuses two ranks on one device).  Exercises on the real library what a
    node would: env shards at env_offset 0 / N of 2N, the policy broadcast, the advantage-statistics all-reduce, the two captured halves of
    every mini-batch step with the eager gradient all-reduce between them, the barrier / MAX-over-ranks timing and the single JSON line."""
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, GO2_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port)] if launch == "torchrun" else [sys.executable]
    cmd += [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "3", "--num-envs", "1024"]
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                    # rank 0 prints ONE line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["backend"] == "gloo" and out["scaling"] == "weak"
    assert out["graphs"]["rollout"] and out["graphs"]["update"]
    assert out["collectives_per_iteration"]["all_reduce"] == 21            # 1 advantage statistics + 5 epochs x 4 mini-batches
    assert out["value"] > 0 and abs(out["value"] - 2 * 1024 * 24 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    assert "cpu_baseline" not in out                                       # rank 0 at N = 1 only


def test_fallen_robot_contact_set_on_gpu(hip):
    """GPU twin of tests/test_lane_emulation.py::test_fallen_robot_reports_base_thigh_and_calf_at_once: robots lying on the trunk and on the
    thigh AND the calf of one leg report all three body forces in one step on the HIP kernel (one contact slot per body group of a leg, the
    non-foot slots' rows parked in LDS), and the 19 body forces equal the oracle's from the same inputs."""
    from helpers import BASE_B, CALF_B, LYING_KW, THIGH_B, lying_robot_batch, three_body_envs
    M = 256
    so, sd = HostSim(load_oracle(), num_envs=M, **LYING_KW), DeviceSim(hip, num_envs=M, **LYING_KW)
    so.reset_all(); sd.reset_all()
    rng = np.random.default_rng(0)
    seen3 = most = 0
    for trial in range(3):
        lying_robot_batch(so, rng)
        for k in STEP_STATE:
            getattr(sd, k)[...] = np.asarray(getattr(so, k))
        a = np.zeros((M, 12), np.float32)
        so.step(a); sd.step(a)
        ids, no = three_body_envs(so.contact_forces)
        _, nd = three_body_envs(np.asarray(sd.contact_forces))
        for e in ids:
            legs = [l for l in range(4) if no[e, THIGH_B[l]] > 0.5 and no[e, CALF_B[l]] > 0.5]
            for b in [BASE_B] + [THIGH_B[l] for l in legs] + [CALF_B[l] for l in legs]:
                assert nd[e, b] > 0.25 * min(no[e, b], 4.0), (e, b, no[e, b], nd[e, b])
        seen3 += len(ids); most = max(most, int((nd > 0.1).sum(1).max()))
        assert ((nd[:, THIGH_B] > 0.1).sum(1) + (nd[:, CALF_B] > 0.1).sum(1)).max() >= 5      # _reward_collision counts past the round-2 model's 4
        fo, fd = np.asarray(so.contact_forces, np.float64), np.asarray(sd.contact_forces, np.float64)
        d = np.abs(fo - fd).reshape(M, -1).max(1) / (1.0 + np.abs(fo).reshape(M, -1).max(1))
        assert np.median(d) < 1e-4 and np.quantile(d, 0.99) < 1e-2, np.sort(d)[-4:]          # relative to each env's force scale (impulse / 5 ms)
        np.testing.assert_allclose(np.asarray(so.root_states), np.asarray(sd.root_states), atol=5e-3)
        np.testing.assert_array_equal(np.asarray(so.reset_buf), np.asarray(sd.reset_buf))
    assert seen3 >= 30 and most >= 10, (seen3, most)
    so.close(); sd.close()
