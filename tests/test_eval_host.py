"""The policy evaluator on the CPU: the host build of the go2nn_eval_* kernels (include/go2nn.h) against float64 restatements written here, PolicyEvaluator on the
oracle + the host build, the calls an evaluation makes by name and order in every mode, its isolation from a training run, and the runner hook / CLI."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from helpers import ROOT, load_nn_emu, load_oracle, lognormal_table, reduce_groups, reduce_twice
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import EVAL_FIELDS, EVAL_METRICS, GO2NN_EVAL_NUM, Go2nnEvalIn
from go2_rl_gym_amd.envs import task_registry
from go2_rl_gym_amd.utils import get_args

U = 2.0 ** -24
WIDTH = {"commands": 4, "base_lin_vel": 3, "base_ang_vel": 3, "projected_gravity": 3, "torques": 12, "actions": 12, "last_actions": 12}
LIMITS = np.stack([np.linspace(-1.0, -0.5, 12), np.linspace(0.6, 1.2, 12)], 1).astype(np.float32)


def random_step(rng, N):
    """one step's inputs (logical shapes, fp32): zero commands, resets with and without time-out, joints on both sides of their limits all occur"""
    d = {k: rng.normal(0, 1, (N, w)).astype(np.float32) for k, w in WIDTH.items()}
    d["commands"][rng.random(N) < 0.25, :2] = 0.0
    d["torques"] *= 10.0
    d["dof_state"] = np.stack([rng.uniform(-1.4, 1.6, (N, 12)), rng.normal(0, 5, (N, 12))], 2).astype(np.float32)
    calm = rng.random(N) < 0.5
    d["dof_state"][calm, :, 0] = rng.uniform(-0.4, 0.5, (int(calm.sum()), 12)).astype(np.float32)          # inside every limit
    d["reset_buf"] = (rng.random(N) < 0.2).astype(np.uint8)
    d["time_out_buf"] = (d["reset_buf"] & (rng.random(N) < 0.5)).astype(np.uint8)
    return d


def reference_terms(d, limits):
    """the table of include/go2nn.h in float64 -> [GO2NN_EVAL_NUM, N]"""
    f = {k: np.asarray(v, np.float64) for k, v in d.items()}
    c, v, N = f["commands"], f["base_lin_vel"], d["commands"].shape[0]
    cn = np.sqrt(c[:, 0] ** 2 + c[:, 1] ** 2)
    q, qd = f["dof_state"][:, :, 0], f["dof_state"][:, :, 1]
    lim = np.asarray(limits, np.float64)
    t = np.zeros((GO2NN_EVAL_NUM, N))
    t[0] = 1.0
    t[1] = np.sqrt((c[:, 0] - v[:, 0]) ** 2 + (c[:, 1] - v[:, 1]) ** 2)
    t[2] = np.abs(c[:, 2] - f["base_ang_vel"][:, 2])
    t[3] = np.where(cn < 1e-6, 0.0, (v[:, 0] * c[:, 0] + v[:, 1] * c[:, 1]) / np.where(cn < 1e-6, 1.0, cn))
    t[4] = np.sqrt(f["projected_gravity"][:, 0] ** 2 + f["projected_gravity"][:, 1] ** 2)
    t[5] = np.abs(f["torques"] * qd).sum(1)
    t[6] = (f["torques"] ** 2).sum(1)
    t[7] = ((f["actions"] - f["last_actions"]) ** 2).sum(1)
    t[8] = ((q < lim[None, :, 0]) | (q > lim[None, :, 1])).any(1)
    t[9] = (d["reset_buf"] != 0) & (d["time_out_buf"] == 0)
    return t


def pack(d, layout):
    """the step's inputs as the libraries store them -> ({name: flat array}, Go2nnEvalIn fields as (env stride, comp stride), dof_vel_offset)"""
    N = d["commands"].shape[0]
    arrs, strides = {}, {}
    for k in EVAL_FIELDS:
        a = d[k]
        if layout == 1 and a.ndim > 1:
            arrs[k] = np.ascontiguousarray(a.transpose(*reversed(range(a.ndim))))          # [N, a, b] stored as [b, a, N]
            strides[k] = (1, N)
        else:
            arrs[k] = np.ascontiguousarray(a)
            strides[k] = (int(np.prod(a.shape[1:])) if a.ndim > 1 else 1, (2 if k == "dof_state" else 1) if a.ndim > 1 else 0)
    return arrs, strides, (12 * N if layout == 1 else 1)


def eval_in(ptr_of, strides, vel_off, limits_ptr):
    a = Go2nnEvalIn()
    for k in EVAL_FIELDS:
        f = getattr(a, k)
        f.p, (f.env_stride, f.comp_stride) = ptr_of(k), strides[k]
    a.dof_limits, a.dof_vel_offset, a.dt = limits_ptr, vel_off, 0.02
    return a


def accumulate_bound(S, abs_sum):
    """|acc - ref| <= (S + 32) 2^-24 sum|terms|: S roundings of the running fp32 sum plus at most 32 rounded operations inside one term"""
    return (S + 32) * U * abs_sum


def run_accumulate_case(call, N, layout, S=64, seed=0):
    """call(arrs, strides, vel_off, acc) runs one go2nn_eval_accumulate on a library; -> (acc fp32 [NUM, N], ref, sum|terms|)"""
    rng = np.random.default_rng(seed + 7 * N + layout)
    acc = np.zeros((GO2NN_EVAL_NUM, N), np.float32)
    ref, mag = np.zeros((GO2NN_EVAL_NUM, N)), np.zeros((GO2NN_EVAL_NUM, N))
    for _ in range(S):
        d = random_step(rng, N)
        t = reference_terms(d, LIMITS)
        ref += t; mag += np.abs(t)
        acc = call(*pack(d, layout), acc)
    return acc, ref, mag


def check_accumulate(acc, ref, mag, S, what):
    for m in (0, 8, 9):
        np.testing.assert_array_equal(acc[m].astype(np.float64), ref[m], err_msg=EVAL_METRICS[m])
    assert ref[8].min() < S and ref[8].max() > 0 and ref[9].max() > 0 and (ref[3] == 0).sum() == 0          # the cases occur (a zero command only some of the steps)
    bound = accumulate_bound(S, mag)
    ratio = np.abs(acc.astype(np.float64) - ref) / np.maximum(bound, 1e-300)
    print("%s: largest |acc - ref| / bound per metric: %s" % (what, ", ".join("%s %.3f" % (EVAL_METRICS[m], ratio[m].max()) for m in range(1, 8))))
    assert (ratio[1:8] <= 1.0).all(), ratio[1:8].max()


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [1, 17, 257])
def test_accumulate_against_float64(emu, N, layout):
    lim = LIMITS.copy()

    def call(arrs, strides, vel_off, acc):
        a = eval_in(lambda k: arrs[k].ctypes.data, strides, vel_off, lim.ctypes.data)
        assert emu.go2nn_eval_accumulate(C.byref(a), C.c_void_p(acc.ctypes.data), N, None) == 0, emu.go2nn_last_error()
        return acc
    acc, ref, mag = run_accumulate_case(call, N, layout)
    check_accumulate(acc, ref, mag, 64, "host N=%d layout=%d" % (N, layout))
    assert emu.go2nn_eval_clear(C.c_void_p(acc.ctypes.data), N, None) == 0 and not acc.any()
    bad = Go2nnEvalIn()
    assert emu.go2nn_eval_accumulate(C.byref(bad), C.c_void_p(acc.ctypes.data), N, None) == _nn.bind.__globals__.get("GO2NN_EINVAL", -22)


def reduce_reference(acc, group, G):
    """math.fsum of the same fp32 accumulators per group -> (out [G, NUM + 2], sum|acc| [G, NUM])"""
    out, mag = np.zeros((G, GO2NN_EVAL_NUM + 2)), np.zeros((G, GO2NN_EVAL_NUM))
    for g in range(G):
        ids = np.nonzero(group == g)[0]
        for m in range(GO2NN_EVAL_NUM):
            out[g, m] = math.fsum(float(x) for x in acc[m, ids])
            mag[g, m] = math.fsum(abs(float(x)) for x in acc[m, ids])
        out[g, GO2NN_EVAL_NUM] = len(ids)
        out[g, GO2NN_EVAL_NUM + 1] = int((acc[9, ids] == 0).sum())
    return out, mag


def reduce_case(N, G, seed=3):
    rng = np.random.default_rng(seed + N)
    acc = lognormal_table(rng, GO2NN_EVAL_NUM, N)
    acc[9] = (rng.random(N) < 0.3) * rng.integers(1, 4, N)
    return acc, reduce_groups(rng, N, G)


def check_reduce(out, acc, group, G, N, what):
    ref, mag = reduce_reference(acc, group, G)
    np.testing.assert_array_equal(out[:, GO2NN_EVAL_NUM:], ref[:, GO2NN_EVAL_NUM:])
    assert (out[1] == 0).all() and ref[1, GO2NN_EVAL_NUM] == 0
    gap = np.abs(out[:, :GO2NN_EVAL_NUM] - ref[:, :GO2NN_EVAL_NUM])
    bound = N * 2.0 ** -53 * mag
    print("%s: largest reduce gap / bound %.3f" % (what, (gap / np.maximum(bound, 1e-300)).max()))
    assert (gap <= bound).all()


@pytest.mark.parametrize("N,G", [(1, 3), (17, 3), (257, 5), (4096, 7)])
def test_reduce_against_fsum(emu, N, G):
    acc, group = reduce_case(N, G)
    out = reduce_twice(lambda *a: emu.go2nn_eval_reduce(*a, None), acc, group, G, GO2NN_EVAL_NUM + 2)
    check_reduce(out, acc, group, G, N, "host N=%d" % N)


def test_eval_symbols_and_struct_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_eval_accumulate", "go2nn_eval_reduce", "go2nn_eval_clear"):
            assert (" T " + f + "\n") in syms, (path, f)
    names = list(EVAL_FIELDS) + ["dof_limits", "dof_vel_offset", "dt"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu %zu %d", sizeof(Go2nnEvalIn), sizeof(Go2nnEvalField), GO2NN_EVAL_NUM);\n'
                   + "".join('printf(" %%zu", offsetof(Go2nnEvalIn, %s));\n' % n for n in names) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:3] == [C.sizeof(Go2nnEvalIn), C.sizeof(_nn.Go2nnEvalField), len(EVAL_METRICS)]
    assert got[3:] == [getattr(Go2nnEvalIn, n).offset for n in names]
    hdr = open(os.path.join(ROOT, "include", "go2nn.h")).read()
    enum = hdr[hdr.index("GO2NN_EVAL_STEPS = 0"):hdr.index("GO2NN_EVAL_NUM\n")]
    assert [e.strip().split(" ")[0].replace("GO2NN_EVAL_", "").lower() for e in enum.split(",") if e.strip()] == list(EVAL_METRICS)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
EVAL = dict(enabled=True, interval=2, num_envs=38, seconds=1.0, warmup_s=0.1, terrain_level=3, seed=77,
            scenarios=[["forward_1.0", 1.0, 0.0, 0.0], ["lateral_0.5", 0.0, 0.5, 0.0], ["turn_1.0", 0.0, 0.0, 1.0], ["stand", 0.0, 0.0, 0.0]])


def small_actor_critic(seed=0):
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(seed)
    return ActorCritic(45, 263, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", init_noise_std=1.0)


def make_evaluator(emu, task="go2_flat", cb=None, **over):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env_cfg, _ = task_registry.get_cfgs(task)
    return PolicyEvaluator(env_cfg, dict(EVAL, **over), task_class=task_registry.get_task_class(task), device="cpu", lib=load_oracle(), nn_lib=emu, step_callback=cb)


def test_evaluator_on_host_libraries(emu):
    from go2_rl_gym_amd.utils.evaluator import EVAL_SOURCE, MEAN_METRICS, RESULT_KEYS
    rec = []

    def cb(ev, k, counted):
        b = ev.env._buf
        rec.append((counted, {n: b[EVAL_SOURCE.get(n, n)].detach().clone().numpy() for n in EVAL_FIELDS}))
    ev = make_evaluator(emu, cb=cb)
    ac = small_actor_critic()
    res = ev.evaluate(ac)
    assert ev.warmup_steps == 5 and ev.steps == 50 and len(rec) == 55 and res["mode"] == "eager"
    S, N, n_s = ev.steps, ev.num_envs, len(EVAL["scenarios"])
    # groups: every (terrain kind x scenario) pair, sizes within one of each other; the commands hold for the whole horizon
    sizes = np.bincount(ev.group_host, minlength=len(ev.groups))
    assert res["terrain_names"] == ["plane"] and len(ev.groups) == n_s and sizes.min() >= 1 and sizes.max() - sizes.min() <= 1 and sizes.sum() == N
    want = np.asarray([s[1:4] for s in EVAL["scenarios"]], np.float32)[ev.group_host % n_s]
    for _, d in rec:
        np.testing.assert_array_equal(d["commands"][:, :3], want)
    # every reported number from the recorded buffers, in float64
    lim = ev.dof_limits.numpy()
    ref, mag = np.zeros((GO2NN_EVAL_NUM, N)), np.zeros((GO2NN_EVAL_NUM, N))
    for counted, d in rec:
        if counted:
            t = reference_terms({k: (v.astype(np.uint8) if v.dtype == bool else v) for k, v in d.items()}, lim)
            ref += t; mag += np.abs(t)
    worst = 0.0
    for gi, (tname, sname) in enumerate(ev.groups + [("all", "all")]):
        ids = np.nonzero(ev.group_host == gi)[0] if gi < len(ev.groups) else np.arange(N)
        got = res["groups"][tname][sname] if gi < len(ev.groups) else res["overall"]
        assert set(got) == set(RESULT_KEYS) and got["n_envs"] == len(ids)
        steps = ref[0, ids].sum()
        assert steps == S * len(ids)
        for i, m in enumerate(MEAN_METRICS):
            r = ref[1 + i, ids].sum() / steps
            bound = (accumulate_bound(S, mag[1 + i, ids]).sum() + len(ids) * 2.0 ** -53 * np.abs(ref[1 + i, ids]).sum()) / steps * (1 + 1e-12) + 1e-300
            if m == "dof_limit_steps":
                assert got[m] == r
            else:
                worst = max(worst, abs(got[m] - r) / bound)
                assert abs(got[m] - r) <= bound, (tname, sname, m, got[m], r, bound)
        assert got["falls"] == ref[9, ids].sum() / len(ids) and got["survival"] == (ref[9, ids] == 0).sum() / len(ids)
    assert res["overall"]["action_rate_sq"] > 0 and res["overall"]["power"] > 0
    print("evaluator vs float64 recomputation: largest gap / bound %.3f; overall %s" % (worst, res["overall"]))
    # the same weights again: bit-identical; other weights: another result
    again = ev.evaluate(ac)
    assert again["table"].tobytes() == res["table"].tobytes()
    other = ev.evaluate(small_actor_critic(1))
    assert other["table"].tobytes() != res["table"].tobytes()
    # an empty group reports NaN means and n_envs = 0
    row = ev._row(np.zeros(GO2NN_EVAL_NUM + 2))
    assert row["n_envs"] == 0 and all(math.isnan(row[k]) for k in RESULT_KEYS if k != "n_envs")
    ev.close()


def test_evaluator_groups_on_a_terrain_task(emu):
    """go2 (trimesh): the kinds are those of the terrain columns, every env stands on the evaluation's level, the scenarios alternate within a kind"""
    ev = make_evaluator(emu, task="go2", num_envs=80, seconds=0.1, warmup_s=0.0)
    env = ev.env
    kinds = env.terrain_cols2id[env.terrain_types].numpy()
    assert len(ev.terrain_names) == len(set(kinds.tolist())) > 1 and len(ev.groups) == len(ev.terrain_names) * 4
    assert (env.terrain_levels == 3).all() and torch.equal(env.env_origins, env.terrain_origins[3, env.terrain_types])
    for ki, k in enumerate(sorted(set(kinds.tolist()))):
        sizes = np.bincount(ev.group_host[kinds == k] - 4 * ki, minlength=4)
        assert sizes.max() - sizes.min() <= 1 and sizes.sum() == (kinds == k).sum()
    res = ev.evaluate(small_actor_critic())
    assert (env.terrain_levels == 3).all()
    assert abs(float((env.root_states[:, :2] - env.env_origins[:, :2]).abs().max())) < 4.0
    assert all(d["n_envs"] > 0 and np.isfinite(d["lin_vel_err"]) for per in res["groups"].values() for d in per.values())
    ev.close()


class Recording:
    """a library (the go2sim oracle or the go2nn host build) with the name of every call an evaluation's steps, begins and reduces are made of appended to one shared list"""
    NAMES = ("go2sim_step", "go2nn_mirror_rows", "go2nn_trace_record", "go2nn_blackbox_record")
    PREFIXES = ("go2nn_eval_", "go2nn_robust_", "go2nn_ladder_", "go2nn_maneuver_", "go2nn_sensor_", "go2nn_gait_", "go2nn_asym_")

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self.NAMES and not name.startswith(self.PREFIXES):
            return fn

        def recorded(*a):
            self._log.append(name)
            return fn(*a)
        return recorded


ADDONS = dict(gait=True, asymmetry=True, record=1, blackbox=1, blackbox_seconds=0.1)
ADDON_BEGINS, ADDON_REDUCES = ["go2nn_gait_begin", "go2nn_asym_begin"], ["go2nn_gait_reduce", "go2nn_asym_reduce"]
ADDON_STEP = ["go2nn_gait_accumulate", "go2nn_asym_accumulate", "go2nn_trace_record", "go2nn_blackbox_record"]
# name -> (task, the mode's options, its calls before the first step, ONE step, its calls after the last): the step sequences of utils/evaluator.py's docstring, written out.
# Before the first step: the reset's zero-action go2sim_step [, the sensor's first frame], go2nn_eval_clear, the tables' begins;  after the last: go2nn_eval_reduce, the tables' reduces
LAUNCH_ORDER = {
    "bare": ("go2_flat", {}, ["go2sim_step", "go2nn_eval_clear"], ["go2sim_step", "go2nn_eval_accumulate"], ["go2nn_eval_reduce"]),
    "plain": ("go2_flat", ADDONS,
              ["go2sim_step", "go2nn_eval_clear"] + ADDON_BEGINS,
              ["go2nn_mirror_rows", "go2sim_step", "go2nn_eval_accumulate"] + ADDON_STEP,
              ["go2nn_eval_reduce"] + ADDON_REDUCES),
    "perturbations": ("go2_flat", dict(ADDONS, perturbations=[["nominal", {}], ["push_front_0.5", {"dv": [0.5, 0.0, 0.0]}]], push_first_s=0.02, push_period_s=0.1, push_window_s=0.1,
                                       recover_hold_s=0.04),
                      ["go2sim_step", "go2nn_eval_clear", "go2nn_robust_begin"] + ADDON_BEGINS,
                      ["go2nn_mirror_rows", "go2nn_robust_apply", "go2sim_step", "go2nn_eval_accumulate", "go2nn_robust_accumulate"] + ADDON_STEP,
                      ["go2nn_eval_reduce", "go2nn_robust_reduce"] + ADDON_REDUCES),
    "sensors": ("go2_flat", dict(ADDONS, sensors=[["nominal", {}], ["delay_1", {"delay": 1}]]),
                ["go2sim_step", "go2nn_sensor_begin", "go2nn_sensor_apply", "go2nn_eval_clear"] + ADDON_BEGINS,
                ["go2nn_mirror_rows", "go2sim_step", "go2nn_sensor_apply", "go2nn_eval_accumulate"] + ADDON_STEP,
                ["go2nn_eval_reduce"] + ADDON_REDUCES),
    "maneuvers": ("go2_flat", dict(ADDONS, maneuvers=[["start_1.0", [[0.0, 0.0, 0.0, 0.0], [0.04, 1.0, 0.0, 0.0]]], ["turn_flip", [[0.0, 0.0, 0.0, 1.0], [0.06, 0.0, 0.0, -1.0]]]],
                                   maneuver_window_s=0.1, maneuver_hold_s=0.04),
                  ["go2sim_step", "go2nn_eval_clear", "go2nn_maneuver_begin"] + ADDON_BEGINS,
                  ["go2nn_mirror_rows", "go2nn_maneuver_apply", "go2sim_step", "go2nn_maneuver_accumulate", "go2nn_eval_accumulate"] + ADDON_STEP,
                  ["go2nn_eval_reduce", "go2nn_maneuver_reduce"] + ADDON_REDUCES),
    "ladder": ("go2", dict(ADDONS, ladder=True, ladder_levels=[0, 4], ladder_distance=0.1),
               ["go2sim_step", "go2nn_eval_clear", "go2nn_ladder_begin"] + ADDON_BEGINS,
               ["go2nn_mirror_rows", "go2sim_step", "go2nn_eval_accumulate", "go2nn_ladder_accumulate"] + ADDON_STEP,
               ["go2nn_eval_reduce", "go2nn_ladder_reduce"] + ADDON_REDUCES),
}


@pytest.mark.parametrize("mode", list(LAUNCH_ORDER))
def test_step_launch_order_of_every_mode(emu, mode):
    """what an evaluation calls, by name and in order: the begins before the first step, the same sequence in every step (warm-up and counted; go2nn_eval_clear once between
    them), the reduces after the last — for the plain evaluation with every add-on off and on, and for each extra axis next to every add-on"""
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    task, over, before, step, after = LAUNCH_ORDER[mode]
    if mode == "ladder":
        from test_ladder_host import SCENARIOS
        over = dict(over, ladder_scenarios=SCENARIOS)
    log, ends = [], []
    env_cfg, _ = task_registry.get_cfgs(task)
    ev = PolicyEvaluator(env_cfg, dict(EVAL, num_envs=38, seconds=0.2, warmup_s=0.1, **over), task_class=task_registry.get_task_class(task), device="cpu",
                         lib=Recording(load_oracle(), log), nn_lib=Recording(emu, log), step_callback=lambda ev, k, counted: ends.append((len(log), counted)))
    del log[:]          # (what building the evaluator called: the specs' checks)
    ev.evaluate(small_actor_critic())
    W, S = ev.warmup_steps, ev.steps
    assert (W, S) == (5, 10) and len(ends) == W + S and [c for _, c in ends] == [False] * W + [True] * S
    assert log[:len(before)] == before
    starts = [len(before)] + [e for e, _ in ends[:-1]]
    slices = [log[a:b] for a, (b, _) in zip(starts, ends)]
    assert slices[W][0] == "go2nn_eval_clear"          # the boundary: the warm-up's sums go, once
    slices[W] = slices[W][1:]
    assert slices[W] == step, (mode, slices[W])          # a counted step
    assert all(s == step for s in slices), (mode, [s for s in slices if s != step][:1])
    assert log[ends[-1][0]:] == after
    assert not any(n.endswith("_begin") for s in slices for n in s) and not any(n.endswith("_reduce") for n in log[:ends[-1][0]])
    ev.close()


def _snapshot(env, runner):
    alg = runner.alg
    snap = {"buf." + k: v.detach().clone() for k, v in env._buf.items()}
    snap["counter"] = torch.tensor(env.common_step_counter)
    rcs, cr, zp = env._curriculum_state()
    snap["curriculum"] = torch.tensor(list(rcs) + [x for r in cr for x in r] + [zp], dtype=torch.float64)
    for n, p in alg.actor_critic.state_dict().items():
        snap["model." + n] = p.detach().clone()
    opts = [getattr(alg, n) for n in ("optimizer", "optimizer1", "optimizer2") if hasattr(alg, n)]
    for oi, opt in enumerate(opts):
        for pi, st in enumerate(opt.state_dict()["state"].values()):
            for k, v in st.items():
                snap["opt%d.%d.%s" % (oi, pi, k)] = torch.as_tensor(v).detach().clone()
    for owner, tag in ((alg, "alg"), (getattr(alg, "storage", None), "storage")):
        for k, v in (vars(owner).items() if owner is not None else ()):
            if torch.is_tensor(v):
                snap["%s.%s" % (tag, k)] = v.detach().clone()
    snap["torch_cpu_rng"] = torch.get_rng_state().clone()
    if torch.cuda.is_available():
        snap["torch_cuda_rng"] = torch.cuda.get_rng_state().clone()
    snap["numpy_rng"] = torch.from_numpy(np.random.get_state()[1].astype(np.int64))
    return snap


def assert_same_snapshot(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype and x.cpu().contiguous().reshape(-1).numpy().tobytes() == y.cpu().contiguous().reshape(-1).numpy().tobytes(), k


def test_evaluation_leaves_the_training_run_untouched(emu, tmp_path):
    args = get_args(["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"])
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    runner.learn(1, init_at_random_ep_len=True)
    assert runner.evaluator is None
    runner.eval_cfg = dict(EVAL, num_envs=12, seconds=0.2)
    runner.evaluator_kwargs = {"nn_lib": emu}
    before = _snapshot(env, runner)
    res = runner.update_evaluation(0, False)
    assert res is not None and runner.evaluator is not None and runner.evaluator.env is not env
    assert_same_snapshot(before, _snapshot(env, runner))
    runner.learn(1)          # ... and the run goes on
    env.close()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_runner_hook_and_cli(emu, tmp_path, task):
    from go2_rl_gym_amd.utils.evaluator import RESULT_KEYS
    base = ["--task", task, "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    # defaults: evaluation off, --robogauge parsed and ignored, save() creates no evaluator
    args = get_args(base + ["--robogauge"])
    assert args.evaluate is False and args.eval_interval is None
    env, _ = task_registry.make_env(task, args, lib=load_oracle())
    runner, train_cfg = task_registry.make_alg_runner(env, task, args, log_root=str(tmp_path / "off"))
    assert train_cfg.evaluation.enabled is False and train_cfg.evaluation.interval == 500 and train_cfg.evaluation.num_envs == 1024
    runner.learn(1)
    assert runner.evaluator is None and not os.path.exists(os.path.join(runner.log_dir, "eval_results"))
    env.close()
    # --evaluate --eval_interval 2: three iterations write results_0, results_2 and the last model's file
    args = get_args(base + ["--evaluate", "--eval_interval", "2"])
    env, _ = task_registry.make_env(task, args, lib=load_oracle())
    _, train_cfg = task_registry.get_cfgs(task)
    train_cfg.runner.save_interval = 1
    train_cfg.evaluation.num_envs, train_cfg.evaluation.seconds, train_cfg.evaluation.warmup_s = 12, 0.2, 0.1
    runner, train_cfg = task_registry.make_alg_runner(env, train_cfg=train_cfg, args=args, log_root=str(tmp_path / "on"))
    assert train_cfg.evaluation.enabled is True and train_cfg.evaluation.interval == 2
    runner.evaluator_kwargs = {"nn_lib": emu}
    tags = []
    runner.writer = type("W", (), {"add_scalar": lambda self, tag, v, step: tags.append((tag, step))})()
    runner.learn(3)
    last = "results_%d.yaml" % runner.current_learning_iteration
    files = sorted(os.listdir(os.path.join(runner.log_dir, "eval_results")))
    assert files == sorted({"results_0.yaml", "results_2.yaml", last}) and last == "results_3.yaml"
    d = yaml.safe_load(open(os.path.join(runner.log_dir, "eval_results", "results_2.yaml")))
    assert d["iteration"] == 2 and set(d["overall"]) == set(RESULT_KEYS) and set(d["groups"]) == {"plane"}
    assert set(d["groups"]["plane"]) == {"forward_1.0", "forward_2.0", "backward_1.0", "lateral_0.5", "turn_1.0", "stand"}
    assert all(set(v) == set(RESULT_KEYS) for v in d["groups"]["plane"].values())
    ev_tags = {t for t, _ in tags if t.startswith("Eval/")}
    assert "Eval/lin_vel_err" in ev_tags and "Eval/plane/forward_1.0/speed_along_cmd" in ev_tags and "Eval/survival" in ev_tags
    assert {s for t, s in tags if t == "Eval/lin_vel_err"} == {0, 2, 3}
    env.close()
