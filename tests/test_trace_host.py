"""The trajectory recorder on the CPU: the host build of go2nn_trace_record (include/go2nn.h) against a numpy gather written here — every column is a copy, so every
comparison is exact —, the ring and its device-side cursor, TrajectoryRecorder on the oracle + the host build, what the host side makes of a trace (MuJoCo qpos, gait
summary, the .npz), and where the recorder plugs in (evaluator, runner hook, CLI)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, load_emu, load_nn_emu, load_oracle
import test_eval_host as th
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import GO2NN_TRACE_WIDTH, TRACE_BLOCKS, TRACE_FIELDS, TRACE_OFFSET, Go2nnTraceIn
from go2_rl_gym_amd.envs import task_registry
from go2_rl_gym_amd.utils import get_args
from go2_rl_gym_amd.utils import recorder as R

SHAPES = {"root_states": (13,), "dof_state": (12, 2), "torques": (12,), "actions": (12,), "commands": (4,), "base_lin_vel": (3,), "base_ang_vel": (3,),
          "projected_gravity": (3,), "rigid_body_states": (19, 13), "contact_forces": (19, 3), "rew_buf": (), "reset_buf": (), "time_out_buf": ()}
FEET = [6, 10, 14, 18]
EINVAL = -22


def random_buffers(rng, N):
    """one step's source buffers in their LOGICAL shapes [N, ...]"""
    d = {k: rng.normal(0, 1, (N,) + s).astype(np.float32) for k, s in SHAPES.items()}
    d["reset_buf"] = (rng.random(N) < 0.3).astype(np.uint8)
    d["time_out_buf"] = (d["reset_buf"] & (rng.random(N) < 0.5)).astype(np.uint8)
    return d


def gather(d, ids, feet=FEET):
    """the frame table of include/go2nn.h as a numpy gather -> fp32 [K, 112]"""
    g = {k: np.asarray(v)[ids] for k, v in d.items()}
    K = len(ids)
    rb, cf = g["rigid_body_states"][:, feet], g["contact_forces"][:, feet]
    cols = [g["root_states"][:, 0:3], g["root_states"][:, 3:7], g["root_states"][:, 7:10], g["root_states"][:, 10:13], g["dof_state"][:, :, 0], g["dof_state"][:, :, 1],
            g["torques"], g["actions"], g["commands"][:, :3], g["base_lin_vel"], g["base_ang_vel"], g["projected_gravity"], rb[:, :, 0:3].reshape(K, 12),
            rb[:, :, 7:10].reshape(K, 12), cf.reshape(K, 12), g["rew_buf"][:, None], g["reset_buf"][:, None] != 0, g["time_out_buf"][:, None] != 0]
    assert [c.shape[1] for c in cols] == [w for _, w in TRACE_BLOCKS]
    return np.concatenate([c.astype(np.float32) for c in cols], 1)


def pack(d, layout):
    """the buffers as the libraries store them (layout 1: field-major, [N, a, b] kept as [b, a, N]) -> ({name: storage}, {name: strides of the logical view in elements})"""
    store, strides = {}, {}
    for k, a in d.items():
        if layout == 1 and a.ndim > 1:
            store[k] = np.ascontiguousarray(a.transpose())
            view = store[k].transpose()
        else:
            store[k] = view = np.ascontiguousarray(a)
        assert view.shape == a.shape
        strides[k] = tuple(s // a.itemsize for s in view.strides)
    return store, strides


def trace_in(ptr_of, strides, feet=FEET):
    a = Go2nnTraceIn()
    for k in TRACE_FIELDS:
        f, st = getattr(a, k), strides[k]
        f.p, f.env_stride, f.comp_stride = ptr_of(k), st[0], (st[-1] if len(st) > 1 else 0)
    a.dof_state.comp_stride, a.dof_vel_offset = strides["dof_state"][1], strides["dof_state"][2]
    a.rigid_body_stride, a.contact_body_stride = strides["rigid_body_states"][1], strides["contact_forces"][1]
    a.foot_body[:] = feet
    return a


def tracked(rng, N, kind):
    if kind == "one":
        return np.asarray([N // 2], np.int32)
    if kind == "all":
        return np.arange(N, dtype=np.int32)
    return np.sort(rng.choice(N, size=min(N, 5), replace=False)).astype(np.int32)


def record_case(call, N, layout, kind, T=4, calls=3, seed=0):
    """call(store, strides, ids, frames, cursor) runs one go2nn_trace_record on a library and returns (frames, cursor) as numpy; -> nothing, asserts"""
    rng = np.random.default_rng(seed + 31 * N + layout)
    ids = tracked(rng, N, kind)
    frames = np.full((T, len(ids), GO2NN_TRACE_WIDTH), np.nan, np.float32)
    cursor = np.zeros(1, np.int32)
    want = frames.copy()
    for c in range(calls):
        d = random_buffers(rng, N)
        want[c % T] = gather(d, ids)
        frames, cursor = call(*pack(d, layout), ids, frames, cursor)
        assert cursor[0] == c + 1
        np.testing.assert_array_equal(frames, want)
    assert np.isnan(frames[calls:]).all() and (kind != "all" or N == 1 or set(np.unique(want[:calls, :, TRACE_OFFSET["reset"]])) == {0.0, 1.0})


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


def emu_call(emu):
    def call(store, strides, ids, frames, cursor):
        a = trace_in(lambda k: store[k].ctypes.data, strides)
        rc = emu.go2nn_trace_record(C.byref(a), C.c_void_p(ids.ctypes.data), len(ids), C.c_void_p(frames.ctypes.data), C.c_void_p(cursor.ctypes.data), frames.shape[0], None)
        assert rc == 0, emu.go2nn_last_error()
        return frames, cursor
    return call


@pytest.mark.parametrize("kind", ["one", "several", "all"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [1, 17, 257])
def test_record_is_a_gather(emu, N, layout, kind):
    record_case(emu_call(emu), N, layout, kind)


def test_frame_table_matches_the_header(emu, tmp_path):
    """the enum of include/go2nn.h, Go2nnTraceIn as gcc sees it, and their restatements in _nn.py"""
    assert emu.go2nn_abi_version() == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert " T go2nn_trace_record\n" in syms and " T go2nn_trace_clear\n" in syms, path
    names = list(TRACE_FIELDS) + ["dof_vel_offset", "rigid_body_stride", "contact_body_stride", "foot_body"]
    blocks = [b for b, _ in TRACE_BLOCKS]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu %d", sizeof(Go2nnTraceIn), GO2NN_TRACE_WIDTH);\n'
                   + "".join('printf(" %%zu", offsetof(Go2nnTraceIn, %s));\n' % n for n in names)
                   + "".join('printf(" %%d", GO2NN_TRACE_%s);\n' % b.upper() for b in blocks) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:2] == [C.sizeof(Go2nnTraceIn), GO2NN_TRACE_WIDTH] and GO2NN_TRACE_WIDTH == 112
    assert got[2:2 + len(names)] == [getattr(Go2nnTraceIn, n).offset for n in names]
    assert got[2 + len(names):] == [TRACE_OFFSET[b] for b in blocks]
    cols = R.column_names(["j%d" % i for i in range(12)], ["a", "b", "c", "d"])
    assert len(cols) == len(set(cols)) == 112 and cols[TRACE_OFFSET["root_quat"] + 3] == "root_quat.w" and cols[TRACE_OFFSET["foot_force"] + 5] == "foot_force.b.z"


def test_ring_and_cursor(emu):
    """T = 5, 12 calls: the slots hold steps 7 .. 11, step s in slot s % 5; clear sets the cursor to 0 and leaves the frames"""
    N, T, rng = 9, 5, np.random.default_rng(5)
    ids = np.asarray([1, 4, 8], np.int32)
    frames, cursor = np.zeros((T, 3, GO2NN_TRACE_WIDTH), np.float32), np.zeros(1, np.int32)
    call, steps = emu_call(emu), []
    for s in range(12):
        d = random_buffers(rng, N)
        steps.append(gather(d, ids))
        call(*pack(d, s % 2), ids, frames, cursor)
    assert cursor[0] == 12
    for s in range(7, 12):
        np.testing.assert_array_equal(frames[s % T], steps[s])
    kept = frames.copy()
    assert emu.go2nn_trace_clear(C.c_void_p(cursor.ctypes.data), None) == 0 and cursor[0] == 0
    np.testing.assert_array_equal(frames, kept)


def test_rejected_arguments(emu):
    N = 4
    d = random_buffers(np.random.default_rng(0), N)
    store, strides = pack(d, 0)
    ids, frames, cursor = np.arange(2, dtype=np.int32), np.zeros((3, 2, GO2NN_TRACE_WIDTH), np.float32), np.zeros(1, np.int32)
    good = lambda: trace_in(lambda k: store[k].ctypes.data, strides)          # noqa: E731

    def run(a, ids_p=ids.ctypes.data, K=2, frames_p=frames.ctypes.data, cursor_p=cursor.ctypes.data, T=3):
        rc = emu.go2nn_trace_record(C.byref(a) if a is not None else None, C.c_void_p(ids_p), K, C.c_void_p(frames_p), C.c_void_p(cursor_p), T, None)
        return rc, emu.go2nn_last_error().decode()
    assert run(good())[0] == 0 and cursor[0] == 1
    cases = [run(None), run(good(), ids_p=None), run(good(), frames_p=None), run(good(), cursor_p=None), run(good(), K=0), run(good(), T=0), run(Go2nnTraceIn())]
    for mutate in ("env", "comp", "body", "vel", "foot", "ptr"):
        a = good()
        if mutate == "env":
            a.torques.env_stride = 0
        elif mutate == "comp":
            a.root_states.comp_stride = 0
        elif mutate == "body":
            a.rigid_body_stride = 0
        elif mutate == "vel":
            a.dof_vel_offset = 0
        elif mutate == "foot":
            a.foot_body[2] = -1
        else:
            a.rew_buf.p = None
        cases.append(run(a))
    for rc, msg in cases:
        assert rc == EINVAL and msg.startswith("trace record"), (rc, msg)
    assert cursor[0] == 1 and not frames[1:].any()          # a refused call writes nothing
    assert emu.go2nn_trace_clear(None, None) == EINVAL and emu.go2nn_last_error().decode().startswith("trace clear")
    # the tracked robots are checked by the binding: the kernel cannot report a bad index
    np.testing.assert_array_equal(_nn.trace_env_ids([0, 2, 3], N), np.asarray([0, 2, 3], np.int32))
    assert _nn.trace_env_ids(range(N), N).dtype == np.int32 and _nn.trace_env_ids(torch.tensor([1, 3]), N).tolist() == [1, 3]
    for bad in ([2, 1], [1, 1], [0, N], [-1, 0], [], [[0, 1]], [0.5, 1.5]):
        with pytest.raises(ValueError):
            _nn.trace_env_ids(bad, N)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def make_env(task="go2_flat", N=8, lib=None, episode_length_s=None):
    args = get_args(["--task", task, "--num_envs", str(N), "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "3"])
    env_cfg, _ = task_registry.get_cfgs(task)
    if episode_length_s is not None:
        env_cfg.env.episode_length_s = episode_length_s
    env, _ = task_registry.make_env(task, args, env_cfg=env_cfg, lib=lib or load_oracle())
    return env, args


def snapshot(env):
    return {k: env._buf[k].detach().clone().numpy() for k in TRACE_FIELDS}


@pytest.mark.parametrize("sim", ["oracle", "field_major_host_build"])
def test_recorder_on_host_libraries(emu, sim):
    """go2_flat, 8 envs, 30 steps: the fetched trace against per-step numpy snapshots of the same buffers — on the oracle's row-major buffers and on the host build of the
    HIP simulator, whose torch views are the field-major transposes the device library has.  Episodes of 0.3 s: every robot times out inside the record, so frames with
    the reset and time-out flags set occur."""
    env, _ = make_env(lib=load_oracle() if sim == "oracle" else load_emu(), episode_length_s=0.3)
    assert env.lib.go2sim_buffer_layout() == (0 if sim == "oracle" else 1)
    with pytest.raises(RuntimeError, match="nn_lib"):
        R.TrajectoryRecorder(env, [0, 1], 4)          # no CPU product path
    for bad in ([3, 1], [0, 8], []):
        with pytest.raises(ValueError):
            R.TrajectoryRecorder(env, bad, 4, nn_lib=emu)
    ids = [0, 3, 4, 7]
    rec = R.TrajectoryRecorder(env, ids, 30, nn_lib=emu)
    ring = R.TrajectoryRecorder(env, ids, 5, nn_lib=emu)
    torch.manual_seed(0)
    want = []
    for s in range(30):
        env.step(torch.randn(8, 12) * 0.5)
        rec.record(); ring.record()
        want.append(gather(snapshot(env), ids, [int(i) for i in env.feet_indices]))
    tr = rec.fetch()
    want = np.stack(want)
    np.testing.assert_array_equal(tr["frames"], want)
    assert tr["steps_recorded"] == 30 and tr["frames"].shape == (30, 4, 112) and tr["env_ids"].tolist() == ids and tr["dt"] == env.dt
    assert tr["dof_names"] == env.dof_names and tr["foot_names"] == ["FL_foot", "FR_foot", "RL_foot", "RR_foot"] and len(tr["columns"]) == 112
    assert tr["reset"].dtype == bool and tr["reset"].any() and tr["time_out"].any() and not tr["reset"].all() and tr["foot_force"].shape == (30, 4, 4, 3) and tr["reward"].shape == (30, 4)
    np.testing.assert_array_equal(tr["foot_force"], want[:, :, TRACE_OFFSET["foot_force"]:TRACE_OFFSET["reward"]].reshape(30, 4, 4, 3))
    np.testing.assert_array_equal(tr["root_quat"], want[:, :, 3:7])
    assert np.abs(np.linalg.norm(tr["root_quat"], axis=-1) - 1).max() < 1e-5 and tr["foot_force"][..., 2].max() > 1.0
    # the ring of 5 holds the steps 25 .. 29, returned in time order; after clear() the cursor is 0 and the next step is step 0
    last = ring.fetch()
    assert last["steps_recorded"] == 30 and int(ring.cursor[0]) == 30
    np.testing.assert_array_equal(last["frames"], want[25:])
    ring.clear()
    assert int(ring.cursor[0]) == 0 and ring.fetch()["frames"].shape == (0, 4, 112)
    env.step(torch.zeros(8, 12)); ring.record()
    np.testing.assert_array_equal(ring.fetch()["frames"][0], gather(snapshot(env), ids))
    env.close()


def hand_made_trace(S=100, K=2, dt=0.02):
    """robot 0: feet 0 and 2 with period 10 frames / 6 in contact, feet 1 and 3 with period 20 / 10 in contact, a reset flag on frame 50; robot 1 stands"""
    z = lambda *s: np.zeros(s, np.float32)          # noqa: E731
    tr = {"foot_force": z(S, K, 4, 3), "foot_pos": z(S, K, 4, 3), "foot_vel": z(S, K, 4, 3), "reset": np.zeros((S, K), bool), "dt": dt,
          "foot_names": ["FL_foot", "FR_foot", "RL_foot", "RR_foot"], "env_ids": np.asarray([2, 5], np.int32)}
    t = np.arange(S)
    for f in range(4):
        period, stance, top = (10, 6, 0.125) if f % 2 == 0 else (20, 10, 0.25)
        phase = t % period
        contact = phase < stance
        tr["foot_force"][:, 0, f, 2] = np.where(contact, 40.0, 0.5)                 # 0.5 N in swing: below the 1 N rule
        tr["foot_force"][:, 0, f, 0] = 7.0                                           # horizontal force never counts
        tr["foot_vel"][:, 0, f, 0] = np.where(contact, 0.75, 2.0)
        tr["foot_vel"][:, 0, f, 1] = np.where(contact, 1.0, 0.0)                    # |(0.75, 1.0)| = 1.25 in stance
        tr["foot_vel"][:, 0, f, 2] = 9.0                                             # vertical speed is no slip
        mid = (phase == (stance + period) // 2) | (phase == (stance + period) // 2 - 1)
        tr["foot_pos"][:, 0, f, 2] = np.where(contact, 0.02, np.where(mid, top, top / 2))
    tr["reset"][50, 0] = True
    tr["foot_pos"][50, 0, :, 2] = 5.0          # the skipped frame's content is never looked at
    tr["foot_force"][:, 1, :, 2] = 30.0
    return tr


def test_gait_summary_on_a_known_pattern():
    """Worked by hand.  Robot 0, segments [0, 50) and [51, 100) around the reset frame.
    Feet 0, 2 (contact when t % 10 < 6): touchdowns at 10, 20, 30, 40 and 60, 70, 80, 90 (the stances that open a segment are not touchdowns) = 8, stride 10 frames;
    eight complete stances of 6 frames, eight complete swings of 4; contact frames 30 + 29 of 99 used.
    Feet 1, 3 (contact when t % 20 < 10): touchdowns at 20, 40 and 60, 80 = 4, stride 20 frames; complete stances [20, 30), [60, 70), [80, 90) (the one at 40 is cut by the
    reset), complete swings [10, 20), [30, 40), [70, 80); contact frames 30 + 20 of 99."""
    tr = hand_made_trace()
    g = R.gait_summary(tr)
    dt = 0.02
    assert g["frames_used"].tolist() == [99, 100]
    assert g["touchdowns"].tolist() == [[8, 4, 8, 4], [0, 0, 0, 0]]
    np.testing.assert_array_equal(g["duty_factor"], [[59 / 99, 50 / 99] * 2, [1.0] * 4])
    np.testing.assert_array_equal(g["stride_frequency"][0], [1.0 / (10.0 * dt), 1.0 / (20.0 * dt)] * 2)
    np.testing.assert_array_equal(g["stance_time"][0], [6.0 * dt, 10.0 * dt] * 2)
    np.testing.assert_array_equal(g["swing_time"][0], [4.0 * dt, 10.0 * dt] * 2)
    np.testing.assert_array_equal(g["slip_speed"], [[1.25] * 4, [0.0] * 4])
    np.testing.assert_array_equal(g["swing_height"][0], [0.125, 0.25] * 2)
    assert all(np.isnan(g[k][1]).all() for k in ("stride_frequency", "stance_time", "swing_time", "swing_height"))
    # without the reset flag the cut stance is whole again, and a higher threshold empties the contact set
    tr["reset"][:] = False
    tr["foot_pos"][50, 0, :, 2] = 0.02
    g2 = R.gait_summary(tr)
    assert g2["touchdowns"].tolist()[0] == [9, 4, 9, 4] and g2["duty_factor"][0].tolist() == [0.6, 0.5, 0.6, 0.5] and g2["stance_time"][0, 1] == 10.0 * dt
    g3 = R.gait_summary(tr, contact_threshold=50.0)
    assert not g3["touchdowns"].any() and (g3["duty_factor"] == 0).all() and np.isnan(g3["slip_speed"]).all()
    assert len(R.format_gait(tr)) == 2 and R.format_gait(tr)[0].startswith("env 2: FL duty 0.60 stride 5.00 Hz")


def test_mujoco_qpos_is_wxyz():
    tr = {"root_pos": np.asarray([[[1.0, 2.0, 3.0]]], np.float32), "root_quat": np.asarray([[[0.1, 0.2, 0.3, 0.9]]], np.float32),
          "dof_pos": np.arange(12, dtype=np.float32).reshape(1, 1, 12) + 10}
    q = R.mujoco_qpos(tr)
    assert q.shape == (1, 1, 19) and q.dtype == np.float32
    np.testing.assert_array_equal(q[0, 0], np.asarray([1.0, 2.0, 3.0, 0.9, 0.1, 0.2, 0.3] + list(range(10, 22)), np.float32))
    assert "wxyz" in R.mujoco_qpos.__doc__.lower() and "go2.yaml" in R.mujoco_qpos.__doc__


def test_trace_file_round_trip(emu, tmp_path):
    env, _ = make_env()
    rec = R.TrajectoryRecorder(env, [1, 2, 6], 12, nn_lib=emu)
    torch.manual_seed(1)
    for _ in range(12):
        env.step(torch.randn(8, 12))
        rec.record()
    tr = rec.fetch()
    path = R.write_trace(str(tmp_path / "sub" / "t.npz"), tr, extra={"group_of_robot": np.asarray([0, 1, 1]), "scenarios": ["a", "bb"], "iteration": 7})
    back = R.read_trace(path)
    assert set(back) == set(tr) | {"qpos", "gait", "group_of_robot", "scenarios", "iteration"}
    for k, v in tr.items():
        if isinstance(v, np.ndarray):
            assert back[k].dtype == v.dtype
            np.testing.assert_array_equal(back[k], v)
        else:
            assert back[k] == v and type(back[k]) is type(v), k
    assert back["columns"] == R.column_names(env.dof_names, tr["foot_names"]) and back["scenarios"] == ["a", "bb"] and back["iteration"] == 7
    np.testing.assert_array_equal(back["qpos"], R.mujoco_qpos(tr))
    gait = R.gait_summary(tr)
    assert set(back["gait"]) == set(gait) == set(R.GAIT_KEYS) | {"frames_used"}
    for k in gait:
        np.testing.assert_array_equal(back["gait"][k], gait[k])
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_records_without_touching_the_scores(emu):
    ac = th.small_actor_critic()
    off = th.make_evaluator(emu)
    assert off.recorder is None
    base = off.evaluate(ac)
    assert "trace" not in base
    off.close()
    snaps = []

    def cb(ev, k, counted):
        if counted:
            snaps.append({n: ev.env._buf[n].detach().clone().numpy() for n in ("commands", "base_lin_vel")})
    ev = th.make_evaluator(emu, cb=cb, record=2)
    res = ev.evaluate(ac)
    assert res["table"].tobytes() == base["table"].tobytes()
    tr, G, S = res["trace"], len(ev.groups), ev.steps
    assert S == 50 and G == 4 and tr["frames"].shape == (S, 2 * G, 112) and tr["steps_recorded"] == S and int(ev.recorder.cursor[0]) == S
    first_two = np.sort(np.concatenate([np.nonzero(ev.group_host == g)[0][:2] for g in range(G)]))
    assert tr["env_ids"].tolist() == first_two.tolist() and tr["group_of_robot"].tolist() == ev.group_host[first_two].tolist()
    assert sorted(tr["group_of_robot"].tolist()) == [g for g in range(G) for _ in range(2)]
    assert tr["terrain_names"] == ["plane"] and tr["scenarios"] == [s[0] for s in th.EVAL["scenarios"]] and tr["dt"] == ev.dt
    want_cmd = np.asarray([s[1:4] for s in th.EVAL["scenarios"]], np.float32)[tr["group_of_robot"] % len(th.EVAL["scenarios"])]
    np.testing.assert_array_equal(tr["commands"], np.broadcast_to(want_cmd, (S, 2 * G, 3)))
    # a figure the scores report, recomputed for single robots: the mean of |cmd_xy - v_xy| over the counted frames, in float64 from the step callback's snapshots
    assert len(snaps) == S
    for k, e in enumerate(tr["env_ids"]):
        got = np.linalg.norm(tr["commands"][:, k, :2].astype(np.float64) - tr["base_lin_vel"][:, k, :2].astype(np.float64), axis=1).mean()
        ref = np.mean([np.linalg.norm(s["commands"][e, :2].astype(np.float64) - s["base_lin_vel"][e, :2].astype(np.float64)) for s in snaps])
        assert got == ref and got > 0
    # every evaluation starts the record anew; the same weights give the same trace
    again = ev.evaluate(ac)
    assert again["table"].tobytes() == base["table"].tobytes() and again["trace"]["frames"].tobytes() == tr["frames"].tobytes()
    ev.close()


def test_runner_hook_writes_the_trace_and_cli_defaults(emu, tmp_path):
    base = ["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    assert args.record is None and args.record_steps == 500
    for task in ("go2_flat", "go2_flat_cts"):
        _, train_cfg = task_registry.get_cfgs(task)
        assert train_cfg.evaluation.record == 0
    args = get_args(base + ["--evaluate", "--eval_interval", "1", "--record", "1"])
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    train_cfg.evaluation.num_envs, train_cfg.evaluation.seconds, train_cfg.evaluation.warmup_s = 12, 0.2, 0.1
    runner, train_cfg = task_registry.make_alg_runner(env, train_cfg=train_cfg, args=args, log_root=str(tmp_path))
    assert train_cfg.evaluation.record == 1 and runner.eval_cfg["record"] == 1
    runner.evaluator_kwargs = {"nn_lib": emu}
    res = runner.update_evaluation(0, False)
    files = sorted(os.listdir(os.path.join(runner.log_dir, "eval_results")))
    assert files == ["results_0.yaml", "trace_0.npz"]
    back = R.read_trace(os.path.join(runner.log_dir, "eval_results", "trace_0.npz"))
    assert back["frames"].shape == (10, 6, 112) and back["scenarios"] == res["trace"]["scenarios"] and back["terrain_names"] == ["plane"]
    np.testing.assert_array_equal(back["frames"], res["trace"]["frames"])
    np.testing.assert_array_equal(back["group_of_robot"], np.arange(6))
    import yaml
    assert "trace" not in yaml.safe_load(open(os.path.join(runner.log_dir, "eval_results", "results_0.yaml")))
    env.close()


def test_play_without_the_flag_is_unchanged(emu, tmp_path, monkeypatch):
    """play() on the oracle (the test hands the library in; the product has no CPU path): without --record it returns (env, exported) as before and writes no trace;
    with it, on a host library, the recorder refuses — it needs the go2nn host build, which only tests hand in"""
    from go2_rl_gym_amd.scripts import play as P
    base = ["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1)
    env.close()
    inner = task_registry.make_env
    monkeypatch.setattr(task_registry, "make_env", lambda *a, **k: inner(*a, lib=load_oracle(), **k))
    env, exported = P.play(get_args(base), steps=3, log_root=str(tmp_path), export_policy=False)
    assert exported is None and not hasattr(env, "trace_path") and not os.path.exists(os.path.join(str(tmp_path), "exported"))
    assert torch.isfinite(env.obs_buf).all()
    env.close()
    with pytest.raises(RuntimeError, match="nn_lib"):
        P.play(get_args(base + ["--record", "2", "--record_steps", "3"]), steps=3, log_root=str(tmp_path), export_policy=False)
