"""The trajectory recorder on a real MI355X: the device build of go2nn_trace_record against the host build on the same buffers (every column is a copy: bit-identical),
TrajectoryRecorder on a real simulator against per-step clones, the evaluator's record inside a replayed HIP graph, scripts/play.py --record, and what the gait summary
says about a policy that is known to walk.  Run with -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip, load_nn_emu  # noqa: E402
import test_trace_host as tt  # noqa: E402
from go2_rl_gym_amd._nn import GO2NN_TRACE_WIDTH, TRACE_FIELDS  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils import get_args  # noqa: E402
from go2_rl_gym_amd.utils import recorder as R  # noqa: E402

DEV = "cuda:0"
SMALL = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True)


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.fixture(scope="module")
def nn(hip):
    from go2_rl_gym_amd._nn import load_nn
    return load_nn()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("kind", ["several", "all"])
@pytest.mark.parametrize("N", [17, 4096])
def test_record_kernel_equals_the_host_build(nn, N, kind):
    """field-major buffers, the same calls on both builds: the device ring and cursor are the host build's, bit for bit (and both are the numpy gather of record_case)"""
    emu = load_nn_emu()
    host_call = tt.emu_call(emu)
    state = {}

    def call(store, strides, ids, frames, cursor):
        if not state:
            state["frames"], state["cursor"] = torch.from_numpy(frames.copy()).to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            state["ids"], state["host"] = torch.from_numpy(ids).to(DEV), (frames.copy(), cursor.copy())
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in store.items()}
        a = tt.trace_in(lambda k: dev[k].data_ptr(), strides)
        rc = nn.go2nn_trace_record(C.byref(a), C.c_void_p(state["ids"].data_ptr()), len(ids), C.c_void_p(state["frames"].data_ptr()), C.c_void_p(state["cursor"].data_ptr()),
                                   frames.shape[0], _st())
        assert rc == 0, nn.go2nn_last_error()
        torch.cuda.synchronize()
        state["host"] = host_call(store, strides, ids, *state["host"])
        got = state["frames"].cpu().numpy(), state["cursor"].cpu().numpy()
        assert got[0].tobytes() == state["host"][0].tobytes() and got[1].tolist() == state["host"][1].tolist()
        return got
    tt.record_case(call, N, 1, kind, T=3, calls=5)
    assert nn.go2nn_trace_clear(C.c_void_p(state["cursor"].data_ptr()), _st()) == 0 and int(state["cursor"].item()) == 0
    bad = tt.trace_in(lambda k: 0, {k: (1,) * (1 + len(s)) for k, s in tt.SHAPES.items()})
    assert nn.go2nn_trace_record(C.byref(bad), C.c_void_p(state["ids"].data_ptr()), 1, C.c_void_p(state["frames"].data_ptr()), C.c_void_p(state["cursor"].data_ptr()), 3,
                                 _st()) == tt.EINVAL


def test_recorder_on_a_real_simulator(hip):
    """go2_flat, 64 envs, 50 eager steps: the fetched trace against per-step clones of the same buffers; the ring of 7 keeps the last 7 of them"""
    args = get_args(["--task", "go2_flat", "--num_envs", "64", "--headless", "--seed", "3"])
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    env_cfg.env.episode_length_s = 0.5          # time-outs inside the record: frames with the reset flag occur
    env, _ = task_registry.make_env("go2_flat", args, env_cfg=env_cfg)
    ids = [0, 1, 17, 40, 63]
    rec, ring = R.TrajectoryRecorder(env, ids, 50), R.TrajectoryRecorder(env, ids, 7)
    torch.manual_seed(0)
    clones = []
    for _ in range(50):
        env.step(torch.randn(64, 12, device=DEV) * 0.5)
        rec.record(); ring.record()
        clones.append({k: env._buf[k].clone() for k in TRACE_FIELDS})
    tr, last = rec.fetch(), ring.fetch()
    feet = [int(i) for i in env.feet_indices.tolist()]
    want = np.stack([tt.gather({k: v.cpu().numpy() for k, v in c.items()}, ids, feet) for c in clones])
    assert tr["frames"].shape == (50, 5, GO2NN_TRACE_WIDTH) and tr["frames"].tobytes() == want.tobytes()
    assert tr["steps_recorded"] == last["steps_recorded"] == 50 and last["frames"].tobytes() == want[43:].tobytes()
    assert tr["reset"].any() and tr["time_out"].any() and not tr["reset"].all() and tr["foot_force"][..., 2].max() > 1.0
    env.close()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_record_inside_the_replayed_graph(hip, monkeypatch, task):
    """record = 2 with replay: the captured chunk's record call lands in a new slot on every replay — the second (captured) evaluation's trace is the first (eager)
    one's, byte for byte —, the cursor counts the counted steps, and the scores are those of record = 0"""
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    args = get_args(["--task", task, "--num_envs", "64", "--headless"])
    env, _ = task_registry.make_env(task, args)
    runner, _ = task_registry.make_alg_runner(env, task, args, log_root=None)
    ac = runner.alg.actor_critic
    make = lambda **kw: PolicyEvaluator(env.cfg, dict(SMALL, **kw), task_class=type(env), sim_params=env.sim_params, device=env.sim_device)          # noqa: E731
    off = make()
    assert off.recorder is None
    base = off.evaluate(ac, use_graph=False)
    off.close()
    ev = make(record=2)
    eager = ev.evaluate(ac, use_graph=False)
    assert int(ev.recorder.cursor.item()) == ev.steps
    replay = ev.evaluate(ac)
    assert (eager["mode"], replay["mode"]) == ("eager", "graph") and ev.chunk == 25 and int(ev.recorder.cursor.item()) == ev.steps == 100
    G = len(ev.groups)
    for res in (eager, replay):
        assert res["table"].tobytes() == base["table"].tobytes()
        assert res["trace"]["frames"].shape == (ev.steps, 2 * G, GO2NN_TRACE_WIDTH) and res["trace"]["steps_recorded"] == ev.steps
    assert replay["trace"]["frames"].tobytes() == eager["trace"]["frames"].tobytes()
    tr = eager["trace"]
    assert np.isfinite(tr["frames"]).all() and len({f.tobytes() for f in tr["frames"]}) == ev.steps          # every slot holds another step
    want_cmd = np.asarray([s[1:4] for s in ev.scenarios], np.float32)[tr["group_of_robot"] % len(ev.scenarios)]
    assert (tr["commands"] == want_cmd[None]).all()
    ev.close(); env.close()


def test_play_records_the_last_steps(hip, tmp_path, capsys):
    from go2_rl_gym_amd.scripts.play import play
    args = get_args(["--task", "go2_flat", "--num_envs", "256", "--headless"])
    env, _ = task_registry.make_env("go2_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1, init_at_random_ep_len=True)
    env.close()
    args = get_args(["--task", "go2_flat", "--num_envs", "32", "--headless", "--record", "3", "--record_steps", "12"])
    env, _ = play(args, steps=30, log_root=str(tmp_path), export_policy=False)
    assert env.trace_path == os.path.join(str(tmp_path), "exported", "traces", "play_go2_flat.npz")
    back = R.read_trace(env.trace_path)
    assert back["frames"].shape == (12, 3, GO2NN_TRACE_WIDTH) and back["steps_recorded"] == 30 and back["env_ids"].tolist() == [0, 1, 2]
    # the last recorded frame is the simulator's state as play() left it
    np.testing.assert_array_equal(back["root_pos"][-1], env.root_states[:3, :3].cpu().numpy())
    np.testing.assert_array_equal(back["dof_pos"][-1], env.dof_pos[:3].cpu().numpy())
    out = capsys.readouterr().out
    assert env.trace_path in out and sum(l.startswith("env ") for l in out.splitlines()) == 3
    env.close()


def test_gait_of_the_pretrained_student(hip):
    """the committed pretrained CTS student on the plane under forward_1.0: all four feet touch down repeatedly and are neither always nor never in contact (a sanity
    condition on the trace and its summary, not a gait number)"""
    from test_export import pretrained_policy
    from test_gpu_eval import _evaluator
    m, _ = pretrained_policy()
    ev = _evaluator("go2_flat_cts", record=2)
    res = ev.evaluate(m.to(DEV))
    tr = res["trace"]
    g = R.gait_summary(tr)
    k = [i for i, gr in enumerate(tr["group_of_robot"]) if tr["scenarios"][gr % len(tr["scenarios"])] == "forward_1.0"]
    assert len(k) == 2 and tr["frames"].shape[0] == ev.steps == 500
    print("\n".join(R.format_gait(tr, g)[i] for i in k))
    print({key: g[key][k].round(3).tolist() for key in R.GAIT_KEYS})
    assert not tr["reset"][:, k].any()
    assert (g["touchdowns"][k] > 0).all() and (g["duty_factor"][k] > 0).all() and (g["duty_factor"][k] < 1).all()
    q = R.mujoco_qpos(tr)
    assert np.abs(np.linalg.norm(q[..., 3:7], axis=-1) - 1).max() < 1e-4
    ev.close()
