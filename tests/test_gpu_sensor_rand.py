"""Training under randomised sensors on a real MI355X: the device build of go2nn_sensor_rand_apply over the scripted run of tests/test_sensor_rand_host.py (same
restatement, same bounds), LeggedRobot with domain_rand.randomize_sensors on the HIP libraries, and PPO / CTS rollouts replayed from the captured graph, restated from the
rollout storage alone — the cursor, the ring, the held frames and the episode starts live on the device and carry across replays and across the rollout boundary.
Run with -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_sensor_rand_host as rh  # noqa: E402
from test_gpu_sensor import DeviceMemory  # noqa: E402
from test_sensor_host import GO2_KIND, TOY_KIND, bits  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.fixture(scope="module")
def nn(hip):
    from go2_rl_gym_amd._nn import load_nn
    return load_nn()


@pytest.mark.parametrize("N", [17, 300])
@pytest.mark.parametrize("layout", ["go2", "toy"])
def test_scripted_run_on_the_device(nn, N, layout):
    """17 x 45 = 765 lanes leave a ragged last workgroup, 300 x 45 fill 53 of them; 17 x 7 lanes do not fill one"""
    kind = GO2_KIND if layout == "go2" else TOY_KIND
    case = rh.Case(N, kind=kind, env_offset=0 if N == 17 else 0xFFFFFF00, gravity_bias=0.02 if layout == "toy" else 0.0)
    rh.check_script(case, rh.run_script(nn, DeviceMemory(), case), "device N=%d D=%d" % (N, len(kind)))


@pytest.mark.parametrize("rows", [False, True])
def test_env_steps_on_the_hip_libraries(hip, nn, rows):
    """40 steps at 64 envs, plain and through rollout rows: obs_buf keeps the simulator's frame, the policy is handed the restated one"""
    env, _ = rh.make_env(hip, None, rh.sensor_cfg(), device=DEV)
    assert env._sensors["nn"] is nn and env._sensors["state"].is_cuda          # (loaded lazily: the HIP library)
    x, fresh, got = rh.drive(env, rows=rows)
    rh.check_env_run(env, x, fresh, got, "device env, 40 steps%s" % (" through rollout rows" if rows else ""))
    env.close()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_replayed_rollouts_against_the_restatement(hip, nn, monkeypatch, task):
    """two eager rollouts, the capture and one more replay: the last rollout's storage rows were written by the captured sensor launches"""
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    env, runner = rh.make_runner(hip, None, task, on=True, device=DEV)
    runner.learn(4, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert runner._rollout_graph is not None and runner._fuse_step, "the last rollout was not a graph replay"
    cursor = int(env._sensors["state"][:4].cpu().numpy().view(np.int32)[0])
    assert cursor == 1 + 4 * runner.num_steps_per_env          # reset() + every step, eager, captured or replayed
    rh.check_storage(env, runner, "%s, replayed rollout on the device" % task)
    model = runner.alg.actor_critic if hasattr(runner.alg, "actor_critic") else runner.alg.model
    assert all(torch.isfinite(p).all() for p in model.parameters())
    if task.endswith("cts"):
        assert bits(runner.history[:, -1].cpu().numpy()).tobytes() == bits(env.get_observations().cpu().numpy()).tobytes()
    env.close()


class Spy:
    """a go2nn handle that records which entry points were looked up"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def test_flag_off_never_calls_the_sensor_kernels(hip, nn, monkeypatch):
    from go2_rl_gym_amd import _nn
    spy = Spy(nn)
    monkeypatch.setattr(_nn, "_cached", spy)          # what load_nn() hands out, to the env and to everyone else
    env, runner = rh.make_runner(hip, None, "go2_flat", on=False, device=DEV)
    runner.learn(3, init_at_random_ep_len=True)
    env.reset_idx(torch.tensor([1, 2], device=DEV))
    obs = env.step(torch.zeros(env.num_envs, 12, device=DEV))[0]
    torch.cuda.synchronize()
    assert obs is env.obs_buf and env._sensors is None and not any("sensor" in k for k in vars(env))
    assert not [c for c in spy.calls if c.startswith("go2nn_sensor")], spy.calls
    st = runner.alg.storage
    assert bits(st.privileged_observations[:, :, 3:48].cpu().numpy()).tobytes() == bits(st.observations.cpu().numpy()).tobytes()
    env.close()
    spy.calls.clear()          # (and the spy does see them when the flag is on)
    env, _ = rh.make_env(hip, None, rh.sensor_cfg(), device=DEV)
    env.reset()
    assert {"go2nn_sensor_rand_check", "go2nn_sensor_rand_state_bytes", "go2nn_sensor_rand_begin", "go2nn_sensor_rand_apply"} <= set(spy.calls)
    env.close()
