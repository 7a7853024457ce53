"""The evaluator's sensor model on a real MI355X: the device build of go2nn_sensor_apply over the scripted run of tests/test_sensor_host.py (same restatement, same
checks, same bound), graph replay against eager execution with delays and held frames crossing the chunk boundaries, the nominal condition against the plain evaluation,
and what the pretrained CTS student was actually shown.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_sensor_host as sh  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils import get_args  # noqa: E402

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


class DeviceMemory:
    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)

    def ptr(self, h):
        return h.data_ptr()

    def get(self, h):
        return h.cpu().numpy()

    def set(self, h, a):
        h.view(-1).copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))


@pytest.mark.parametrize("N", [17, 300])
def test_scripted_run_on_the_device(nn, N):
    """17 x 45 lanes leave a ragged last workgroup, 300 x 45 fill 53 of them; identity, delays, drops byte for byte, noise and bias to 4 ulp of the largest term"""
    case = sh.Case(N)
    out = sh.run_script(nn, DeviceMemory(), case)
    sh.check_run(case, out, "device N=%d D=45" % N)


@pytest.fixture(scope="module")
def flat(hip):
    args = get_args(["--task", "go2_flat", "--num_envs", "64", "--headless"])
    env, _ = task_registry.make_env("go2_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    yield env, runner.alg.actor_critic
    env.close()


CFG = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None)


def test_replay_equals_eager_with_sensors(flat, monkeypatch):
    """a captured chunk is 25 steps and is replayed 5 times; the cursor, the ring and the held frames live on the device, so the delay_2 robots of a chunk's first two steps
    read what the previous replay stored, and a frame dropped at a chunk's first step repeats the previous replay's last one — as in the eager run"""
    from go2_rl_gym_amd.utils.evaluator import DEFAULT_SENSORS, PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    env, ac = flat
    ev = PolicyEvaluator(env.cfg, dict(CFG, replay=True, sensors=DEFAULT_SENSORS), task_class=type(env), sim_params=env.sim_params, device=env.sim_device)
    eager = ev.evaluate(ac, use_graph=False)
    replay = ev.evaluate(ac)
    again = ev.evaluate(ac, use_graph=False)
    assert (eager["mode"], replay["mode"], again["mode"]) == ("eager", "graph", "eager") and ev.chunk == 25
    print("overall %s" % eager["overall"])
    assert np.isfinite(eager["cell_table"]).all() and eager["cell_table"][:, 0].sum() == 256 * ev.steps
    assert eager["cell_table"][0::8].tobytes() != eager["cell_table"][2::8].tobytes()          # (nominal and noise_3.0 robots do not score alike)
    for other in (again, replay):
        assert eager["table"].tobytes() == other["table"].tobytes() and eager["cell_table"].tobytes() == other["cell_table"].tobytes()
        assert str(eager["cells"]) == str(other["cells"]) and str(eager["sensors"]) == str(other["sensors"])
    ev.close()


def test_nominal_alone_equals_the_plain_evaluation_on_the_device(flat):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env, ac = flat
    tables = []
    for sensors in (None, [["nominal", {}]]):
        ev = PolicyEvaluator(env.cfg, dict(CFG, sensors=sensors), task_class=type(env), sim_params=env.sim_params, device=env.sim_device)
        res = ev.evaluate(ac)
        assert (sensors is None) == (not hasattr(ev, "sstate")) and ("sensors" in res) == (sensors is not None)
        tables.append((res["table"].tobytes(), str(res["groups"])))
        ev.close()
    assert tables[0] == tables[1]


def test_what_the_pretrained_student_saw(hip):
    """the committed pretrained CTS student on the plane under the default conditions (1024 robots, 1 s + 10 s, eager): at three consecutive counted steps the delay_1
    robots were shown the proprioceptive columns the simulator wrote one step earlier — the current ones where the robot was reset in that step — and the current commands
    and previous actions; the nominal robots the current observation.  No inequality between the conditions' scores is asserted: none holds by construction"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import DEFAULT_SENSORS, PolicyEvaluator, format_table
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    m, _ = pretrained_policy()
    m = m.to(DEV)
    env_cfg, train_cfg = task_registry.get_cfgs("go2_flat_cts")
    cfg = dict(class_to_dict(train_cfg.evaluation), sensors=DEFAULT_SENSORS)
    first, seen = 200, {}

    def cb(ev, k, counted):
        s = k - ev.warmup_steps
        if first - 1 <= s < first + 3:
            seen[s] = (ev.delivered.cpu().numpy(), ev.env.obs_buf.cpu().numpy(), ev.env._buf["reset_buf"].cpu().numpy() != 0)
    ev = PolicyEvaluator(env_cfg, cfg, task_class=task_registry.get_task_class("go2_flat_cts"), device=DEV, step_callback=cb)
    res = ev.evaluate(m)
    print(format_table(res))
    names = [c[0] for c in DEFAULT_SENSORS]
    nominal, late = ev.sensor_host == names.index("nominal"), ev.sensor_host == names.index("delay_1")
    prop = sh.GO2_KIND != sh.K["pass"]
    assert sorted(seen) == [first - 1, first, first + 1, first + 2]
    for s in range(first, first + 3):
        (dl, ob, reset), (_, ob_prev, _) = seen[s], seen[s - 1]
        assert (sh.bits(dl[nominal]) == sh.bits(ob[nominal])).all()
        want = np.where(reset[late][:, None], ob[late], ob_prev[late])
        assert (sh.bits(dl[late][:, prop]) == sh.bits(want[:, prop])).all() and (sh.bits(dl[late][:, ~prop]) == sh.bits(ob[late][:, ~prop])).all()
        assert reset[late].mean() < 0.5 and (sh.bits(dl[late][:, prop]) != sh.bits(ob[late][:, prop])).any()
    S, Pn = len(res["scenarios"]), len(names)
    sizes = np.bincount(ev.cell_host, minlength=ev.num_cells)
    assert ev.num_cells == S * Pn and sizes.sum() == 1024 and sizes.min() >= 4 and sizes.max() - sizes.min() <= 1
    for si, s in enumerate(res["scenarios"]):
        for pi, n in enumerate(names):
            assert res["cells"]["plane"][s][n]["n_envs"] == sizes[si * Pn + pi]
    assert res["cell_table"][:, 0].sum() == 1024 * ev.steps and sum(d["n_envs"] for d in res["sensors"].values()) == 1024 == res["overall"]["n_envs"]
    assert all(np.isfinite(d["lin_vel_err"]) for d in res["sensors"].values())
    ev.close()
