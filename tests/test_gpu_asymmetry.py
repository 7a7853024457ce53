"""The evaluator's left-right asymmetry scores on a real MI355X: the device build of the go2nn_asym_* kernels against the float64 restatement of
tests/test_asymmetry_host.py (same script, same bounds) at the wave and workgroup edges in both buffer layouts, the reduce against the host build bit for bit, the two
policies with a known answer and the CTS student through PolicyEvaluator on the HIP libraries, the add-on discipline, and graph replay against eager execution.
Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip, load_nn_emu  # noqa: E402
import test_asymmetry_host as ah  # noqa: E402
from test_gpu_robust import DeviceMemory  # noqa: E402
from go2_rl_gym_amd._nn import GO2NN_ASYM_OUT_NUM  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils import symmetry as sym  # noqa: E402

DEV = "cuda:0"
BASE = dict(enabled=True, interval=1, terrain_level=3, seed=77, scenarios=ah.th.EVAL["scenarios"])


@pytest.fixture(scope="module")
def hip():
    lib = load_hip()
    assert lib.go2sim_is_device_library() == 1 and lib.go2sim_buffer_layout() == 1
    return lib


@pytest.fixture(scope="module")
def nn(hip):
    from go2_rl_gym_amd._nn import load_nn
    return load_nn()


def make_evaluator(_nn_lib, task="go2_flat", cb=None, **over):
    """tests/test_eval_host.py make_evaluator's signature, on the HIP libraries"""
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env_cfg, _ = task_registry.get_cfgs(task)
    return PolicyEvaluator(env_cfg, dict(BASE, **over), task_class=task_registry.get_task_class(task), device=DEV, step_callback=cb)


def device_reduce(nn, table, group, G):
    N = table.shape[1]
    t_d, g_d = torch.from_numpy(np.ascontiguousarray(table)).to(DEV), torch.from_numpy(group).to(DEV)
    out = torch.full((G, GO2NN_ASYM_OUT_NUM), -1.0, dtype=torch.float64, device=DEV)
    assert nn.go2nn_asym_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), N, G, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0, nn.go2nn_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_accumulate_and_reduce_on_the_device(nn, N, layout):
    """one lane, one short of a wave, a whole wave, one more, one more than a 256-lane workgroup; field-major buffers as the HIP simulator keeps them, and row-major ones"""
    emu = load_nn_emu()
    table, ref, _ = ah.run_script(nn, DeviceMemory(), N, layout)
    ah.check_table(table, ref, N, "device N=%d layout=%d" % (N, layout))
    G = 5
    for tab, group in (ah.reduce_case(N, G), (table, (np.arange(N) % 4).astype(np.int32))):          # a random table; the script's own, grouped by env index mod 4
        outs = [device_reduce(nn, tab, group, G) for _ in range(2)]
        assert outs[0].tobytes() == outs[1].tobytes()
        assert outs[0].tobytes() == ah.emu_reduce(emu, np.ascontiguousarray(tab), group, G).tobytes()
    tab, group = ah.reduce_case(N, G)
    ah.check_reduce(device_reduce(nn, tab, group, G), tab, group, G, N, "device N=%d" % N)


def test_constant_policy_has_its_closed_form(nn):
    ah.constant_policy_case(nn, make_evaluator, DEV)


def test_equivariant_policy_reads_zero_and_a_random_one_does_not(nn):
    """the forward kernels are what they were before this feature: their own gap to float64, measured in the same run, is the yardstick"""
    ah.equivariant_policy_case(nn, make_evaluator, DEV)


def test_flag_on_moves_nothing_else_and_repeats(nn):
    ac = ah.th.small_actor_critic().to(DEV)
    over = dict(ah.ASYM, gait=True, record=1)
    runs = {}
    for name, extra in (("off", {}), ("on", dict(asymmetry=True))):
        ev = make_evaluator(nn, **dict(over, **extra))
        runs[name] = (ev, ev.evaluate(ac))
    (ev, res), (ev0, res0) = runs["on"], runs["off"]
    assert "asymmetry" not in res0 and not hasattr(ev0, "atable") and res["asymmetry"]["overall"]["n_envs"] == 64
    assert res["table"].tobytes() == res0["table"].tobytes() and res["gait_table"].tobytes() == res0["gait_table"].tobytes()
    assert str(res["overall"]) == str(res0["overall"]) and str(res["groups"]) == str(res0["groups"]) and str(res["gait"]) == str(res0["gait"])
    assert res["trace"]["frames"].tobytes() == res0["trace"]["frames"].tobytes()
    again = ev.evaluate(ac)
    assert again["asymmetry_table"].tobytes() == res["asymmetry_table"].tobytes() and str(again["asymmetry"]) == str(res["asymmetry"])
    ev.close()
    ev0.close()


def test_cts_student_on_the_device(nn):
    """go2_flat_cts, the packed kernels' path: the history fed to the encoder's second run is mirror_rows(history, history_table) bit for bit, the figures are those of the
    kept frames; a recurrent model is refused"""
    from test_sensor_host import small_models
    models = small_models()
    cts = models["cts"].to(DEV)
    frames = []
    ev = make_evaluator(nn, task="go2_flat_cts", cb=ah.keeper(frames), asymmetry=True, **ah.ASYM)
    res = ev.evaluate(cts)
    assert ev._policy.kernels and len(frames) == ev.warmup_steps + ev.steps
    H = cts.history_length
    htab = sym.history_table(ah.OBS_TABLE, H)
    ah.check_frames(frames)
    for k, f in enumerate(frames):
        assert f["hist"].shape == (64, H * 45) and f["hist_m"].tobytes() == sym.mirror_rows(f["hist"], htab).astype(np.float32).tobytes(), k
    ah.check_result(ev, res, ah.reference_of(ev, frames), "cts on the device")
    import copy
    m64 = copy.deepcopy(cts).cpu().double()
    fr = [f for f in frames if f["counted"]]
    with torch.no_grad():
        fwd = lambda h, o: m64.policy_mean(m64.student_latent(torch.from_numpy(h.astype(np.float64)))[0], torch.from_numpy(o.astype(np.float64))).numpy()
        a64, am64 = np.stack([fwd(f["hist"], f["obs"]) for f in fr]), np.stack([fwd(f["hist_m"], f["obs_m"]) for f in fr])
    delta = max(np.abs(a64 - np.stack([f["a"] for f in fr])).max(), np.abs(am64 - np.stack([f["a_m"] for f in fr])).max())
    assert 0 < delta < 1e-4
    ah.check_against_float64(ev, res, a64, am64, delta, "cts on the device")
    ev.close()
    rec = make_evaluator(nn, asymmetry=True, **ah.ASYM)
    with pytest.raises(NotImplementedError, match="twin hidden state"):
        rec.evaluate(models["lstm"].to(DEV))
    rec.close()


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_replay_equals_eager_with_asymmetry(nn, task, monkeypatch):
    """evaluation.replay: the first evaluation runs eagerly, the second is a captured chunk replayed — the mirror launch, the second forward and the accumulate launch
    inside it; the step counter lives in the table, so the same captured launch skips the warm-up in one replay and counts in the later ones"""
    from test_sensor_host import small_models
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    ac = (ah.th.small_actor_critic() if task == "go2_flat" else small_models()["cts"]).to(DEV)
    ev = make_evaluator(nn, task=task, asymmetry=True, replay=True, gait=True, **ah.ASYM)
    eager = ev.evaluate(ac)
    t_eager = ev.atable.cpu().numpy()
    replay = ev.evaluate(ac)
    assert (eager["mode"], replay["mode"]) == ("eager", "graph") and ev.chunk == 5 and (ev.atable.cpu().numpy()[0] == ev.steps).all()
    assert t_eager.tobytes() == ev.atable.cpu().numpy().tobytes() and eager["asymmetry_table"].tobytes() == replay["asymmetry_table"].tobytes()
    assert str(eager["asymmetry"]) == str(replay["asymmetry"]) and eager["table"].tobytes() == replay["table"].tobytes()
    assert eager["gait_table"].tobytes() == replay["gait_table"].tobytes() and eager["asymmetry"]["overall"]["equivariance_rmse"] > 0
    ev.close()
