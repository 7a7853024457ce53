"""The evaluator's action and torque spectra on a real MI355X: the device build of the go2nn_spectrum_* kernels against the float64 restatement of
tests/test_spectrum_host.py (same traces, same derived bound) at the wave and workgroup edges, against the host build bit for bit (every multiply-add of the Welch pass is
an explicit fma and the scales are computed on the host, so hipcc and g++ round at the same places), twice on the same trace, the argument checks, graph replay against
eager execution, and one small full evaluation.  Run with -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip, load_nn_emu  # noqa: E402
import test_spectrum_host as sh  # noqa: E402
from test_robust_host import HostMemory  # noqa: E402
from test_gpu_robust import DeviceMemory  # noqa: E402
from go2_rl_gym_amd._nn import spectrum_rows, spectrum_trace_rows, spectrum_twiddle  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402

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


def device_reduce(nn, table, group, G, W):
    t_d, g_d = torch.from_numpy(np.ascontiguousarray(table)).to(DEV), torch.from_numpy(group).to(DEV)
    out = torch.full((G, 1 + spectrum_rows(W)), -1.0, dtype=torch.float64, device=DEV)
    assert nn.go2nn_spectrum_reduce(C.c_void_p(t_d.data_ptr()), C.c_void_p(g_d.data_ptr()), table.shape[1], G, W, C.c_void_p(out.data_ptr()), DeviceMemory().stream) == 0, nn.go2nn_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("W", [8, 64])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_record_welch_and_reduce_on_the_device(nn, N, W):
    """one workgroup, one short of a wave of robots, a whole wave, one more, one more than a 256-lane workgroup of the record launch; field-major buffers as the HIP
    simulator keeps them; T = 2 W + 3: three windows and a dropped tail"""
    emu = load_nn_emu()
    T = 2 * W + 3
    actions, torques, reset = sh.random_trace(N, T)
    mem = DeviceMemory()
    trace_h = sh.record(nn, mem, actions, torques, reset, T, layout=1)
    trace = mem.get(trace_h).reshape(-1, N)
    sh.check_trace(trace, actions, torques, reset, T)
    tables = [sh.welch(nn, mem, trace_h, N, T, W, fill=f) for f in (7.0, -3.0)]          # twice on the same trace, over different stale contents
    assert tables[0].tobytes() == tables[1].tobytes()
    ref = sh.reference(actions[sh.WARMUP:], torques[sh.WARMUP:], reset[sh.WARMUP:], W)
    sh.check_table(tables[0], ref, W, "device N=%d W=%d" % (N, W))
    host_table, host_trace = sh.run_trace(emu, HostMemory(), actions, torques, reset, W)
    assert host_trace.tobytes() == trace.tobytes()
    assert host_table.tobytes() == tables[0].tobytes()          # device against host build, bit for bit
    G = 5
    for tab, group in (sh.reduce_case(N, G, W), (tables[0], (np.arange(N) % 4).astype(np.int32))):
        outs = [device_reduce(nn, tab, group, G, W) for _ in range(2)]
        assert outs[0].tobytes() == outs[1].tobytes()
        assert outs[0].tobytes() == sh.emu_reduce(emu, np.ascontiguousarray(tab), group, G, W).tobytes()
    if N >= 63:
        tab, group = sh.reduce_case(N, G, W)
        sh.check_reduce(device_reduce(nn, tab, group, G, W), tab, group, G, N, "device N=%d" % N)


def test_largest_window_on_the_device(nn):
    """W = 256: every lane owns four outputs and the workgroup's LDS is at its largest (53.4 KB); T = W + W / 2: two windows"""
    emu = load_nn_emu()
    N, W = 3, 256
    T = W + W // 2
    actions, torques, reset = sh.random_trace(N, T, resets=False)
    table, _ = sh.run_trace(nn, DeviceMemory(), actions, torques, reset, W)
    ref = sh.reference(actions[sh.WARMUP:], torques[sh.WARMUP:], reset[sh.WARMUP:], W)
    assert (ref["used"] == 2).all()
    sh.check_table(table, ref, W, "device W=256")
    assert table.tobytes() == sh.run_trace(emu, HostMemory(), actions, torques, reset, W)[0].tobytes()


def test_bad_arguments_write_nothing_on_the_device(nn):
    N, T, W = 4, 20, 8
    mem = DeviceMemory()
    trace, table = mem.put(np.full((spectrum_trace_rows(T), N), 3.0, np.float32)), mem.put(np.full((spectrum_rows(W), N), 3.0, np.float32))
    tw, out, group = mem.put(spectrum_twiddle(W)), mem.put(np.full((2, 1 + spectrum_rows(W)), 3.0)), mem.put(np.zeros(N, np.int32))
    bufs = {k: mem.put(np.zeros((12, N), np.float32)) for k in ("actions", "torques")}
    bufs["reset_buf"] = mem.put(np.zeros(N, np.uint8))
    p = lambda h: None if h is None else C.c_void_p(mem.ptr(h))
    make_in = lambda: sh.spectrum_in(mem, bufs, {"actions": (1, N), "torques": (1, N)})
    st = mem.stream
    assert nn.go2nn_spectrum_begin(None, N, 0, T, st) == sh.EINVAL and nn.go2nn_spectrum_begin(p(trace), 0, 0, T, st) == sh.EINVAL and nn.go2nn_spectrum_begin(p(trace), N, 0, 0, st) == sh.EINVAL
    a = make_in()
    a.joint_of_slot[0] = 1
    assert nn.go2nn_spectrum_record(C.byref(a), p(trace), N, T, st) == sh.EINVAL and b"joint_of_slot" in nn.go2nn_last_error()
    a = make_in()
    a.torques.p = None
    assert nn.go2nn_spectrum_record(C.byref(a), p(trace), N, T, st) == sh.EINVAL and nn.go2nn_spectrum_record(C.byref(make_in()), p(trace), N, 0, st) == sh.EINVAL
    for args in ((None, N, T, W, sh.FS, p(tw), p(table)), (p(trace), N, T, W, sh.FS, None, p(table)), (p(trace), N, T, W, sh.FS, p(tw), None), (p(trace), 0, T, W, sh.FS, p(tw), p(table)),
                 (p(trace), N, 0, W, sh.FS, p(tw), p(table)), (p(trace), N, T, 7, sh.FS, p(tw), p(table)), (p(trace), N, T, 258, sh.FS, p(tw), p(table)),
                 (p(trace), N, T, W, 0.0, p(tw), p(table))):
        assert nn.go2nn_spectrum_welch(*args, st) == sh.EINVAL and nn.go2nn_last_error(), args[1:5]
    for args in ((None, p(group), N, 2, W, p(out)), (p(table), p(group), N, 0, W, p(out)), (p(table), p(group), N, 2, 9, p(out)), (p(table), p(group), N, 2, W, None)):
        assert nn.go2nn_spectrum_reduce(*args, st) == sh.EINVAL
    torch.cuda.synchronize()
    assert (mem.get(trace) == 3.0).all() and (mem.get(table) == 3.0).all() and (mem.get(out) == 3.0).all()


def test_replay_equals_eager_with_spectrum(hip, monkeypatch):
    """the record launch sits inside the captured chunk (its step counter lives in the trace, so the same captured launch skips the warm-up in one replay and writes the
    right frame in every later one); the Welch launch runs once, outside the capture"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    m, _ = pretrained_policy()
    m = m.to(DEV)
    env_cfg, _ = task_registry.get_cfgs("go2_cts")
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, replay=True, spectrum=True, spectrum_window=32)
    ev = PolicyEvaluator(env_cfg, cfg, task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    eager = ev.evaluate(m, use_graph=False)
    t_eager, s_eager = ev.strace.cpu().numpy(), ev.stable.cpu().numpy()
    sh.check_spectrum_result(ev, eager, "eager")
    replay = ev.evaluate(m)
    t_replay, s_replay = ev.strace.cpu().numpy(), ev.stable.cpu().numpy()
    again = ev.evaluate(m, use_graph=False)
    assert (eager["mode"], replay["mode"], again["mode"]) == ("eager", "graph", "eager") and ev.chunk == 25 and ev.steps == 100 and ev.warmup_steps == 25
    assert t_eager.tobytes() == t_replay.tobytes() == ev.strace.cpu().numpy().tobytes() and s_eager.tobytes() == s_replay.tobytes() == ev.stable.cpu().numpy().tobytes()
    for other in (replay, again):
        assert eager["spectrum_table"].tobytes() == other["spectrum_table"].tobytes() and eager["table"].tobytes() == other["table"].tobytes()
        assert str(eager["spectrum"]) == str(other["spectrum"])
    # the device's table is the restatement's on the device's own trace
    frames = t_eager[1:].reshape(ev.steps, 25, ev.num_envs)
    unslot = np.argsort(sh.SLOTS)
    ref = sh.reference(frames[:, 0:12].transpose(0, 2, 1)[:, :, unslot], frames[:, 12:24].transpose(0, 2, 1)[:, :, unslot], frames[:, 24] != 0, 32, fs=ev.spectrum_fs)
    assert len(ref["windows"]) == 5 and ref["used"].sum() > 0
    sh.check_table(s_eager, ref, 32, "evaluation")
    ev.close()


def test_spectrum_of_a_small_full_evaluation(hip):
    """the committed pretrained CTS student on go2_cts, every terrain kind x six commands, 256 robots, 4 s, the default window: every figure finite, the centroids inside
    (0, fs / 2], the shares inside [0, 1]; the table is printed — these figures are what the run is there to show"""
    from test_export import pretrained_policy
    from go2_rl_gym_amd.utils.evaluator import SPECTRUM_KEYS, PolicyEvaluator, format_table
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    m, _ = pretrained_policy()
    env_cfg, train_cfg = task_registry.get_cfgs("go2_cts")
    ev = PolicyEvaluator(env_cfg, dict(class_to_dict(train_cfg.evaluation), num_envs=256, seconds=4.0, spectrum=True), task_class=task_registry.get_task_class("go2_cts"), device=DEV)
    res = ev.evaluate(m.to(DEV))
    print(format_table(res))
    print("overall per kind: %s" % {k: round(v, 4) for k, v in res["spectrum"]["overall"].items() if "/" in k})
    sh.check_spectrum_result(ev, res, "small full evaluation")
    d = res["spectrum"]["overall"]
    assert ev.spectrum_window == 64 and ev.steps == 200 and d["n_envs"] == 256 and d["spectrum_windows"] > 0
    for k, v in d.items():
        assert math.isfinite(v), (k, v)
    for sig in ("action", "torque"):
        assert 0.0 < d[sig + "_centroid_hz"] <= 0.5 * ev.spectrum_fs and 0.0 <= d[sig + "_hf_share"] <= 1.0 and d[sig + "_power"] > 0.0 and d[sig + "_smoothness"] > 0.0
    assert set(SPECTRUM_KEYS) < set(res["overall"])
    ev.close()
