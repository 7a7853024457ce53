"""The black box on the CPU: the host build of go2nn_blackbox_* (include/go2nn.h) against a numpy model written here over a scripted sequence of resets that meets every
edge of the rule — every frame is a copy, so every comparison is exact —, a frozen robot under poisoned buffers, the argument checks, the symbols and the state block's enum,
and PolicyEvaluator with `blackbox` on the oracle + the host build: nothing changes with it off, nothing else moves with it on, real falls are the existing recorder's frames
byte for byte, it runs next to every mode, and what the host side makes of a falls dict (fall_summary, the .npz)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, load_nn_emu
import test_eval_host as th
import test_gait_host as tg
import test_trace_host as tt
from test_robust_host import HostMemory
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import BLACKBOX_ROWS, GO2NN_BLACKBOX_NUM, GO2NN_TRACE_WIDTH, TRACE_FIELDS, TRACE_OFFSET
from go2_rl_gym_amd.utils import recorder as R

EINVAL = -22
WARM = 3          # uncounted calls before counted step 0
W = GO2NN_TRACE_WIDTH
CASES = ("warmup_fall_restarts", "timeout_restarts", "fall_at_step_0", "fall_at_written_T", "fall_at_written_T_plus_1", "second_fall_ignored", "never_falls", "short_ring")
PATTERNS = 8


def steps_of(T):
    return 3 * T + 2          # counted steps: at least 3 T


def script(N, T, offset=0, seed=0):
    """-> (reset, time_out) bool [WARM + steps, N].  Robot e follows pattern (e + offset) % 8; from the 17th robot on a random script.  F fall, O time-out, at call index:
      0  F in the warm-up (call 1), nothing else             4  O at counted step 0, F at counted step T + 1: WRITTEN = T + 1, one past the wrap
      1  O at counted step 2, never falls                    5  F at counted steps 1 and 3: the second changes nothing
      2  F at counted step 0                                 6  no reset at all
      3  O at counted step 0, F at counted step T: the ring has just been filled, WRITTEN = T exactly
      7  O at counted step 1, F at counted step T: T - 1 frames, a ring that is not full"""
    calls = WARM + steps_of(T)
    rng = np.random.default_rng(seed + 1000 * N + T)
    reset, tout = np.zeros((calls, N), bool), np.zeros((calls, N), bool)
    for e in range(N):
        F, O = [], []
        if e >= 2 * PATTERNS:
            kind = rng.choice(3, calls, p=[0.86, 0.08, 0.06])
            F, O = np.nonzero(kind == 1)[0].tolist(), np.nonzero(kind == 2)[0].tolist()
        else:
            p = (e + offset) % PATTERNS
            F, O = {0: ([1], []), 1: ([], [WARM + 2]), 2: ([WARM], []), 3: ([WARM + T], [WARM]), 4: ([WARM + T + 1], [WARM]), 5: ([WARM + 1, WARM + 3], []), 6: ([], []),
                    7: ([WARM + T], [WARM + 1])}[p]
        reset[F, e] = True
        reset[O, e] = tout[O, e] = True
    return reset, tout


def distinct_buffers(N, call, reset, tout):
    """one call's source buffers in their LOGICAL shapes [N, ...]: every float is a whole number of its own — per (call, field, robot, component) —, exact in fp32"""
    per_call = sum(N * int(np.prod(s, dtype=np.int64)) for k, s in tt.SHAPES.items() if not k.endswith("_buf") or k == "rew_buf")
    assert (WARM + 64) * per_call < 2 ** 24
    d, at = {}, call * per_call
    for k, s in tt.SHAPES.items():
        if k in ("reset_buf", "time_out_buf"):
            continue
        n = N * int(np.prod(s, dtype=np.int64))
        d[k] = (at + np.arange(n)).reshape((N,) + s).astype(np.float32)
        at += n
    d["reset_buf"], d["time_out_buf"] = reset.astype(np.uint8), tout.astype(np.uint8)
    return d


class Model:
    """the rule of include/go2nn.h in numpy, robot by robot"""

    def __init__(self, N, T, first_step):
        self.N, self.T, self.step = N, T, first_step
        self.written, self.frozen, self.fall_step = np.zeros(N, np.int32), np.zeros(N, np.int32), np.full(N, -1, np.int32)
        self.frames = np.full((N, T, W), np.nan, np.float32)
        self.seen = set()

    def record(self, frame, reset, tout):
        s = self.step
        for e in range(self.N):
            fell = reset[e] and not tout[e]
            if self.frozen[e]:
                if fell:
                    self.seen.add("second_fall_ignored")
                continue
            self.frames[e, self.written[e] % self.T] = frame[e]
            self.written[e] += 1
            if fell and s >= 0:
                self.frozen[e], self.fall_step[e] = 1, s
                self.seen.add("fall_at_step_0" if s == 0 else "fall_later")
                for name, w in (("fall_at_written_T", self.T), ("fall_at_written_T_plus_1", self.T + 1)):
                    if self.written[e] == w:
                        self.seen.add(name)
                if self.written[e] < self.T:
                    self.seen.add("short_ring")
            elif reset[e]:
                self.written[e] = 0
                self.seen.add("warmup_fall_restarts" if fell else ("timeout_restarts" if s >= 0 else "warmup_timeout"))
        self.step += 1

    def state(self):
        return np.concatenate([self.written, self.frozen, self.fall_step, [self.step]]).astype(np.int32)


def run_script(lib, mem, N, T, layout, offset=0, check_every=True, poison=False):
    """the scripted sequence on `lib` with its buffers in `mem` (HostMemory here, DeviceMemory on the GPU), against the Model after every call or at the end
    -> (frames, state, model).  poison: once a robot is frozen its source rows hold garbage and its flags say `fall` on every later call"""
    reset, tout = script(N, T, offset)
    calls = reset.shape[0]
    model = Model(N, T, -WARM)
    d = distinct_buffers(N, 0, reset[0], tout[0])
    store, strides = tt.pack(d, layout)
    h = {k: mem.put(v) for k, v in store.items()}
    a = tt.trace_in(lambda k: mem.ptr(h[k]), strides)
    frames, state = mem.put(np.full((N, T, W), np.nan, np.float32)), mem.put(np.full(GO2NN_BLACKBOX_NUM * N + 1, 77, np.int32))
    assert lib.go2nn_blackbox_begin(C.c_void_p(mem.ptr(state)), N, -WARM, mem.stream) == 0, lib.go2nn_last_error()
    assert mem.get(state).tobytes() == model.state().tobytes()
    frozen_at = {}
    for call in range(calls):
        r, t = reset[call].copy(), tout[call].copy()
        d = distinct_buffers(N, call, r, t)
        if poison:
            for e in np.nonzero(model.frozen)[0]:
                for k in TRACE_FIELDS:
                    d[k][e] = 1 if k == "reset_buf" else (0 if k == "time_out_buf" else -7777.0)
            r, t = d["reset_buf"] != 0, d["time_out_buf"] != 0
        for k, v in tt.pack(d, layout)[0].items():
            mem.set(h[k], v)
        assert lib.go2nn_blackbox_record(C.byref(a), N, C.c_void_p(mem.ptr(frames)), C.c_void_p(mem.ptr(state)), T, mem.stream) == 0, lib.go2nn_last_error()
        model.record(tt.gather(d, np.arange(N)), r, t)
        if check_every or call == calls - 1:
            got_f, got_s = mem.get(frames).reshape(N, T, W), mem.get(state)
            assert got_s.tobytes() == model.state().tobytes(), (call, got_s, model.state())
            assert got_f.tobytes() == model.frames.tobytes(), call
            if poison:          # a robot's ring and state row as they were on the call that froze it
                for e in np.nonzero(model.frozen)[0]:
                    now = (got_f[e].tobytes(), got_s[:-1].reshape(GO2NN_BLACKBOX_NUM, N)[:, e].tobytes())
                    assert frozen_at.setdefault(int(e), now) == now, (e, call)
    return mem.get(frames).reshape(N, T, W), mem.get(state), model


def run_offsets(lib, make_mem, N, T, layout, **kw):
    """every pattern is met: with fewer robots than patterns, by as many runs as it takes -> the models"""
    models = [run_script(lib, make_mem(), N, T, layout, offset=o, **kw)[2] for o in (range(0, PATTERNS, N) if N < PATTERNS else [0])]
    seen = set().union(*[m.seen for m in models])
    if any((m.frozen == 0).any() for m in models):
        seen.add("never_falls")
    assert seen >= set(CASES), set(CASES) - seen          # the script really contains every case
    return models


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("T", [2, 4, 7])
@pytest.mark.parametrize("N", [1, 3, 70])
def test_kernel_against_the_numpy_model(emu, N, T, layout):
    models = run_offsets(emu, HostMemory, N, T, layout)
    assert all(m.step == steps_of(T) and steps_of(T) >= 3 * T for m in models)
    if N == 70:          # the hand-written figures of the eight patterns, first robot of each
        m = models[0]
        assert m.frozen[:8].tolist() == [0, 0, 1, 1, 1, 1, 0, 1] and m.fall_step[:8].tolist() == [-1, -1, 0, T, T + 1, 1, -1, T]
        assert m.written[:8].tolist() == [WARM + steps_of(T) - 2, steps_of(T) - 3, WARM + 1, T, T + 1, WARM + 2, WARM + steps_of(T), T - 1]
        assert m.frozen[16:].any() and not m.frozen[16:].all()


@pytest.mark.parametrize("layout", [0, 1])
def test_frozen_stays_frozen(emu, layout):
    """once a robot has fallen its source rows are garbage and its flags say `fall` on every call: ring and state row stay what they were, byte for byte"""
    frames, state, model = run_script(emu, HostMemory(), 20, 4, layout, poison=True)
    assert model.frozen.sum() >= 6 and "second_fall_ignored" in model.seen and not (frames == -7777.0).any()


def test_argument_checks(emu):
    N, T = 4, 3
    d = distinct_buffers(N, 0, np.zeros(N, bool), np.zeros(N, bool))
    store, strides = tt.pack(d, 0)
    frames, state = np.zeros((N, T, W), np.float32), np.zeros(GO2NN_BLACKBOX_NUM * N + 1, np.int32)
    p = lambda x: C.c_void_p(x.ctypes.data)          # noqa: E731
    good = lambda: tt.trace_in(lambda k: store[k].ctypes.data, strides)          # noqa: E731
    assert emu.go2nn_blackbox_begin(p(state), N, -2, None) == 0 and state.tolist() == [0] * 8 + [-1] * 4 + [-2]
    assert emu.go2nn_blackbox_record(C.byref(good()), N, p(frames), p(state), T, None) == 0, emu.go2nn_last_error()
    kept = frames.copy(), state.copy()
    assert state[-1] == -1 and state[:N].tolist() == [1] * N
    cases = [emu.go2nn_blackbox_record(None, N, p(frames), p(state), T, None), emu.go2nn_blackbox_record(C.byref(good()), N, None, p(state), T, None),
             emu.go2nn_blackbox_record(C.byref(good()), N, p(frames), None, T, None)]
    assert cases == [EINVAL] * 3 and b"null" in emu.go2nn_last_error()
    for n, t in ((0, T), (-1, T), (N, 0), (N, -3), (2 ** 31 // W + 1, T)):
        assert emu.go2nn_blackbox_record(C.byref(good()), n, p(frames), p(state), t, None) == EINVAL and emu.go2nn_last_error().startswith(b"blackbox record: N ="), (n, t)
    assert emu.go2nn_blackbox_record(C.byref(_nn.Go2nnTraceIn()), N, p(frames), p(state), T, None) == EINVAL
    for mutate in ("env", "comp", "body", "vel", "foot", "ptr"):
        a = good()
        if mutate == "env":
            a.torques.env_stride = 0
        elif mutate == "comp":
            a.root_states.comp_stride = 0
        elif mutate == "body":
            a.contact_body_stride = 0
        elif mutate == "vel":
            a.dof_vel_offset = 0
        elif mutate == "foot":
            a.foot_body[1] = -1
        else:
            a.time_out_buf.p = None
        assert emu.go2nn_blackbox_record(C.byref(a), N, p(frames), p(state), T, None) == EINVAL and emu.go2nn_last_error().startswith(b"blackbox record: bad source"), mutate
    assert frames.tobytes() == kept[0].tobytes() and state.tobytes() == kept[1].tobytes()          # a refused call writes nothing
    assert emu.go2nn_blackbox_begin(None, N, 0, None) == EINVAL and emu.go2nn_blackbox_begin(p(state), 0, 0, None) == EINVAL and emu.go2nn_last_error().startswith(b"blackbox begin")
    assert state.tobytes() == kept[1].tobytes()


def test_symbols_and_state_enum_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7 and _nn.GO2NN_ABI_VERSION == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_blackbox_begin", "go2nn_blackbox_record"):
            assert (" T " + f + "\n") in syms, (path, f)
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "go2nn.h"\nint main(void) { printf("%d %lld", (int)GO2NN_BLACKBOX_NUM, (long long)GO2NN_BLACKBOX_STATE_INTS(1000));\n'
                   + "".join('printf(" %%d", (int)GO2NN_BLACKBOX_%s);\n' % r.upper() for r in BLACKBOX_ROWS) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [GO2NN_BLACKBOX_NUM, GO2NN_BLACKBOX_NUM * 1000 + 1] + list(range(len(BLACKBOX_ROWS))) and GO2NN_BLACKBOX_NUM == 3
    hdr = open(os.path.join(ROOT, "include", "go2nn.h")).read()
    enum = hdr[hdr.index("GO2NN_BLACKBOX_WRITTEN = 0"):hdr.index("GO2NN_BLACKBOX_NUM }")]
    assert [e.strip().split(" ")[0].replace("GO2NN_BLACKBOX_", "").lower() for e in enum.split(",") if e.strip()] == list(BLACKBOX_ROWS)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# The evaluator.  A zero-weight actor: the action is 0 and the robot holds its default pose — the nominal robots stand for the whole horizon, and the `limp` ones (motor
# strength 0.05) sink to base contact.  Verified on the CPU oracle with these values: 24 robots, 0.2 s + 2 s: all 12 limp robots fall, at counted steps 0 .. 16; no nominal one.
LIMP = [["nominal", {}], ["limp", {"strength": 0.05}]]
REAL = dict(warmup_s=0.2, seconds=2.0, perturbations=LIMP, push_first_s=0.5, push_period_s=1.0, push_window_s=0.4)


def zero_actor():
    ac = th.small_actor_critic()
    with torch.no_grad():
        for p in ac.actor.parameters():
            p.zero_()
    return ac


def reset_log():
    """-> (step callback, list): the reset flags of every env after every eager step, warm-up included — the one thing about the warm-up the trace does not show"""
    log = []
    return (lambda ev, k, counted: log.append(ev.env._buf["reset_buf"].detach().cpu().numpy().astype(bool).copy())), log


def check_falls_against_trace(ev, res, resets, what):
    """res of an evaluation with record = every robot and a black box that keeps every fall; resets [warm-up + counted steps, N] from reset_log: per fallen robot the black
    box's frames are the full trace's"""
    falls, tr, resets = res["falls"], res["trace"], np.stack(resets)
    assert resets.shape == (ev.warmup_steps + ev.steps, ev.num_envs) and (resets[ev.warmup_steps:] == tr["reset"]).all()
    T, S = ev.fall_recorder.T, ev.steps
    assert tr["env_ids"].tolist() == list(range(ev.num_envs)) and tr["frames"].shape[0] == S == tr["steps_recorded"]
    fell = tr["reset"] & ~tr["time_out"]          # [S, N]
    want_ids = np.nonzero(fell.any(0))[0]
    assert falls["fell_env_ids"].tolist() == want_ids.tolist() and falls["fell_total"] == len(want_ids) and falls["env_ids"].tolist() == want_ids.tolist()
    pert = ev.pert_host[want_ids]
    assert len(want_ids) >= 1 and (pert == 1).all(), (want_ids, pert)          # the precondition: limp robots fell, no nominal robot did
    assert falls["frames"].shape == (len(want_ids), T, W) and falls["steps"] == S
    from_warmup = 0
    for k, e in enumerate(want_ids):
        s, n = int(fell[:, e].argmax()), int(falls["length"][k])
        assert falls["fall_step"][k] == s and 1 <= n <= T
        assert np.isnan(falls["frames"][k, :T - n]).all() and not falls["reset"][k, :T - n].any()
        counted = min(n, s + 1)          # frames s - counted + 1 .. s lie in the counted steps; older ones are warm-up frames, which the trace does not have
        assert falls["frames"][k, T - counted:].tobytes() == tr["frames"][s - counted + 1:s + 1, e].tobytes(), (e, s, n)
        call = ev.warmup_steps + s          # the ring started again after the robot's last reset before the fall (in the warm-up: a fall there freezes nothing)
        before = np.nonzero(resets[:call, e])[0]
        assert n == min(T, call - (int(before[-1]) if len(before) else -1)), (e, s, n)          # so many of them are warm-up frames: n - counted
        assert np.isfinite(falls["frames"][k, T - n:]).all() and falls["reset"][k, -1] and not falls["time_out"][k, -1] and not falls["reset"][k, T - n:-1].any()
        from_warmup += n - counted
    wrapped = int((fell.argmax(0)[want_ids] + 1 + ev.warmup_steps > T).sum())
    print("%s: %d of %d robots fell (counted steps %s), T = %d, %d rings wrapped, %d frames from the warm-up" % (what, len(want_ids), ev.num_envs,
                                                                                                                sorted(set(falls["fall_step"].tolist())), T, wrapped, from_warmup))
    return wrapped, from_warmup


@pytest.fixture(scope="module")
def real_falls(emu):
    cb, log = reset_log()
    ev = th.make_evaluator(emu, cb=cb, num_envs=24, record=24, blackbox=24, blackbox_seconds=0.3, **REAL)
    res = ev.evaluate(zero_actor())
    yield ev, res, log
    ev.close()


def test_real_falls_against_the_existing_recorder(real_falls):
    ev, res, log = real_falls
    assert ev.fall_recorder.T == 15 and ev.warmup_steps == 10 and ev.steps == 100
    wrapped, from_warmup = check_falls_against_trace(ev, res, log, "oracle, limp 0.05")
    assert wrapped >= 1 and from_warmup >= 1          # both kinds of ring occur: one that has wrapped, one that still holds warm-up frames
    falls = res["falls"]
    assert falls["perturbations"] == ["nominal", "limp"] and (falls["pert_of_robot"] == 1).all() and falls["push_steps"].tolist() == ev.push_steps.tolist()
    assert falls["group_of_robot"].tolist() == ev.group_host[falls["env_ids"]].tolist() and falls["cell_of_robot"].tolist() == ev.cell_host[falls["env_ids"]].tolist()
    assert falls["fell_per_cell"].sum() == falls["fell_total"] and falls["fell_per_cell"][0::2].sum() == 0
    sm = R.fall_summary(falls)
    has = falls["length"] >= 2
    assert has.any() and (sm["time_s"] == falls["fall_step"] * ev.dt).all() and (sm["base_height"][has] < 0.25).all() and (sm["tilt"][has] >= 0).all()
    np.testing.assert_array_equal(sm["command"][has], ev.commands_host[falls["env_ids"]][has, :3])


def test_outputs_with_falls(real_falls, tmp_path):
    from go2_rl_gym_amd.utils.evaluator import format_table, scalars, write_results
    ev, res, _ = real_falls
    falls = res["falls"]
    assert dict(scalars(res))["Eval/falls/robots_fell"] == falls["fell_total"]
    text = format_table(res).splitlines()
    at = [i for i, l in enumerate(text) if l.startswith("falls (first counted fall per robot)")]
    cells = np.nonzero(falls["fell_per_cell"])[0]
    assert len(at) == 1 and len(text) == at[0] + 1 + len(cells) + 1 and all("/limp" in l for l in text[at[0] + 1:-1]) and text[-1].split() == ["all", str(falls["fell_total"]), str(len(falls["env_ids"]))]
    first = text[at[0] + 1].split()
    k = falls["cell_of_robot"] == cells[0]
    assert first[0] == falls["cell_names"][cells[0]] and first[1:3] == [str(falls["fell_per_cell"][cells[0]]), str(int(k.sum()))]
    assert float(first[3]) == pytest.approx(np.median(R.fall_summary(falls)["time_s"][k]), abs=1e-4)
    write_results(str(tmp_path), 7, res)
    assert sorted(os.listdir(tmp_path / "eval_results")) == ["falls_7.npz", "results_7.yaml", "trace_7.npz"]
    back = R.read_falls(str(tmp_path / "eval_results" / "falls_7.npz"))
    assert back["frames"].tobytes() == falls["frames"].tobytes() and back["cell_names"] == falls["cell_names"] and back["fell_total"] == falls["fell_total"]
    assert len(R.format_falls(back, back["summary"])) == len(falls["env_ids"])


PLAIN = dict(num_envs=32, seconds=0.6, warmup_s=0.1)


@pytest.fixture(scope="module")
def plain_runs(emu):
    """the same weights five times: an evaluator that never heard of the black box, blackbox = 0 given, record + gait without it, record + gait with it"""
    ac = th.small_actor_critic()
    out = {}
    for name, over in (("never", {}), ("off", dict(blackbox=0, blackbox_seconds=0.5)), ("base", dict(record=1, gait=True)), ("on", dict(record=1, gait=True, blackbox=2))):
        ev = th.make_evaluator(emu, **dict(PLAIN, **over))
        out[name] = (ev, ev.evaluate(ac))
    yield out
    for ev, _ in out.values():
        ev.close()


def same_tree(a, b):
    assert type(a) is type(b), (type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            same_tree(a[k], b[k])
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same_tree(x, y)
    else:
        assert a == b or (a != a and b != b), (a, b)


def test_off_changes_nothing(plain_runs, tmp_path):
    import yaml
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.evaluator import format_table, results_dict, scalars, write_results
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    (ev0, res0), (ev1, res1) = plain_runs["never"], plain_runs["off"]
    assert "blackbox" not in th.EVAL and ev1.blackbox == 0 and ev1.fall_recorder is None and ev0.fall_recorder is None
    same_tree(res0, res1)
    assert "falls" not in res1 and format_table(res1) == format_table(res0)
    same_tree(scalars(res1), scalars(res0))
    assert yaml.safe_dump(results_dict(res1, 3)) == yaml.safe_dump(results_dict(res0, 3))
    for name, res in (("a", res0), ("b", res1)):
        write_results(str(tmp_path / name), 3, res)
    assert os.listdir(tmp_path / "a" / "eval_results") == os.listdir(tmp_path / "b" / "eval_results") == ["results_3.yaml"]
    assert open(tmp_path / "a" / "eval_results" / "results_3.yaml").read() == open(tmp_path / "b" / "eval_results" / "results_3.yaml").read()
    for task in ("go2_flat", "go2_cts"):
        e = task_registry.get_cfgs(task)[1].evaluation
        assert (e.blackbox, e.blackbox_seconds, e.blackbox_max_bytes) == (0, 2.0, 512 * 1024 * 1024)
    assert get_args([]).blackbox is None and get_args(["--blackbox"]).blackbox == 2 and get_args(["--blackbox", "5", "--robust"]).blackbox == 5
    _, cfg = update_cfg_from_args(None, task_registry.get_cfgs("go2_flat")[1], get_args(["--blackbox", "--gait"]))
    assert cfg.evaluation.blackbox == 2 and cfg.evaluation.gait is True and task_registry.get_cfgs("go2_flat")[1].evaluation.blackbox == 0


def test_on_leaves_everything_else_alone(plain_runs):
    from go2_rl_gym_amd.utils.evaluator import results_dict
    (_, base), (ev, res) = plain_runs["base"], plain_runs["on"]
    assert set(res) == set(base) | {"falls"} and ev.fall_recorder.T == 100
    same_tree({k: v for k, v in res.items() if k != "falls"}, base)          # the score table, the trace and the gait table among them
    assert res["table"].tobytes() == base["table"].tobytes() and res["trace"]["frames"].tobytes() == base["trace"]["frames"].tobytes()
    assert res["gait_table"].tobytes() == base["gait_table"].tobytes() and str(results_dict(res)) == str(results_dict(base))
    falls = res["falls"]          # a random policy on the plane for 0.6 s: whoever fell, the dict is well formed and says what the score table says
    assert falls["frames"].shape[1:] == (100, W) and falls["kept_per_cell"] == 2 and len(falls["columns"]) == W
    assert falls["fell_total"] == round((1.0 - res["overall"]["survival"]) * ev.num_envs) == len(falls["fell_env_ids"])


MODES = dict(tg.MODES, plain=dict(task="go2_flat"), limp=dict(task="go2_flat", **{k: v for k, v in REAL.items() if k not in ("warmup_s", "seconds")}))
LABELS = {"perturbations": ("perturbations", "pert_of_robot", "push_steps"), "limp": ("perturbations", "pert_of_robot", "push_steps"), "sensors": ("sensors", "sensor_of_robot"),
          "maneuvers": ("maneuvers", "maneuver_of_robot", "switch_steps"), "ladder": ("levels", "level_of_robot"), "plain": ()}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_blackbox_next_to_every_mode(emu, mode):
    """an add-on: next to each extra axis it runs, the labels of the mode are there, and per cell the kept robots are the (at most `blackbox`) lowest env ids that fell"""
    over = dict(tg.GAIT, **MODES[mode])
    task = over.pop("task")
    ac = zero_actor() if mode == "limp" else th.small_actor_critic()
    base = th.make_evaluator(emu, task=task, **over)
    res0 = base.evaluate(ac)
    base.close()
    ev = th.make_evaluator(emu, task=task, blackbox=1, blackbox_seconds=0.2, gait=True, record=1, **over)
    res = ev.evaluate(ac)
    assert res["table"].tobytes() == res0["table"].tobytes()
    falls = res["falls"]
    for key in ("group_of_robot", "terrain_names", "scenarios", "cell_names", "cell_of_robot", "fell_per_cell") + LABELS[mode]:
        assert key in falls, key
    assert set(LABELS[mode]) == {k for ks in LABELS.values() for k in ks} & set(falls) and len(falls["cell_names"]) == len(set(falls["cell_names"])) == ev.num_cells
    fell = falls["fell_env_ids"]
    assert falls["fell_total"] == len(fell) == round((1.0 - res["overall"]["survival"]) * ev.num_envs) and falls["frames"].shape[1] == 10
    want = []
    for c in range(ev.num_cells):
        ids = fell[ev.cell_host[fell] == c]
        assert falls["fell_per_cell"][c] == len(ids)
        want += sorted(ids.tolist())[:1]
    assert falls["env_ids"].tolist() == sorted(want) and (np.bincount(falls["cell_of_robot"], minlength=ev.num_cells) <= 1).all()
    if mode == "limp":
        assert len(want) == 4 and falls["fell_total"] > len(want)          # more fell than are kept
    for k, e in enumerate(falls["env_ids"]):          # the recorded robots are the first of every cell: whichever of them fell is in both records
        if e in res["trace"]["env_ids"]:
            j, s, n = res["trace"]["env_ids"].tolist().index(e), int(falls["fall_step"][k]), int(min(falls["length"][k], falls["fall_step"][k] + 1))
            assert falls["frames"][k, 10 - n:].tobytes() == res["trace"]["frames"][s - n + 1:s + 1, j].tobytes()
    again = ev.evaluate(ac)
    same_tree(again["falls"], falls)
    ev.close()
    print("%s: %d robots fell, %d kept" % (mode, falls["fell_total"], len(falls["env_ids"])))


def hand_made_falls():
    """two kept falls, T = 4.  Robot 0 (length 4): upright, then tipping about x by 0.1, 0.4 rad; robot 1 (length 2): one frame before the fall.  dt = 0.02"""
    T, dt = 4, 0.02
    frames = np.full((2, T, W), np.nan, np.float32)
    o = TRACE_OFFSET

    def frame(angle, height, v, cmd, fz, reset=0.0):
        f = np.zeros(W, np.float32)
        f[o["projected_gravity"]:o["projected_gravity"] + 3] = [0.0, np.sin(angle), -np.cos(angle)]
        f[o["root_pos"] + 2] = height
        f[o["root_lin_vel"]:o["root_lin_vel"] + 3] = v
        f[o["commands"]:o["commands"] + 3] = cmd
        f[o["foot_force"] + 2:o["foot_force"] + 12:3] = fz
        f[o["reset"]] = reset
        return f
    frames[0, 0] = frame(0.0, 0.30, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [20.0, 20.0, 20.0, 20.0])
    frames[0, 1] = frame(0.1, 0.28, [0.3, 0.0, 0.0], [1.0, 0.0, 0.0], [20.0, 0.5, 20.0, 0.0])
    frames[0, 2] = frame(0.4, 0.20, [0.3, 0.4, 9.0], [1.0, 0.0, 0.5], [30.0, 1.0, -2.0, 0.0])          # 1.0 is not > the threshold; |-2| is
    frames[0, 3] = frame(0.0, 0.34, [0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [20.0] * 4, reset=1.0)
    frames[1, 2] = frame(0.25, 0.1, [0.0, -2.0, 0.0], [0.0, 0.5, 0.0], [0.0] * 4)
    frames[1, 3] = frame(0.0, 0.34, [0.0, 0.0, 0.0], [0.0, 0.5, 0.0], [20.0] * 4, reset=1.0)
    falls = {"frames": frames, "length": np.asarray([4, 2]), "fall_step": np.asarray([7, 0]), "env_ids": np.asarray([3, 9], np.int32), "fell_total": 3,
             "fell_env_ids": np.asarray([3, 5, 9], np.int32), "steps": 50, "dt": dt, "dof_names": ["j%d" % i for i in range(12)], "foot_names": ["FL_foot", "FR_foot", "RL_foot", "RR_foot"]}
    falls["columns"] = R.column_names(falls["dof_names"], falls["foot_names"])
    falls.update(R.split_frames(frames))
    return falls


def test_fall_summary_and_the_file_round_trip(tmp_path):
    falls = hand_made_falls()
    sm = R.fall_summary(falls)
    assert set(sm) == set(R.FALL_KEYS)
    np.testing.assert_array_equal(sm["time_s"], [7 * 0.02, 0.0])
    np.testing.assert_array_equal(sm["command"], np.asarray([[1.0, 0.0, 0.5], [0.0, 0.5, 0.0]], np.float32))
    np.testing.assert_allclose(sm["tilt"], [0.4, 0.25], rtol=0, atol=1e-6)          # fp32 sin / cos of the angle, back through arccos
    np.testing.assert_array_equal(sm["base_height"], np.asarray([0.20, 0.1], np.float32).astype(np.float64))
    np.testing.assert_allclose(sm["planar_speed"], [0.5, 2.0], rtol=1e-6)
    np.testing.assert_array_equal(sm["feet_in_contact"], [2.0, 0.0])
    np.testing.assert_allclose(sm["max_tilt_rate"][0], 0.3 / 0.02, rtol=1e-5)
    assert np.isnan(sm["max_tilt_rate"][1])
    assert R.fall_summary(falls, contact_threshold=25.0)["feet_in_contact"].tolist() == [1.0, 0.0]
    one = dict(falls, frames=falls["frames"][:, 3:], length=np.asarray([1, 1]))          # nothing but the fall frame: no figure exists
    s1 = R.fall_summary(one)
    assert all(np.isnan(s1[k]).all() for k in R.FALL_KEYS if k != "time_s")
    lines = R.format_falls(falls)
    assert len(lines) == 2 and lines[0].startswith("env 3 fell at 0.14 s (4 frames kept)") and "2 feet down" in lines[0]
    path = R.write_falls(str(tmp_path / "sub" / "f.npz"), falls, extra={"scenarios": ["a", "bb"], "iteration": 7})
    back = R.read_falls(path)
    assert set(back) == set(falls) | {"summary", "scenarios", "iteration"}
    for k, v in falls.items():
        if isinstance(v, np.ndarray):
            assert back[k].dtype == v.dtype and back[k].tobytes() == v.tobytes(), k
        else:
            assert back[k] == v and type(back[k]) is type(v), k
    assert back["scenarios"] == ["a", "bb"] and back["iteration"] == 7 and set(back["summary"]) == set(R.FALL_KEYS)
    for k in R.FALL_KEYS:
        np.testing.assert_array_equal(back["summary"][k], sm[k])
    same_tree(R.fall_summary(back), sm)


def test_cli_prints_the_falls_block_and_writes_the_file(emu, tmp_path, capsys, monkeypatch):
    """a tiny go2_flat run on the oracle, then scripts/evaluate.py --robust --blackbox 2: the falls block is printed, falls_<checkpoint>.npz is written next to the run's
    results, and read_falls + fall_summary read it back"""
    import copy
    import json
    from helpers import load_oracle
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils import get_args
    train_cfg = copy.deepcopy(task_registry.train_cfgs["go2_flat"])
    train_cfg.runner.save_interval = 1
    e = train_cfg.evaluation
    e.num_envs, e.seconds, e.warmup_s, e.push_first_s, e.push_period_s, e.push_window_s = 56, 0.6, 0.1, 0.1, 0.3, 0.2
    monkeypatch.setitem(task_registry.train_cfgs, "go2_flat", train_cfg)
    base = ["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1)
    env.close()
    capsys.readouterr()
    out = evaluate(base + ["--robust", "--blackbox", "2"], log_root=str(tmp_path), env_kwargs={"lib": load_oracle()}, evaluator_kwargs={"nn_lib": emu})
    text = capsys.readouterr().out
    row = out["checkpoints"][-1]
    assert "falls (first counted fall per robot)" in text and "robots_fell" in text and json.loads([l for l in text.splitlines() if l.startswith("{")][-1])["best"] == out["best"]
    path = [l.split("falls: ", 1)[1] for l in text.splitlines() if l.startswith("falls: ")][-1]
    assert os.path.basename(path) == "falls_1.npz" and os.path.basename(os.path.dirname(path)) == "eval_results" and os.path.exists(path)
    back = R.read_falls(path)
    assert back["fell_total"] == row["robots_fell"] == round((1.0 - row["overall"]["survival"]) * 56) and back["kept_per_cell"] == 2 and back["frames"].shape[1:] == (100, W)
    assert back["perturbations"][0] == "nominal" and len(back["cell_names"]) == len(back["fell_per_cell"]) == 6 * 7          # plane x six scenarios x seven perturbations
    sm = R.fall_summary(back)
    assert set(sm) == set(R.FALL_KEYS) and len(sm["time_s"]) == len(back["env_ids"]) <= 2 * int((back["fell_per_cell"] > 0).sum())
    for k in R.FALL_KEYS:
        np.testing.assert_array_equal(back["summary"][k], sm[k])


def test_refused_configurations(emu):
    with pytest.raises(ValueError, match="blackbox_seconds"):
        th.make_evaluator(emu, num_envs=12, blackbox=1, blackbox_seconds=0.02)          # one step
    with pytest.raises(ValueError, match="evaluation.blackbox"):
        th.make_evaluator(emu, num_envs=12, blackbox=-1)
    with pytest.raises(ValueError, match=r"12 robots x 100 steps x 448 bytes.*537600.*500000"):
        th.make_evaluator(emu, num_envs=12, blackbox=1, blackbox_max_bytes=500000)
    ev = th.make_evaluator(emu, num_envs=12, blackbox=1, blackbox_max_bytes=537600, seconds=0.1, warmup_s=0.0)          # exactly the cap is allowed
    assert ev.fall_recorder.frames.numel() * 4 == 537600
    with pytest.raises(ValueError, match="did not fall"):
        ev.fall_recorder.fetch(lambda fell: np.asarray([0]))
    ev.close()
    env, _ = tt.make_env()
    with pytest.raises(RuntimeError, match="nn_lib"):
        R.FallRecorder(env, 4)          # no CPU product path
    with pytest.raises(ValueError, match="at least 1 step"):
        R.FallRecorder(env, 0.001, nn_lib=emu)
    assert R.FallRecorder(env, 0.1, nn_lib=emu).T == 5 and R.FallRecorder(env, 7, nn_lib=emu).T == 7
    env.close()
