"""TrajectoryRecorder — per-step frames of chosen robots, recorded on the device, and what is made of them on the host.

The simulator holds root state, joints, torques, foot positions and foot contact forces of every robot after every step; scripts/play.py and the policy evaluator throw them
away.  A recorder keeps them for a few robots: record() is ONE go2nn_trace_record call (include/go2nn.h, csrc/go2nn_trace.h; two small launches, no host read) that copies
the frame of every tracked robot into a device-resident ring [capacity, K, 112] at the slot a device-side cursor names, so it works inside a captured HIP graph, and fetch()
is the one device -> host copy at the end.  The frame's columns are specified once, by the enum GO2NN_TRACE_* of include/go2nn.h; _nn.TRACE_BLOCKS restates it for slicing.

A frame is the state AFTER the env step: a robot that fell during the step shows its post-reset pose, with the reset flag set (gait_summary restarts its bookkeeping there).

FallRecorder is the black box next to it: the same frame, but a ring for EVERY robot that stops at the robot's first counted fall, so the robot that fell — almost never one
of the few tracked ones — leaves its last seconds behind (fall_summary, write_falls / read_falls).

The trace file (write_trace) is one .npz of named arrays that numpy, a plotting script or a MuJoCo viewer on a workstation reads; `qpos` is MuJoCo's generalised position
of the Go2 model (mujoco_qpos).  There is no CPU product path: on a host simulator library the recorder needs the go2nn host build handed in (tests only)."""
import ctypes as C
import os

import numpy as np
import torch

from .._nn import BLACKBOX_ROWS, GO2NN_BLACKBOX_NUM, GO2NN_TRACE_WIDTH, TRACE_BLOCKS, TRACE_FIELDS, TRACE_OFFSET, Go2nnTraceIn, trace_env_ids

FOOT_BLOCKS = ("foot_pos", "foot_vel", "foot_force")
FLAG_BLOCKS = ("reset", "time_out")
GAIT_KEYS = ("duty_factor", "touchdowns", "stride_frequency", "stance_time", "swing_time", "slip_speed", "swing_height")
_AXES = {3: "xyz", 4: "xyzw"}


def column_names(dof_names, foot_names):
    """the 112 column names of a frame, e.g. root_pos.x, dof_pos.FL_hip_joint, foot_force.FL_foot.z, reward"""
    out = []
    for name, w in TRACE_BLOCKS:
        if name in FOOT_BLOCKS:
            out += ["%s.%s.%s" % (name, f, a) for f in foot_names for a in "xyz"]
        elif w == 12:
            out += ["%s.%s" % (name, j) for j in dof_names]
        elif w == 1:
            out.append(name)
        else:
            out += ["%s.%s" % (name, a) for a in (("vx", "vy", "yaw_rate") if name == "commands" else _AXES[w])]
    return out


def split_frames(frames):
    """frames [steps, K, 112] -> {block: array}: [steps, K, w], the foot blocks as [steps, K, 4, 3], reward [steps, K], the flags as bool [steps, K]"""
    out = {}
    for name, w in TRACE_BLOCKS:
        a = frames[..., TRACE_OFFSET[name]:TRACE_OFFSET[name] + w]
        if name in FOOT_BLOCKS:
            a = a.reshape(a.shape[:-1] + (4, 3))
        elif w == 1:
            a = a[..., 0] != 0 if name in FLAG_BLOCKS else a[..., 0]
        out[name] = np.ascontiguousarray(a)
    return out


class TrajectoryRecorder:
    def __init__(self, env, env_ids, capacity, nn_lib=None):
        """env: a LeggedRobot;  env_ids: the tracked robots, strictly increasing, each in [0, env.num_envs);  capacity: slots of the ring — after more than `capacity`
        record() calls it holds the last `capacity` steps.  nn_lib: the go2nn library (tests hand in the host build; the product passes nothing)."""
        on_device = env.lib.go2sim_is_device_library() == 1
        if nn_lib is None:
            if not on_device:
                raise RuntimeError("TrajectoryRecorder on a host simulator library needs the go2nn host build passed as nn_lib (tests only)")
            from .._nn import load_nn
            nn_lib = load_nn()
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %r" % (capacity,))
        self.nn, self.on_device, self.device = nn_lib, on_device, env.device
        ids = trace_env_ids(env_ids, env.num_envs)
        self.env_ids_host, self.K, self.T = ids, len(ids), int(capacity)
        self.env_ids = torch.from_numpy(ids).to(self.device)
        # frames and cursor share one allocation, the cursor being its last element: fetch() is one copy
        self._store = torch.zeros(self.T * self.K * GO2NN_TRACE_WIDTH + 1, device=self.device)
        self.frames = self._store[:-1].view(self.T, self.K, GO2NN_TRACE_WIDTH)
        self.cursor = self._store[-1:].view(torch.int32)
        self.bind(env)

    def bind(self, env):
        """point the recorder at `env`'s buffers (the evaluator builds a fresh simulator of the same shape per evaluation)"""
        if env.num_envs <= int(self.env_ids_host[-1]):
            raise ValueError("the simulator has %d envs, env_ids reach %d" % (env.num_envs, int(self.env_ids_host[-1])))
        self._bind_sources(env)

    def _bind_sources(self, env):
        """Go2nnTraceIn over `env`'s buffers, and the names a fetched record carries"""
        self.env, b, a = env, env._buf, Go2nnTraceIn()
        for name in TRACE_FIELDS:
            t, f = b[name], getattr(a, name)
            f.p, f.env_stride, f.comp_stride = t.data_ptr(), t.stride(0), (t.stride(t.dim() - 1) if t.dim() > 1 else 0)
        a.dof_state.comp_stride, a.dof_vel_offset = b["dof_state"].stride(1), b["dof_state"].stride(2)
        a.rigid_body_stride, a.contact_body_stride = b["rigid_body_states"].stride(1), b["contact_forces"].stride(1)
        feet = [int(i) for i in env.feet_indices.tolist()]
        a.foot_body[:] = feet
        self._in = a
        self.dt = float(env.dt)
        self.dof_names, self.foot_names = list(env.dof_names), [env.body_names[i] for i in feet]

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.on_device else None

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, self.nn.go2nn_last_error().decode()))

    def record(self):
        """the current state of the tracked robots -> the ring's next slot (pure enqueue on the current stream; capturable)"""
        self._check(self.nn.go2nn_trace_record(C.byref(self._in), C.c_void_p(self.env_ids.data_ptr()), self.K, C.c_void_p(self.frames.data_ptr()),
                                               C.c_void_p(self.cursor.data_ptr()), self.T, self._stream()), "go2nn_trace_record")

    def clear(self):
        self._check(self.nn.go2nn_trace_clear(C.c_void_p(self.cursor.data_ptr()), self._stream()), "go2nn_trace_clear")

    def fetch(self):
        """-> the trace: {"frames" [steps, K, 112] in time order and every block of it by name (split_frames), "steps_recorded" (the cursor: record() calls since the last
        clear; steps = min(it, capacity)), "env_ids", "dt", "dof_names", "foot_names", "columns"}.  The one device -> host copy (and synchronisation)."""
        host = self._store.cpu().numpy()
        count = int(host[-1:].view(np.int32)[0])
        ring = host[:-1].reshape(self.T, self.K, GO2NN_TRACE_WIDTH)
        frames = ring[:count] if count <= self.T else np.roll(ring, -(count % self.T), axis=0)          # the oldest kept step is in slot count % T
        trace = {"frames": np.ascontiguousarray(frames)}
        trace.update(split_frames(trace["frames"]))
        trace.update(steps_recorded=count, env_ids=self.env_ids_host.copy(), dt=self.dt, dof_names=list(self.dof_names), foot_names=list(self.foot_names),
                     columns=column_names(self.dof_names, self.foot_names))
        return trace


class FallRecorder:
    """The black box: for EVERY robot of the simulator a ring of the last T frames, which stops for a robot when that robot falls (reset without a time-out, on a counted
    step) and stays stopped while the simulator resets the robot and carries on.  record() is ONE go2nn_blackbox_record call (include/go2nn.h, csrc/go2nn_blackbox.h; two
    small launches, no host read, capturable); the rings [N, T, 112] and the small int32 state block live on the device; fetch() reads the state block, gathers the rings of
    the fallen robots it is asked to keep on the device and copies those.  Only a robot's FIRST counted fall is kept.  A ring's last frame is the fall step's own frame,
    i.e. the post-reset pose with the reset flag set (the recorder's convention): the frames before it are the fall, and it is not the moment of impact."""

    def __init__(self, env, seconds_or_steps, nn_lib=None):
        """env: a LeggedRobot;  seconds_or_steps: the ring's length — an int is a number of steps, a float a time in seconds (rounded to steps of env.dt); at least 1 step.
        nn_lib: the go2nn library (tests hand in the host build; the product passes nothing)."""
        on_device = env.lib.go2sim_is_device_library() == 1
        if nn_lib is None:
            if not on_device:
                raise RuntimeError("FallRecorder on a host simulator library needs the go2nn host build passed as nn_lib (tests only)")
            from .._nn import load_nn
            nn_lib = load_nn()
        T = int(seconds_or_steps) if isinstance(seconds_or_steps, (int, np.integer)) else int(round(float(seconds_or_steps) / float(env.dt)))
        if T < 1:
            raise ValueError("the ring needs at least 1 step, got %r (%d steps of %.4f s)" % (seconds_or_steps, T, float(env.dt)))
        self.nn, self.on_device, self.device = nn_lib, on_device, env.device
        self.N, self.T = int(env.num_envs), T
        self.frames = torch.zeros(self.N, self.T, GO2NN_TRACE_WIDTH, device=self.device)
        self.state = torch.zeros(GO2NN_BLACKBOX_NUM * self.N + 1, dtype=torch.int32, device=self.device)
        self.bind(env)
        self.begin(0)

    def bind(self, env):
        """point the recorder at `env`'s buffers (the evaluator builds a fresh simulator of the same shape per evaluation)"""
        if env.num_envs != self.N:
            raise ValueError("the simulator has %d envs, the black box was built for %d" % (env.num_envs, self.N))
        self._bind_sources(env)

    _bind_sources, _stream, _check = TrajectoryRecorder._bind_sources, TrajectoryRecorder._stream, TrajectoryRecorder._check

    def begin(self, first_step=0):
        """no robot frozen, every ring empty; the step counter starts at `first_step` (negative: that many uncounted warm-up steps, whose falls only restart a ring)"""
        self._check(self.nn.go2nn_blackbox_begin(C.c_void_p(self.state.data_ptr()), self.N, int(first_step), self._stream()), "go2nn_blackbox_begin")

    def record(self):
        """the current state of every robot that has not fallen yet -> its ring's next slot (pure enqueue on the current stream; capturable)"""
        self._check(self.nn.go2nn_blackbox_record(C.byref(self._in), self.N, C.c_void_p(self.frames.data_ptr()), C.c_void_p(self.state.data_ptr()), self.T, self._stream()),
                    "go2nn_blackbox_record")

    def fetch(self, keep=None):
        """keep: None = every fallen robot, or a function (sorted env ids of the fallen robots) -> the env ids to keep.
        -> the falls: {"frames" [F, T, 112] in time order and RIGHT-ALIGNED — [:, -1] is the fall frame, [:, -2] the last frame before the fall, slots before a robot's
        `length` are NaN —, every block of it by name (split_frames; the flags False in the padding), per kept robot "length", "fall_step" (the counted step of the fall =
        the index of its frame in a trace of the counted steps) and "env_ids" [F]; over all robots "fell_total" and "fell_env_ids"; "steps" (the step counter), "dt",
        "dof_names", "foot_names", "columns"}.  Two device -> host copies: the state block, then the kept rings."""
        state = self.state.cpu().numpy()
        rows = state[:-1].reshape(GO2NN_BLACKBOX_NUM, self.N)
        written, frozen, fall_step = (rows[BLACKBOX_ROWS.index(k)] for k in BLACKBOX_ROWS)
        fell = np.nonzero(frozen != 0)[0].astype(np.int64)
        ids = fell if keep is None else np.sort(np.asarray(keep(fell), np.int64).reshape(-1))
        if len(ids) and not np.isin(ids, fell).all():
            raise ValueError("keep() returned robots that did not fall: %s" % sorted(set(ids.tolist()) - set(fell.tolist())))
        T = self.T
        rings = self.frames.index_select(0, torch.from_numpy(ids).to(self.device)).cpu().numpy() if len(ids) else np.zeros((0, T, GO2NN_TRACE_WIDTH), np.float32)
        length = np.minimum(written[ids], T).astype(np.int64)
        frames = np.full((len(ids), T, GO2NN_TRACE_WIDTH), np.nan, np.float32)
        for k in range(len(ids)):          # the oldest kept frame is in slot (written - length) % T
            n = int(length[k])
            frames[k, T - n:] = rings[k, (int(written[ids[k]]) - n + np.arange(n)) % T]
        falls = {"frames": frames}
        falls.update(split_frames(frames))
        valid = np.arange(T)[None, :] >= (T - length)[:, None]
        for name in FLAG_BLOCKS:
            falls[name] &= valid
        falls.update(length=length, fall_step=fall_step[ids].astype(np.int64), env_ids=ids.astype(np.int32), fell_total=int(len(fell)), fell_env_ids=fell.astype(np.int32),
                     steps=int(state[-1]), dt=self.dt, dof_names=list(self.dof_names), foot_names=list(self.foot_names), columns=column_names(self.dof_names, self.foot_names))
        return falls


FALL_KEYS = ("time_s", "command", "tilt", "base_height", "planar_speed", "feet_in_contact", "max_tilt_rate")


def _tilt(projected_gravity):
    """angle [rad] between the base's z axis and the world's, from the gravity direction in the base frame (0 upright, pi upside down)"""
    g = np.asarray(projected_gravity, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.arccos(np.clip(-g[..., 2] / np.linalg.norm(g, axis=-1), -1.0, 1.0))


def fall_summary(falls, contact_threshold=1.0):
    """Per kept fall (host numpy) -> {key: [F]} ("command" [F, 3]):
      time_s           [s] fall_step * dt: when, in the counted horizon, the step that ended in the fall was taken
      command          vx, vy, yaw rate on the last frame before the fall
      tilt             [rad] angle of the base's z axis from the vertical on the last frame before the fall (from projected_gravity)
      base_height      [m] root_pos z there;  planar_speed [m/s]: |root_lin_vel xy| there
      feet_in_contact  feet with |foot_force z| > contact_threshold there (the gait rule's threshold)
      max_tilt_rate    [rad/s] largest |tilt difference| / dt between consecutive kept frames before the fall
    NaN where the ring holds no frame before the fall (length < 2; max_tilt_rate: length < 3).  The fall frame itself ([:, -1]) shows the post-reset pose and is not used."""
    frames, length, dt = np.asarray(falls["frames"]), np.asarray(falls["length"]), float(falls["dt"])
    F, T = frames.shape[:2]
    b = split_frames(frames)
    nan = np.full(F, np.nan)
    out = {"time_s": np.asarray(falls["fall_step"], np.float64) * dt, "command": np.full((F, 3), np.nan), "tilt": nan.copy(), "base_height": nan.copy(),
           "planar_speed": nan.copy(), "feet_in_contact": nan.copy(), "max_tilt_rate": nan.copy()}
    if T < 2 or F == 0:
        return out
    has = length >= 2
    tilt = _tilt(b["projected_gravity"])          # [F, T]; NaN in the padding
    out["command"][has] = b["commands"][has, -2]
    out["tilt"][has] = tilt[has, -2]
    out["base_height"][has] = b["root_pos"][has, -2, 2]
    out["planar_speed"][has] = np.hypot(b["root_lin_vel"][has, -2, 0].astype(np.float64), b["root_lin_vel"][has, -2, 1].astype(np.float64))
    out["feet_in_contact"][has] = (np.abs(b["foot_force"][has, -2, :, 2]) > contact_threshold).sum(-1)
    if T >= 3:
        rate = np.abs(np.diff(tilt[:, :-1], axis=1)) / dt          # between the frames before the fall; NaN where either is padding
        some = (length >= 3) & np.isfinite(rate).any(1)
        out["max_tilt_rate"][some] = np.nanmax(rate[some], axis=1)
    return out


def format_falls(falls, summary=None):
    """one line per kept fall"""
    s = fall_summary(falls) if summary is None else summary
    return ["env %d fell at %.2f s (%d frames kept): cmd (%.2f, %.2f, %.2f)  tilt %.2f rad  height %.3f m  speed %.2f m/s  %s feet down  max tilt rate %.2f rad/s"
            % (int(e), s["time_s"][k], int(falls["length"][k]), s["command"][k, 0], s["command"][k, 1], s["command"][k, 2], s["tilt"][k], s["base_height"][k],
               s["planar_speed"][k], "%d" % s["feet_in_contact"][k] if np.isfinite(s["feet_in_contact"][k]) else "nan", s["max_tilt_rate"][k])
            for k, e in enumerate(np.asarray(falls["env_ids"]))]


def write_falls(path, falls, extra=None):
    """one .npz: every entry of the falls dict, the summary as flat arrays summary_<key> (fall_summary) and whatever `extra` holds (arrays, numbers, lists of names)"""
    d = {k: np.asarray(v) for k, v in falls.items()}
    for k, v in fall_summary(falls).items():
        d["summary_" + k] = v
    for k, v in (extra or {}).items():
        d[k] = np.asarray(v)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **d)
    return path


def read_falls(path):
    """-> what write_falls was given, as fetch() returns it (numbers as Python numbers, name lists as lists), with the extras and "summary": {key: array}"""
    out, summary = {}, {}
    with np.load(path, allow_pickle=False) as z:
        for k in z.files:
            v = z[k]
            if k.startswith("summary_"):
                summary[k[8:]] = v
            elif v.dtype.kind == "U":
                out[k] = v.tolist()
            else:
                out[k] = v.item() if v.ndim == 0 else v
    out["summary"] = summary
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def mujoco_qpos(trace):
    """-> [steps, K, 19]: MuJoCo's qpos of the free-floating Go2 — root position, root quaternion in MuJoCo's order WXYZ (the simulator and the frame hold xyzw), then the
    twelve joint angles.  The joint order (FL, FR, RL, RR; hip, thigh, calf) is already the one of the reference's deploy/deploy_mujoco/configs/go2.yaml: the quaternion
    order is the only change.  No MuJoCo replay is part of this project's tests; this convention is."""
    q = trace["root_quat"]
    return np.concatenate([trace["root_pos"], q[..., 3:4], q[..., 0:3], trace["dof_pos"]], axis=-1)


def _runs(mask):
    """maximal runs of True in a 1-d bool array -> [(first, last + 1)]"""
    edge = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return list(zip(np.nonzero(edge == 1)[0].tolist(), np.nonzero(edge == -1)[0].tolist()))


def gait_summary(trace, contact_threshold=1.0):
    """Per robot and foot, from the recorded vertical contact force: a foot is in contact on a frame when foot_force z > contact_threshold (the reference's `> 1 N` rule,
    legged_robot.py _reward_feet_air_time).  Frames with the reset flag set are skipped and split a robot's record into SEGMENTS; no phase is followed across one.
    -> {key: [K, 4]} (NaN where a quantity has no sample) plus "frames_used" [K]:
      duty_factor       contact frames / frames used
      touchdowns        swing -> contact transitions inside a segment (int)
      stride_frequency  [Hz] 1 / mean time between consecutive touchdowns of a segment
      stance_time       [s] mean length of the COMPLETE stance phases (touchdown and lift-off both seen in the segment);  swing_time: the same for swings
      slip_speed        [m/s] mean horizontal speed of the foot over its contact frames
      swing_height      [m] highest foot position (world z) of each complete swing, averaged
    Host numpy on a few hundred frames.  The evaluator's device-side scorer (csrc/go2nn_gait.h, `evaluation.gait`) follows the same rule for every robot and is tested
    against this function: change the two together."""
    force, pos, vel, reset, dt = trace["foot_force"], trace["foot_pos"], trace["foot_vel"], trace["reset"], float(trace["dt"])
    S, K = reset.shape
    out = {k: np.full((K, 4), np.nan) for k in GAIT_KEYS}
    out["touchdowns"] = np.zeros((K, 4), np.int64)
    out["frames_used"] = (~reset).sum(0).astype(np.int64)
    for k in range(K):
        segments = _runs(~reset[:, k])
        for f in range(4):
            contact = force[:, k, f, 2] > contact_threshold
            speed = np.hypot(vel[:, k, f, 0].astype(np.float64), vel[:, k, f, 1].astype(np.float64))
            used = n_contact = touchdowns = 0
            slip, strides, stances, swings, heights = 0.0, [], [], [], []
            for a, b in segments:
                c = contact[a:b]
                used += b - a
                n_contact += int(c.sum())
                slip += float(speed[a:b][c].sum())
                downs = [a + i for i, _ in _runs(c) if i > 0]          # a run that starts the segment is not a touchdown: the swing before it was not seen
                touchdowns += len(downs)
                strides += np.diff(downs).tolist()
                stances += [j - i for i, j in _runs(c) if i > 0 and j < b - a]
                for i, j in _runs(~c):
                    if i > 0 and j < b - a:
                        swings.append(j - i)
                        heights.append(float(pos[a + i:a + j, k, f, 2].max()))
            out["touchdowns"][k, f] = touchdowns
            if used:
                out["duty_factor"][k, f] = n_contact / used
            if n_contact:
                out["slip_speed"][k, f] = slip / n_contact
            if strides:
                out["stride_frequency"][k, f] = 1.0 / (float(np.mean(strides)) * dt)
            if stances:
                out["stance_time"][k, f] = float(np.mean(stances)) * dt
            if swings:
                out["swing_time"][k, f] = float(np.mean(swings)) * dt
                out["swing_height"][k, f] = float(np.mean(heights))
    return out


def format_gait(trace, gait=None):
    """one line per robot: duty factor and stride frequency of the four feet"""
    gait = gait_summary(trace) if gait is None else gait
    names = [n.replace("_foot", "") for n in trace["foot_names"]]
    return ["env %d: %s" % (int(e), "  ".join("%s duty %.2f stride %.2f Hz" % (n, gait["duty_factor"][k, f], gait["stride_frequency"][k, f]) for f, n in enumerate(names)))
            for k, e in enumerate(np.asarray(trace["env_ids"]))]


def write_trace(path, trace, extra=None):
    """one .npz: every entry of the trace, `qpos` (mujoco_qpos), the gait summary as flat arrays gait_<key> and whatever `extra` holds (arrays, numbers, lists of names)"""
    d = {k: np.asarray(v) for k, v in trace.items()}
    d["qpos"] = mujoco_qpos(trace)
    for k, v in gait_summary(trace).items():
        d["gait_" + k] = v
    for k, v in (extra or {}).items():
        d[k] = np.asarray(v)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **d)
    return path


def read_trace(path):
    """-> what write_trace was given, as fetch() returns it (numbers as Python numbers, name lists as lists), with `qpos`, the extras and "gait": {key: [K, 4]}"""
    out, gait = {}, {}
    with np.load(path, allow_pickle=False) as z:
        for k in z.files:
            v = z[k]
            if k.startswith("gait_"):
                gait[k[5:]] = v
            elif v.dtype.kind == "U":
                out[k] = v.tolist()
            else:
                out[k] = v.item() if v.ndim == 0 else v
    out["gait"] = gait
    return out


def write_spectrum(path, spectrum):
    """one .npz of the evaluator's mean power spectra (res["spectrum_psd"]): `freqs` [K] in Hz, `psd` [cells, 2, 3, K] — per cell of the active mode, signal and joint kind
    the mean over the used windows and the kind's 4 joints, NaN for a cell without a used window —, the names `cell_names`, `signals`, `kinds`, and the estimator's
    `window`, `cutoff_hz` and `fs`"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **{k: np.asarray(v) for k, v in spectrum.items()})
    return path


def read_spectrum(path):
    """-> what write_spectrum was given (numbers as Python numbers, name lists as lists)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: (z[k].tolist() if z[k].dtype.kind == "U" else z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files}
