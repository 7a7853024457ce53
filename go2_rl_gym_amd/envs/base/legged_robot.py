"""LeggedRobot — the reference's vectorised environment surface (legged_gym/envs/base/legged_robot.py) as a thin
host layer over the go2sim C ABI.

Everything the reference computes per env in ~300 eager torch launches per step (torque loop :73-92,
post_physics_step :102-142 and all it calls) happens inside ONE HIP kernel launch per step
(go2_rl_gym_amd/csrc); this class only translates the config, owns the handle, exposes the library's buffers
under the attribute names the reference uses and keeps the Python-visible scalars
(common_step_counter, curricula) in sync.
"""
import ctypes as C
from itertools import product

import numpy as np
import torch

from ... import _abi
from ...utils.helpers import class_to_dict
from .base_task import BaseTask, wrap_buffers
from .legged_robot_config import LeggedRobotCfg

_DOF_NAMES = [f"{l}_{j}_joint" for l in ("FL", "FR", "RL", "RR") for j in ("hip", "thigh", "calf")]
_BODY_NAMES = ["base", "Head_upper", "Head_lower"] + [f"{l}_{p}" for l in ("FL", "FR", "RL", "RR") for p in ("hip", "thigh", "calf", "foot")]
# reference reward-scale keys that differ from the enum spelling
_REWARD_KEY_ALIASES = {"feet_stumble": "stumble"}


class LeggedRobot(BaseTask):
    _terrain_prebuilt = None      # a utils.terrain.Terrain to use instead of generating one (utils/evaluator.py recreates its simulator per evaluation and keeps the terrain on the host)

    _sensors = None               # the sensor randomisation's buffers (domain_rand.randomize_sensors; None: the policy reads the simulator's own observation)

    def __init__(self, cfg: LeggedRobotCfg, sim_params, physics_engine, sim_device, headless, lib=None, env_offset=0, num_envs_global=None, nn=None):
        self.cfg = cfg
        self.sim_params = sim_params
        self.height_samples = None
        self.debug_viz = False
        self.init_done = False
        self._env_offset = int(env_offset)
        self._num_envs_global = num_envs_global
        self._parse_cfg(self.cfg)
        super().__init__(self.cfg, sim_params, physics_engine, sim_device, headless, lib=lib)
        self._init_buffers()
        if getattr(self.cfg.domain_rand, "randomize_sensors", False):
            self._init_sensors(nn)
        self.init_done = True
        self.num_steps_per_env = 24          # hard-coded in the reference env (:58)
        self.reward_curriculum_configs = list(getattr(self.cfg.rewards, "curriculum_rewards", None) or [])

    # ------------------------------------------------------------------ config -> Go2SimCfg
    def _parse_cfg(self, cfg):
        sim_dt = self.sim_params.dt if hasattr(self.sim_params, "dt") else self.sim_params["sim"]["dt"]
        self.dt = cfg.control.decimation * sim_dt                                  # :1094
        self.obs_scales = cfg.normalization.obs_scales
        self.reward_scales = class_to_dict(cfg.rewards.scales)
        self.command_ranges = class_to_dict(cfg.commands.ranges)
        self.max_episode_length_s = cfg.env.episode_length_s
        self.max_episode_length = np.ceil(self.max_episode_length_s / self.dt)     # :1104
        cfg.domain_rand.push_interval = np.ceil(cfg.domain_rand.push_interval_s / self.dt)   # :1106
        self._sim_dt = sim_dt

    def _fill_cfg(self):
        cfg, abi = self.cfg, self.abi
        c = abi.Cfg()
        self.lib.go2sim_default_cfg(C.byref(c))
        N = cfg.env.num_envs
        c.num_envs, c.env_offset = N, self._env_offset
        c.num_envs_global = self._num_envs_global if self._num_envs_global is not None else self._env_offset + N
        c.seed = int(getattr(cfg, "seed", 1)) & 0xFFFFFFFFFFFFFFFF
        c.sim_dt, c.decimation = self._sim_dt, cfg.control.decimation
        g = cfg.sim.gravity
        for i in range(3):
            c.gravity[i] = g[i]
        sol = getattr(cfg.sim, "solver", None)
        if sol is not None:
            c.solver_iterations, c.erp, c.contact_cfm, c.joint_limit_margin = sol.iterations, sol.erp, sol.cfm, sol.joint_limit_margin
        px = cfg.sim.physx
        c.contact_offset, c.max_depenetration_velocity, c.bounce_threshold_velocity = px.contact_offset, px.max_depenetration_velocity, px.bounce_threshold_velocity
        c.joint_armature = cfg.asset.armature
        c.max_linear_velocity, c.max_angular_velocity = cfg.asset.max_linear_velocity, cfg.asset.max_angular_velocity
        mesh = cfg.terrain.mesh_type
        if mesh == "plane":
            c.terrain_mode = 0
        elif mesh in ("heightfield", "trimesh"):
            # create_sim (:292-310): the Terrain is built on the host; the library copies the int16 samples to HBM at create.
            from ...utils.terrain import Terrain
            self.terrain = self._terrain_prebuilt if self._terrain_prebuilt is not None else Terrain(cfg.terrain, c.num_envs_global)
            hs = np.ascontiguousarray(self.terrain.heightsamples, dtype=np.int16)
            org = np.ascontiguousarray(self.terrain.env_origins, dtype=np.float32)
            ids = np.ascontiguousarray(self.terrain.cols2id, dtype=np.int32)
            if ids.shape[0] == 0:
                # Terrain fills cols2id only in curiculum() (utils/terrain.py); with terrain.curriculum off (play.py) the reference has no
                # terrain_ids and falls back to the global command ranges / the default tracking sigma (legged_robot.py:863,1074-1075,1303).
                # The library's sentinel for "no terrain kind" is -1.
                ids = np.full(cfg.terrain.num_cols, -1, dtype=np.int32)
            if ids.shape[0] != cfg.terrain.num_cols:
                raise ValueError("terrain.cols2id has %d entries for %d columns" % (ids.shape[0], cfg.terrain.num_cols))
            self._terrain_host = (hs, org, ids)                                    # keep alive until go2sim_create has copied them
            if mesh == "trimesh":
                # _create_trimesh (:1127-1141) hands PhysX the mesh convert_heightfield_to_trimesh builds WITH terrain.slope_treshold: steep
                # edges become vertical faces.  The library's contact query gets that surface cell by cell (utils/terrain.py)
                cells = np.ascontiguousarray(self.terrain.cell_heights, dtype=np.int16)
                self._terrain_host = (hs, org, ids, cells)
                c.hf_cells = cells.ctypes.data_as(type(c.hf_cells))
                c.hf_walls = 1
            c.terrain_mode = 1
            c.hf_rows, c.hf_cols = self.terrain.tot_rows, self.terrain.tot_cols
            c.hf_samples = hs.ctypes.data_as(type(c.hf_samples))
            c.terrain_origins = org.ctypes.data_as(type(c.terrain_origins))
            c.terrain_type_id = ids.ctypes.data_as(type(c.terrain_type_id))
        else:
            raise ValueError("Terrain mesh type not recognised. Allowed types are [plane, heightfield, trimesh]")
        t = cfg.terrain
        c.terrain_friction, c.terrain_restitution = t.static_friction, t.restitution
        c.hf_hscale, c.hf_vscale, c.hf_border = t.horizontal_scale, t.vertical_scale, (t.border_size if mesh != "plane" else 0.0)
        c.terrain_num_levels, c.terrain_num_types = t.num_rows, t.num_cols
        c.terrain_curriculum, c.max_init_terrain_level = int(t.curriculum), t.max_init_terrain_level
        c.move_down_by_accumulated_xy_command = int(t.move_down_by_accumulated_xy_command)
        c.terrain_length, c.env_spacing, c.measure_heights = t.terrain_length, cfg.env.env_spacing, int(t.measure_heights)
        # PD gains / default pose by substring match of the joint name (:843-859)
        for i, name in enumerate(_DOF_NAMES):
            c.default_dof_pos[i] = cfg.init_state.default_joint_angles[name]
            c.kp[i] = c.kd[i] = 0.0
            for key in cfg.control.stiffness:
                if key in name:
                    c.kp[i], c.kd[i] = cfg.control.stiffness[key], cfg.control.damping[key]
        if cfg.control.control_type not in ("P", "V", "T"):
            raise NameError(f"Unknown controller type: {cfg.control.control_type}")          # legged_robot.py:616-617
        c.control_type = "PVT".index(cfg.control.control_type)
        c.action_scale, c.clip_actions, c.clip_observations = cfg.control.action_scale, cfg.normalization.clip_actions, cfg.normalization.clip_observations
        init = cfg.init_state.pos + cfg.init_state.rot + cfg.init_state.lin_vel + cfg.init_state.ang_vel      # :1000
        for i in range(13):
            c.base_init_state[i] = init[i]
        ist = cfg.init_state                                                                                   # turn_over (:642-684)
        c.turn_over = int(bool(getattr(ist, "turn_over", False)))
        if c.turn_over:
            for k in range(3):
                c.turn_over_proportions[k] = ist.turn_over_proportions[k]
            for k, key in enumerate(("backflip", "sideflip")):
                c.turn_over_init_heights[k][0], c.turn_over_init_heights[k][1] = ist.turn_over_init_heights[key]
                c.turn_over_zero_time[k] = cfg.commands.turn_over_zero_time[key]
            c.turn_over_roll_threshold = cfg.rewards.turn_over_roll_threshold
        d = cfg.domain_rand
        for flag, rng, src in (("randomize_friction", "friction_range", d.friction_range), ("randomize_restitution", "restitution_range", d.restitution_range),
                               ("randomize_base_mass", "added_mass_range", d.added_mass_range), ("randomize_link_mass", "link_mass_range", d.multiplied_link_mass_range),
                               ("randomize_base_com", "base_com_range", d.added_base_com_range), ("randomize_motor_zero_offset", "motor_zero_offset_range", d.motor_zero_offset_range),
                               ("randomize_motor_strength", "motor_strength_range", d.motor_strength_range)):
            setattr(c, flag, int(getattr(d, flag)))
            getattr(c, rng)[0], getattr(c, rng)[1] = src[0], src[1]
        c.randomize_pd_gains = int(d.randomize_pd_gains)
        c.stiffness_mult_range[0], c.stiffness_mult_range[1] = d.stiffness_multiplier_range
        c.damping_mult_range[0], c.damping_mult_range[1] = d.damping_multiplier_range
        c.push_robots, c.push_interval, c.max_push_vel_xy, c.max_push_ang_vel = int(d.push_robots), int(d.push_interval), d.max_push_vel_xy, d.max_push_ang_vel
        c.randomize_action_delay = int(d.randomize_action_delay)
        cm = cfg.commands
        c.cmd_tracking_curriculum, c.cmd_max_curriculum = int(getattr(cm, "curriculum", False)), float(getattr(cm, "max_curriculum", 1.0))
        c.cmd_resampling_time, c.heading_command, c.dynamic_resample_commands = cm.resampling_time, int(cm.heading_command), int(cm.dynamic_resample_commands)
        c.limit_vel_prob, c.limit_vel_invert_when_continuous, c.stop_heading_at_limit = cm.limit_vel_prob, int(cm.limit_vel_invert_when_continuous), int(cm.stop_heading_at_limit)
        c.limit_ang_vel_at_zero_command_prob = cm.limit_ang_vel_at_zero_command_prob
        comb = list(product(cm.limit_vel["lin_vel_x"], cm.limit_vel["lin_vel_y"], cm.limit_vel["ang_vel_yaw"]))     # :827-831
        c.limit_vel_comb_count = len(comb)
        for i, row in enumerate(comb):
            for k in range(3):
                c.limit_vel_comb[i][k] = row[k]
        z = cm.zero_command_curriculum
        c.zero_cmd_curriculum_enabled = int(z is not None)
        if z is not None:
            for k, key in enumerate(("start_iter", "end_iter", "start_value", "end_value")):
                c.zero_cmd_curriculum[k] = z[key]
        for r, key in enumerate(("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")):
            c.cmd_ranges[r][0], c.cmd_ranges[r][1] = self.command_ranges[key]
        cur = sorted(cm.command_range_curriculum, key=lambda x: x["iter"])
        c.cmd_curriculum_count = len(cur)
        for i, ent in enumerate(cur):
            vals = [ent["iter"]] + [v for key in ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading") for v in ent[key]]
            for k in range(9):
                c.cmd_curriculum[i][k] = vals[k]
        for kidx, ent in enumerate(cm.terrain_max_command_ranges):
            for r, key in enumerate(("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")):
                c.terrain_max_cmd_ranges[kidx][r][0], c.terrain_max_cmd_ranges[kidx][r][1] = ent[key]
        rw = cfg.rewards
        names = abi.reward_names
        for i in range(len(names)):
            c.reward_scales[i] = 0.0
        for key, val in self.reward_scales.items():
            k = _REWARD_KEY_ALIASES.get(key, key)
            if val == 0:
                continue                                                                                     # zero scales are dropped (:914-920)
            if k not in names:
                raise ValueError("reward %r has no kernel implementation" % key)
            c.reward_scales[names.index(k)] = val
        self.reward_turn_over_scales = class_to_dict(rw.turn_over_scales) if c.turn_over else {}                   # :1097, :922-930
        for i in range(len(names)):
            c.turn_over_scales[i] = 0.0
        for key, val in self.reward_turn_over_scales.items():
            k = _REWARD_KEY_ALIASES.get(key, key)
            if val != 0:
                if k not in names:
                    raise ValueError("turn-over reward %r has no kernel implementation" % key)
                c.turn_over_scales[names.index(k)] = val
        c.only_positive_rewards, c.tracking_sigma = int(rw.only_positive_rewards), rw.tracking_sigma
        ds = rw.dynamic_sigma
        c.dynamic_sigma_enabled = int(ds is not None)
        if ds is not None:
            for k, key in enumerate(("min_lin_vel", "max_lin_vel", "min_ang_vel", "max_ang_vel")):
                c.dynamic_sigma_vel[k] = ds[key]
            for k in range(9):
                c.dynamic_sigma_max[k] = ds["max_sigma"][k]
        c.soft_dof_pos_limit, c.soft_dof_vel_limit, c.soft_torque_limit = rw.soft_dof_pos_limit, rw.soft_dof_vel_limit, rw.soft_torque_limit
        c.base_height_target, c.max_contact_force, c.min_legs_distance = rw.base_height_target, rw.max_contact_force, rw.min_legs_distance
        cr = list(getattr(rw, "curriculum_rewards", None) or [])
        c.reward_curriculum_count = len(cr)
        for i, ent in enumerate(cr):
            c.reward_curriculum_term[i] = names.index(ent["reward_name"])
            for k, key in enumerate(("start_iter", "end_iter", "start_value", "end_value")):
                c.reward_curriculum[i][k] = ent[key]
        o = cfg.normalization.obs_scales
        c.obs_scale_lin_vel, c.obs_scale_ang_vel, c.obs_scale_dof_pos, c.obs_scale_dof_vel, c.obs_scale_height = o.lin_vel, o.ang_vel, o.dof_pos, o.dof_vel, o.height_measurements
        n = cfg.noise
        c.add_noise, c.noise_level = int(n.add_noise), n.noise_level
        ns = n.noise_scales
        c.noise_dof_pos, c.noise_dof_vel, c.noise_lin_vel, c.noise_ang_vel, c.noise_gravity, c.noise_height = ns.dof_pos, ns.dof_vel, ns.lin_vel, ns.ang_vel, ns.gravity, ns.height_measurements
        c.episode_length_s, c.send_timeouts, c.num_steps_per_env = cfg.env.episode_length_s, int(cfg.env.send_timeouts), 24
        return c

    def create_sim(self):
        """Creates the simulator handle (the reference's create_sim/_create_envs, :292-310,952-1052)."""
        self._c = self._fill_cfg()
        dev_id = 0
        if self.lib.go2sim_is_device_library() == 1:
            dev_id = torch.device(self.device).index or 0
        h = C.c_void_p()
        _abi.check(self.lib, self.lib.go2sim_create(C.byref(self._c), dev_id, C.byref(h)), "go2sim_create")
        self.handle = h
        self.num_dof = self.num_dofs = 12
        self.num_bodies = 19
        self.dof_names = list(_DOF_NAMES)
        self.body_names = list(_BODY_NAMES)

    # ------------------------------------------------------------------ buffers
    def _init_buffers(self):
        dev = self.device
        b = wrap_buffers(self.lib, self.handle, self.num_envs, dev)
        self._buf = b
        # the four Isaac Gym tensors and their views (:779-787)
        self.root_states, self.dof_state = b["root_states"], b["dof_state"]
        self.dof_pos, self.dof_vel = self.dof_state[..., 0], self.dof_state[..., 1]
        self.base_quat, self.base_pos = self.root_states[:, 3:7], self.root_states[:, 0:3]
        self.contact_forces, self.rigid_body_states = b["contact_forces"], b["rigid_body_states"]
        # VecEnv buffers (base_task.py:41-49)
        self.obs_buf, self.privileged_obs_buf, self.rew_buf = b["obs_buf"], b["privileged_obs_buf"], b["rew_buf"]
        if self.num_privileged_obs is None:
            self.privileged_obs_buf = None
        self.reset_buf, self.time_out_buf = b["reset_buf"].view(torch.bool), b["time_out_buf"].view(torch.bool)
        self._episode_length_buf = b["episode_length_buf"]
        for src, dst in (("torques", "torques"), ("actions", "actions"), ("last_actions", "last_actions"), ("last_last_actions", "last_last_actions"),
                         ("last_dof_vel", "last_dof_vel"), ("last_root_vel", "last_root_vel"), ("commands", "commands"),
                         ("commands_resampling_step", "commands_resampling_step"), ("commands_xy_accumulation", "commands_xy_accumulation"),
                         ("base_lin_vel", "base_lin_vel"), ("base_ang_vel", "base_ang_vel"), ("projected_gravity", "projected_gravity"), ("rpy", "rpy"),
                         ("measured_heights", "measured_heights"), ("max_move_distance", "max_move_distance"), ("turn_over_timer", "turn_over_timer"), ("feet_air_time", "feet_air_time"),
                         ("motor_strengths", "motor_strengths"), ("motor_zero_offsets", "motor_zero_offsets"), ("p_gains_multiplier", "p_gains_multiplier"),
                         ("d_gains_multiplier", "d_gains_multiplier"), ("env_origins", "env_origins"), ("terrain_levels", "terrain_levels"),
                         ("terrain_types", "terrain_types"), ("friction_coeffs", "friction_coeffs")):
            setattr(self, dst, b[src])
        self.stop_heading, self.last_is_limit_vel = b["stop_heading"].view(torch.bool), b["last_is_limit_vel"].view(torch.bool)
        self.last_contacts = b["last_contacts"].view(torch.bool)
        names = self.abi.reward_names
        active = [i for i in range(len(names)) if self._c.reward_scales[i] != 0 or (self._c.turn_over and self._c.turn_over_scales[i] != 0)]
        self.reward_names = [names[i] for i in active if names[i] != "termination"]
        self.episode_sums = {names[i]: b["episode_sums"][i] for i in active}
        self.reward_scales = {names[i]: self._c.reward_scales[i] * self.dt for i in active}
        # extras["episode"]: 0-d views of a per-step snapshot ring of the library's episode_info vector
        self._episode_info = b["episode_info"]
        self._info_ring = torch.zeros(32, self._episode_info.shape[0], device=dev)
        self._info_slot = 0
        self._first_reset_done = False
        self._active_idx = active
        self.extras = {}
        f32 = dict(dtype=torch.float, device=dev)
        self.p_gains = torch.tensor([self._c.kp[i] for i in range(12)], **f32)
        self.d_gains = torch.tensor([self._c.kd[i] for i in range(12)], **f32)
        self.default_dof_pos = torch.tensor([self._c.default_dof_pos[i] for i in range(12)], **f32).unsqueeze(0)
        lo = torch.tensor([-1.0472, -1.5708, -2.7227] * 2 + [-1.0472, -0.5236, -2.7227] * 2, **f32)
        hi = torch.tensor([1.0472, 3.4907, -0.83776] * 2 + [1.0472, 4.5379, -0.83776] * 2, **f32)
        m, r = (lo + hi) / 2, hi - lo                                                # soft limits (:372-375)
        self.dof_pos_limits = torch.stack([m - 0.5 * r * self.cfg.rewards.soft_dof_pos_limit, m + 0.5 * r * self.cfg.rewards.soft_dof_pos_limit], dim=1)
        self.torque_limits = torch.tensor([23.7, 23.7, 35.55] * 4, **f32)
        self.dof_vel_limits = torch.tensor([30.1, 30.1, 20.07] * 4, **f32)
        self.feet_indices = torch.tensor([6, 10, 14, 18], dtype=torch.long, device=dev)
        self.penalised_contact_indices = torch.tensor([4, 5, 8, 9, 12, 13, 16, 17], dtype=torch.long, device=dev)
        self.termination_contact_indices = torch.tensor([0], dtype=torch.long, device=dev)
        self.commands_scale = torch.tensor([self.obs_scales.lin_vel, self.obs_scales.lin_vel, self.obs_scales.ang_vel], **f32)
        self.gravity_vec = torch.tensor([0.0, 0.0, -1.0], **f32).repeat(self.num_envs, 1)
        self.custom_origins = self.cfg.terrain.mesh_type in ("heightfield", "trimesh")
        self._level_groups = None
        if self.custom_origins:                                                      # _create_heightfield/_get_env_origins (:964-1079)
            hs, org, ids = self._terrain_host[:3]
            self.height_samples = torch.from_numpy(hs).view(self.terrain.tot_rows, self.terrain.tot_cols).to(dev)
            self.terrain_cols2id = torch.from_numpy(ids).to(dev).long()
            if len(self.terrain.cols2id):                                            # (:1074-1075) no terrain_ids attribute without a curriculum layout
                self.terrain_ids = self.terrain_cols2id[self.terrain_types]
            self.max_terrain_level = self.cfg.terrain.num_rows
            self.terrain_origins = torch.from_numpy(org).to(dev)
            # extras terrain_level_<name> (:230-237): the library keeps the mean level of all envs and of the envs on each terrain KIND as of
            # the latest pass that reset an env (episode_info[NUM_REWARDS + 3 ..]); a name of name2cols is a kind (utils/terrain.py KIND_NAMES)
            from ...utils.terrain import KIND_NAMES
            nr = self.abi.GO2_NUM_REWARDS
            self._level_groups = [("all", nr + 3)] + [(name, nr + 4 + KIND_NAMES.index(name)) for name in self.terrain.name2cols]
        self.add_noise = self.cfg.noise.add_noise

    # ------------------------------------------------------------------ domain_rand.randomize_sensors
    def _init_sensors(self, nn):
        """Per-episode observation latency, dropped frames and constant gyro / gravity / encoder offsets between obs_buf and what step() returns (include/go2nn.h:
        go2nn_sensor_rand_*; csrc/go2nn_sensor_rand.h).  nn: a go2nn library handle in the simulator's memory space (the tests hand in the host build); None loads the HIP one."""
        from ..._nn import GO2_OBS_KINDS, SENSOR_KINDS, Go2nnSensorIn, Go2nnSensorRand, load_nn
        d, D, N = self.cfg.domain_rand, int(self.num_obs), self.num_envs
        if D != len(GO2_OBS_KINDS) or not hasattr(self, "_get_noise_scale_vec"):
            raise ValueError("domain_rand.randomize_sensors: no observation layout for %s with %d observation columns (the Go2 layout of envs/go2/go2_env.py is covered)"
                             % (type(self).__name__, D))
        nn = load_nn() if nn is None else nn
        if nn.go2nn_is_device_library() != self.lib.go2sim_is_device_library():
            raise ValueError("domain_rand.randomize_sensors: the go2nn library and the simulator do not share a memory space")
        lo, hi = d.sensor_delay_range
        if int(lo) != lo or int(hi) != hi:
            raise ValueError("domain_rand.sensor_delay_range = %r: whole policy steps" % (d.sensor_delay_range,))
        r, o = Go2nnSensorRand(), self.cfg.normalization.obs_scales
        r.delay_lo, r.delay_hi, r.drop_lo, r.drop_hi = int(lo), int(hi), float(d.sensor_drop_range[0]), float(d.sensor_drop_range[1])
        r.gyro_bias, r.gravity_bias, r.joint_offset = float(d.sensor_gyro_bias) * float(o.ang_vel), float(d.sensor_gravity_bias), float(d.sensor_joint_offset) * float(o.dof_pos)
        r.env_offset = self._env_offset & 0xFFFFFFFF
        kind = np.asarray([SENSOR_KINDS.index(k) for k in GO2_OBS_KINDS], np.int32)
        if nn.go2nn_sensor_rand_check(C.byref(r), C.c_void_p(kind.ctypes.data), D) != 0:
            raise ValueError("domain_rand.randomize_sensors: %s" % nn.go2nn_last_error().decode())
        dev, t = self.obs_buf.device, self.obs_buf
        sn = self._sensors = {"nn": nn, "rand": r, "kind": torch.from_numpy(kind).to(dev), "pending": False}
        sn["state"] = torch.zeros(int(nn.go2nn_sensor_rand_state_bytes(N, D)), dtype=torch.uint8, device=dev)
        sn["delivered"] = torch.zeros(N, D, device=dev)
        sn["also_fresh"] = torch.zeros(N, dtype=torch.uint8, device=dev)
        a = sn["in"] = Go2nnSensorIn()
        a.obs.p, a.obs.env_stride, a.obs.comp_stride = t.data_ptr(), t.stride(0), t.stride(1)
        a.dones, a.scale, a.kind = self._buf["reset_buf"].data_ptr(), None, sn["kind"].data_ptr()
        a.D, a.num_specs, a.clip, a.seed = D, 0, float(self.cfg.normalization.clip_observations), int(getattr(self.cfg, "seed", 1)) & 0xFFFFFFFF
        print("[go2_rl_gym_amd] randomize_sensors: per episode, observation latency %d .. %d policy steps, dropped frames %g .. %g, offsets gyro %g rad/s, gravity %g, "
              "joint position %g rad (the privileged observation stays exact)" % (r.delay_lo, r.delay_hi, r.drop_lo, r.drop_hi, d.sensor_gyro_bias, d.sensor_gravity_bias,
                                                                                 d.sensor_joint_offset))

    def _sensor_check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, self._sensors["nn"].go2nn_last_error().decode()))

    def _sensor_apply(self, out):
        """obs_buf -> out [N, num_obs] (a storage row or the delivered buffer) on the step's stream; envs reset from outside a step since the last call start a new episode"""
        sn = self._sensors
        fresh = C.c_void_p(sn["also_fresh"].data_ptr()) if sn["pending"] else None
        self._sensor_check(sn["nn"].go2nn_sensor_rand_apply(C.byref(sn["in"]), C.byref(sn["rand"]), fresh, C.c_void_p(sn["state"].data_ptr()), C.c_void_p(out.data_ptr()),
                                                            self.num_envs, self._stream()), "go2nn_sensor_rand_apply")
        if sn["pending"]:
            sn["also_fresh"].zero_()
            sn["pending"] = False
        return out

    def get_observations(self):
        return self.obs_buf if self._sensors is None else self._sensors["delivered"]

    def reset(self):
        """(base_task.py:82-86) with randomize_sensors the sensor state begins here: the frame of the zero-action step is its step 0"""
        if self._sensors is None:
            return super().reset()
        self.reset_idx(torch.arange(self.num_envs, device=self.device))
        sn = self._sensors
        self._sensor_check(sn["nn"].go2nn_sensor_rand_begin(C.c_void_p(sn["state"].data_ptr()), self._stream()), "go2nn_sensor_rand_begin")
        sn["also_fresh"].zero_()          # (step 0 refills every lane anyway)
        sn["pending"] = False
        obs, privileged_obs, _, _, _ = self.step(torch.zeros(self.num_envs, self.num_actions, device=self.device, requires_grad=False))
        return obs, privileged_obs

    # the runner REPLACES this attribute (on_policy_runner.py:118): copy into the library's buffer instead
    @property
    def episode_length_buf(self):
        return self._episode_length_buf

    @episode_length_buf.setter
    def episode_length_buf(self, value):
        self._episode_length_buf.copy_(value)

    @property
    def common_step_counter(self):
        return int(self.lib.go2sim_get_common_step_counter(self.handle))

    @common_step_counter.setter
    def common_step_counter(self, value):                       # train.py:14
        _abi.check(self.lib, self.lib.go2sim_set_common_step_counter(self.handle, int(value)), "set_common_step_counter")

    def update_reward_curriculum(self, force_update: bool = False):   # :144-152
        _abi.check(self.lib, self.lib.go2sim_update_reward_curriculum(self.handle, int(force_update)), "update_reward_curriculum")

    def _curriculum_state(self):
        R = self.abi.real
        rcs = (R * self.abi.GO2_NUM_REWARDS)()
        cr = (R * 8)()
        zp = R()
        self.lib.go2sim_get_curriculum_state(self.handle, rcs, cr, C.byref(zp))
        return list(rcs), [[cr[2 * i], cr[2 * i + 1]] for i in range(4)], zp.value

    @property
    def reward_curriculum_scales(self):
        rcs, _, _ = self._curriculum_state()
        return {c["reward_name"]: rcs[self.abi.reward_names.index(c["reward_name"])] for c in self.reward_curriculum_configs}

    @property
    def zero_command_proba(self):
        return self._curriculum_state()[2]

    # ------------------------------------------------------------------ the hot path
    def step(self, actions, rollout=None):
        """LeggedRobot.step (:60-100): one library call = one fused kernel launch.

        rollout (optional, this build's runners): dict with the destinations of one policy step's bookkeeping (go2sim_step_rollout) —
        `obs_out` / `priv_out`: float32 [N,45] / [N,263] tensors (the next rollout-storage rows) that receive the observations INSTEAD of
        obs_buf / privileged_obs_buf and are what this call returns; `values` [N], `rewards_out` [N], `dones_out` [N] uint8, `gamma`: the
        transition store with the time-out bootstrap (ppo.py:104-114).  extras['transition_stored'] tells the algorithm it is done.
        The bootstrap `+ gamma * V * time_out` is applied only with cfg.env.send_timeouts, i.e. when the reference's infos carry
        'time_outs' (ppo.py:107).  CONTRACT of the redirected form: obs_buf / privileged_obs_buf are NOT written by such a step (the
        rows handed in are), so get_observations() is stale until a plain step() or the last step of the rollout, which has no next row.
        A destination this call cannot write in place (other device, dtype or stride) makes it fall back to the plain step(); the
        caller then sees extras without 'transition_stored' and does its own copies.
        With domain_rand.randomize_sensors the simulator writes obs_buf in either form, and what is returned — the delivered buffer, or the `obs_out` row — is written by
        go2nn_sensor_rand_apply: the frame the robot's sensors would have delivered (_init_sensors)."""
        a = actions
        if a.dtype != torch.float32 or not a.is_contiguous() or str(a.device) != str(self.obs_buf.device):
            a = a.to(device=self.obs_buf.device, dtype=torch.float32).contiguous()
        if rollout is not None:
            for name in ("obs_out", "priv_out", "values", "rewards_out", "dones_out"):
                t = rollout.get(name)
                if t is not None and not (t.is_contiguous() and t.device == self.obs_buf.device and t.dtype == (torch.uint8 if name == "dones_out" else torch.float32)):
                    rollout = None
                    break
        if rollout is None:
            _abi.check(self.lib, self.lib.go2sim_step(self.handle, C.c_void_p(a.data_ptr()), self._stream()), "go2sim_step")
            self._publish_extras()
            self.extras.pop("transition_stored", None)
            obs = self.obs_buf if self._sensors is None else self._sensor_apply(self._sensors["delivered"])
            return obs, self.privileged_obs_buf, self.rew_buf, self.reset_buf, self.extras
        o = self.abi.StepOutputs()
        fp, bp = C.POINTER(self.abi.real), C.POINTER(C.c_uint8)
        keep = []
        for name, ctype in (("obs_out", fp), ("priv_out", fp), ("values", fp), ("rewards_out", fp), ("dones_out", bp)):
            t = rollout.get(name)
            if name == "values" and not self.cfg.env.send_timeouts:
                t = None                                        # no 'time_outs' in infos -> no bootstrap (ppo.py:107-108)
            if name == "obs_out" and self._sensors is not None:
                t = None                                        # the simulator writes obs_buf; the sensor kernel below writes the storage row in the copy's place
            if t is not None:
                keep.append(t)
                setattr(o, name, C.cast(C.c_void_p(t.data_ptr()), ctype))
        o.gamma = float(rollout.get("gamma", 0.0))
        slot = self._info_ring[self._info_slot]
        o.episode_info_out = C.cast(C.c_void_p(slot.data_ptr()), fp)
        self._rollout_keep = keep                               # alive until the enqueued kernels have run
        _abi.check(self.lib, self.lib.go2sim_step_rollout(self.handle, C.c_void_p(a.data_ptr()), C.byref(o), self._stream()), "go2sim_step_rollout")
        self._publish_extras(copied=True)
        self.extras["transition_stored"] = rollout.get("rewards_out") is not None and rollout.get("dones_out") is not None
        obs = rollout["obs_out"] if rollout.get("obs_out") is not None else self.obs_buf
        if self._sensors is not None:
            obs = self._sensor_apply(rollout["obs_out"] if rollout.get("obs_out") is not None else self._sensors["delivered"])
        priv = rollout["priv_out"] if rollout.get("priv_out") is not None else self.privileged_obs_buf
        return obs, priv, self.rew_buf, self.reset_buf, self.extras

    def reset_idx(self, env_ids):
        """legged_robot.py:180-245 from OUTSIDE a step (base_task.py:82-84 resets everything before the first step; a caller may reset any
        subset later).  The per-env resets of a step happen inside the step kernel, exactly where post_physics_step does them (:132-133)."""
        if len(env_ids) == 0:
            return
        if not self._first_reset_done:
            if len(env_ids) != self.num_envs:
                raise ValueError("the first reset_idx must cover every environment (base_task.py:82-84): the buffers are undefined before it")
            self._first_reset_done = True
            _abi.check(self.lib, self.lib.go2sim_reset_all(self.handle, self._stream()), "go2sim_reset_all")
        else:
            ids = torch.as_tensor(env_ids, device=self.device).to(torch.int32).contiguous()
            self._reset_ids = ids                               # keep the id tensor alive until the enqueued kernels have run
            ptr = C.c_void_p(ids.data_ptr())
            _abi.check(self.lib, self.lib.go2sim_reset_idx(self.handle, ptr, int(ids.numel()), self._stream()), "go2sim_reset_idx")
            if self._sensors is not None:                       # a new episode for these robots at the next sensor step
                self._sensors["also_fresh"][ids.long()] = 1
                self._sensors["pending"] = True
        self._publish_extras()

    def _publish_extras(self, copied=False):
        """extras['episode'] / extras['time_outs'] (:229-245) without a host sync: the kernel keeps the means of the
        latest step that reset >= 1 env; each step snapshots them into a ring slot so earlier dicts stay intact."""
        slot = self._info_ring[self._info_slot]
        if not copied:                   # (go2sim_step_rollout writes the ring slot itself)
            slot.copy_(self._episode_info)
        self._info_slot = (self._info_slot + 1) % self._info_ring.shape[0]
        names = self.abi.reward_names
        if self._level_groups is None:
            ep = {"terrain_level_all": 0.0}
        else:
            ep = {"terrain_level_" + n: slot[k] for n, k in self._level_groups}
        for i in self._active_idx:
            ep["rew_" + names[i]] = slot[i]
        if self.cfg.commands.curriculum:
            ep["max_command_x"] = slot[len(names) + 2]          # command_ranges['lin_vel_x'][1] as update_command_curriculum keeps it (:241-242)
        self.extras["episode"] = ep
        if self.cfg.env.send_timeouts:
            self.extras["time_outs"] = self.time_out_buf

    def post_physics_step(self):
        """For harnesses that drive the four simulator tensors themselves (the golden-vector tests)."""
        _abi.check(self.lib, self.lib.go2sim_post_physics(self.handle, self._stream()), "go2sim_post_physics")
        self._publish_extras()

    def get_current_scale(self, config):                        # :154-168
        it = self.common_step_counter // self.num_steps_per_env
        pct = (it - config["start_iter"]) / (config["end_iter"] - config["start_iter"])
        pct = max(min(pct, 1.0), 0.0)
        return (1.0 - pct) * config["start_value"] + pct * config["end_value"]
