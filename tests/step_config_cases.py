"""What tests/test_step_configs_host.py (host build of the lanes) and tests/test_gpu_step_configs.py (device) share: the step kernel against the oracle at physics
settings OTHER than go2sim_default_cfg, and on the rows the default settings hardly ever reach (joint stops, the twist clamp).

run_case follows tests/test_gpu_parity.py::test_one_step_parity_vs_oracle: every step starts from the fp32 oracle's state (helpers.STEP_STATE copied into the library
under test and into the fp64 oracle), all three step, and the library's distance to the fp32 oracle is held against the fp32 oracle's own distance to the fp64 oracle on
the same inputs (helpers.check_relative_to_conditioning, factor 3, the floors of the rough-terrain test) and against helpers.ROUGH_BOUND on the well-conditioned
env-steps (helpers.check_rough_errors).  helpers.PLANE_BOUND is NOT applied: it was measured at the default settings, and the host build of the lanes itself exceeds
it at a tilted gravity and with the joints driven into their stops.  What makes a case mean something — that the oracle's trajectory really is at the stops, at the
clamp, in contact — is asserted from the fp32 oracle's buffers alone (REACH).

torque_case: the delay select and the torque law at a decimation other than 4, through go2sim_debug_torque_trace."""
import functools

import numpy as np

from helpers import (JOINT_HI, JOINT_LO, ROUGH_BOUND, STEP_STATE, DeviceSim, HostSim, StepErrors, check_relative_to_conditioning, check_rough_errors,
                     heightfield_overrides, load_oracle)
import test_oracle_golden as tg

FEET = tg.FEET
NON_FEET = [b for b in range(19) if b not in FEET]
FLOORS = {"root_states": 2e-5, "dof_state": 2e-4, "torques": 2e-4, "obs_buf": 2e-5, "privileged_obs_buf": 2e-5, "rew_buf": 2e-7}      # test_heightfield_one_step_parity_vs_oracle's
N_PLANE, N_TRIMESH, STEPS, SEED = 70, 80, 60, 0          # 70: four full 16-env workgroups and a tail of 6
NO_RANDOMISATION = dict(randomize_friction=0, randomize_restitution=0, randomize_base_mass=0, randomize_link_mass=0, randomize_base_com=0, randomize_pd_gains=0,
                        randomize_motor_zero_offset=0, randomize_motor_strength=0, randomize_action_delay=0, push_robots=0, add_noise=0)

# name -> (Go2SimCfg overrides, action sigma, trimesh); the defaults these move: decimation 4, sim_dt 0.005, solver_iterations 8, joint_armature 0, gravity (0, 0, -9.81),
# terrain_friction 1, terrain_restitution 0, contact_offset 0.01, max_depenetration_velocity 1, bounce_threshold_velocity 0.5, max_linear / angular_velocity 1000,
# action_scale 0.25, joint_limit_margin 0.05, every randomisation on
CASES = {
    "dec1": (dict(decimation=1), 1.0, False),
    "dec2_dt": (dict(decimation=2, sim_dt=0.01), 1.0, False),
    "dec6": (dict(decimation=6), 1.0, False),
    "solver1": (dict(solver_iterations=1), 1.0, False),
    "solver16": (dict(solver_iterations=16), 1.0, False),
    "armature": (dict(joint_armature=0.01), 1.0, False),
    "gravity_tilt": (dict(gravity=[1.5, -1.0, -9.0]), 1.0, False),
    "contact_params": (dict(terrain_friction=0.2, terrain_restitution=0.5, erp=0.2, contact_cfm=1e-2, contact_offset=0.02, max_depenetration_velocity=3.0,
                            bounce_threshold_velocity=0.1), 1.0, False),
    "velclamp": (dict(max_linear_velocity=0.5, max_angular_velocity=1.0), 1.0, False),
    "stops": (dict(action_scale=1.0, joint_limit_margin=0.1), 1.5, False),
    "stops_default_margin": (dict(action_scale=1.0), 1.5, False),
    "norand": (NO_RANDOMISATION, 1.0, False),
    "trimesh_dec2_solver4": (dict(decimation=2, sim_dt=0.01, solver_iterations=4, contact_offset=0.02), 0.6, True),
    "trimesh_dec6_armature": (dict(decimation=6, joint_armature=0.01, terrain_friction=0.4), 0.6, True),
}

# name -> {reach statistic: the least share of env-steps}; the counts (foot contacts, height scan) are in check_reach
REACH = {
    "stops": {"near_stop": 0.30, "body_contact": 0.05},
    "stops_default_margin": {"near_stop": 0.30, "body_contact": 0.05},
    "velclamp": {"lin_clamped": 0.05, "ang_clamped": 0.30},
}


@functools.lru_cache(maxsize=None)
def _trimesh():
    return heightfield_overrides(N_TRIMESH, mesh_type="trimesh")[1]


def _make(lib, device, **kw):
    return HostSim(lib, **kw) if device is None else DeviceSim(lib, device=device, **kw)


def _quantiles(e, k):
    v = e.all(k)
    return {"p50": float(np.quantile(v, 0.5)), "p99": float(np.quantile(v, 0.99)), "max": float(v.max())}


def run_case(lib, Sim, device, name, record=None):
    """One case of CASES on `lib` (Sim = HostSim with device None, DeviceSim with a device).  Asserts reset_buf (on the trimesh terrain_levels and the height scan too)
    per step, then the two gates and the reach conditions.  -> the statistics, JSON-ready: per tensor p50 / p99 / max of err (library vs fp32 oracle) and cond (fp32 vs
    fp64 oracle), the counts check_rough_errors prints, the reach counts.  `record(stats)` is called BEFORE the gates, so a failing case leaves its figures behind."""
    ov, sigma, trimesh = CASES[name]
    N = N_TRIMESH if trimesh else N_PLANE
    ov = dict(_trimesh(), **ov) if trimesh else dict(ov)
    assert (Sim is HostSim) == (device is None)
    so, s64, su = HostSim(load_oracle(), num_envs=N, **ov), HostSim(load_oracle(f64=True), num_envs=N, **ov), _make(lib, device, num_envs=N, **ov)
    np.testing.assert_array_equal(so.peek(), su.peek())
    so.reset_all(); su.reset_all(); s64.reset_all()
    rng = np.random.default_rng(SEED)
    margin, vmax, wmax = float(so.cfg.joint_limit_margin), float(so.cfg.max_linear_velocity), float(so.cfg.max_angular_velocity)
    reach = dict(env_steps=0, foot_contacts=0, near_stop=0, body_contact=0, lin_clamped=0, ang_clamped=0, max_abs_height=0.0)
    err, cond, abs_err = StepErrors(FLOORS), StepErrors(FLOORS), StepErrors(ROUGH_BOUND, bounds=ROUGH_BOUND)
    for it in range(STEPS):
        a = rng.normal(0, sigma, (N, 12)).astype(np.float32)
        for k in STEP_STATE:
            v = np.asarray(getattr(so, k))
            getattr(su, k)[...] = v; getattr(s64, k)[...] = v
        q = np.asarray(so.dof_state, np.float64)[:, :, 0]          # the pose the step STARTS from
        reach["near_stop"] += int((np.minimum(q - JOINT_LO, JOINT_HI - q) < margin).any(1).sum())
        so.step(a); su.step(a); s64.step(a.astype(np.float64))
        f, r = np.asarray(so.contact_forces, np.float64), np.asarray(so.root_states, np.float64)
        reach["env_steps"] += N
        reach["foot_contacts"] += int((f[:, FEET, 2] > 1).sum())
        reach["body_contact"] += int((np.linalg.norm(f[:, NON_FEET], axis=-1) > 1).any(1).sum())
        reach["lin_clamped"] += int((np.linalg.norm(r[:, 7:10], axis=1) >= 0.999 * vmax).sum())
        reach["ang_clamped"] += int((np.linalg.norm(r[:, 10:13], axis=1) >= 0.999 * wmax).sum())
        err.add(so, su, N); cond.add(so, s64, N); abs_err.add(so, su, N, ref64=s64)
        np.testing.assert_array_equal(np.asarray(so.reset_buf), np.asarray(su.reset_buf), err_msg="%s: reset_buf at step %d" % (name, it))
        if trimesh:
            np.testing.assert_array_equal(np.asarray(so.terrain_levels), np.asarray(su.terrain_levels), err_msg="%s: terrain_levels at step %d" % (name, it))
            assert (np.abs(np.asarray(so.measured_heights) - np.asarray(su.measured_heights)) > 1e-6).sum() <= 6, (name, it)      # (see test_heightfield_one_step_parity_vs_oracle)
            reach["max_abs_height"] = max(reach["max_abs_height"], float(np.abs(np.asarray(so.measured_heights)).max()))
    stats = {"case": name, "envs": N, "steps": STEPS, "sigma": sigma, "err": {k: _quantiles(err, k) for k in FLOORS}, "cond": {k: _quantiles(cond, k) for k in FLOORS},
             "err_well_conditioned": {k: _quantiles(abs_err, k) for k in ROUGH_BOUND}, "outside_rough_bound": {k: int((abs_err.all(k) > b).sum()) for k, b in ROUGH_BOUND.items()}, "ill_conditioned_tensor_rows": int(getattr(abs_err, "ill", 0)),
             "reward_threshold_env_steps": int(getattr(abs_err, "edge", 0)), "reach": reach}
    print("[step config %s] %d envs x %d steps, sigma %.1f; reach %r" % (name, N, STEPS, sigma, reach))
    for k in FLOORS:
        e, c = stats["err"][k], stats["cond"][k]
        print("   %-20s err p50 %.2e p99 %.2e max %.2e | oracle fp32 vs fp64 p50 %.2e p99 %.2e max %.2e" % (k, e["p50"], e["p99"], e["max"], c["p50"], c["p99"], c["max"]))
    so.close(); s64.close(); su.close()
    if record is not None:
        record(stats)
    check_reach(name, reach, trimesh)
    check_relative_to_conditioning(err, cond, FLOORS, factor=3.0)
    check_rough_errors(abs_err)
    return stats


def check_reach(name, reach, trimesh):
    """the oracle's own trajectory went where the case is about"""
    n = reach["env_steps"]
    for k, share in REACH.get(name, {}).items():
        assert reach[k] >= share * n, (name, k, reach[k], n, share)
    if trimesh:
        assert reach["foot_contacts"] > 2000 and reach["max_abs_height"] > 0.05, (name, reach)
    else:
        assert reach["foot_contacts"] > 1000, (name, reach)


# ---- the torque law and the delay select at other decimations -----------------------------------------------------------------------------------------------------
TORQUE_DECIMATIONS, TORQUE_CONTROL_TYPES, TORQUE_N, TORQUE_CALLS = (1, 2, 6), (0, 1, 2), 37, 6


def switch_positions(tq):
    """tq [D, N, 12], every substep fed the SAME joint state: the substep at which an env's torques change is where its delay select went from the last actions to the
    new ones -> the set of such positions (1 .. D - 1; an env that starts on the new actions or never leaves the old ones has none)"""
    changed = (tq[1:] != tq[:-1]).any(2)          # [D - 1, N]
    assert (changed.sum(0) <= 1).all(), "more than one switch in a call"
    return set((np.nonzero(changed)[0] + 1).tolist())


def torque_case(lib, Sim, device, decimation, control_type):
    """go2sim_debug_torque_trace of `lib` against the fp32 oracle's at `decimation` substeps and `control_type`: TORQUE_CALLS calls with one ordinary step between them (so
    last_actions differs from the new actions), every substep of a call fed the oracle's current joint state.  -> the switch positions the ORACLE's output shows"""
    kw = dict(num_envs=TORQUE_N, decimation=decimation, control_type=control_type)
    so, su = HostSim(load_oracle(), **kw), _make(lib, device, **kw)
    assert so.cfg.randomize_action_delay == 1
    so.reset_all(); su.reset_all()
    rng = np.random.default_rng(SEED)
    seen, worst = set(), 0.0
    for call in range(TORQUE_CALLS + 1):
        a = rng.normal(0, 1, (TORQUE_N, 12)).astype(np.float32)
        for k in STEP_STATE:
            getattr(su, k)[...] = np.asarray(getattr(so, k))
        if call:
            assert np.abs(np.asarray(so.last_actions) - a).max() > 0.1
            dof = np.repeat(np.asarray(so.dof_state, np.float32)[None], decimation, 0)
            want, got = tg.torque_trace(so, so.lib, a, dof), tg.torque_trace(su, lib, a, dof)
            assert want.shape == (decimation, TORQUE_N, 12) and np.abs(want).max() > 0.1
            seen |= switch_positions(want)
            worst = max(worst, float(np.abs(got - want).max()))
            np.testing.assert_allclose(got, want, atol=tg.TOL["torques"], rtol=1e-5, err_msg="decimation %d, control type %d, call %d" % (decimation, control_type, call))
            np.testing.assert_allclose(np.asarray(su.torques), want[-1], atol=tg.TOL["torques"], rtol=1e-5)          # the hook leaves the last substep's torques behind
        so.step(a); su.step(a)
    print("[torque trace] decimation %d, control type %d: %d calls x %d envs, largest |difference| %.2e, switch positions seen in the oracle's output %s"
          % (decimation, control_type, TORQUE_CALLS, TORQUE_N, worst, sorted(seen)))
    so.close(); su.close()
    if decimation == 6:
        assert seen >= {1, 2, 3, 4, 5}, seen
    return seen
