"""Left-right mirror tables of the Go2 tasks' observation and action vectors (`algorithm.symmetry`, rsl_rl/algorithms/ppo.py).

The mirror image of a row x is x[perm] * sign.  The tables are built from the declared block layout below — the layout of envs/go2/go2_env.py (reference go2_env.py:26-47)
as csrc/go2_post.h writes it — never typed in column by column, and any other observation size raises: there are no guessed tables.

Block kinds (reflection in the robot's x-z plane):
  polar     a vector (linear velocity, gravity direction)               (x, -y, z)
  axial     a pseudo-vector (angular velocity)                          (-x, y, -z)
  command   (vx, vy, yaw rate)                                          (vx, -vy, -yaw)
  joint     FL FR RL RR x (hip, thigh, calf)                            FL <-> FR, RL <-> RR; the hip (abduction) changes sign, thigh and calf do not
  foot      FL FR RL RR                                                 FL <-> FR, RL <-> RR
  heights   the grid measured_points_x x measured_points_y, column ix * ny + iy      (x, y) <-> (x, -y)
The action std goes with the joints but is a magnitude: permuted, never negated.

What this is not: the simulator is not exactly mirror-symmetric (the trunk's inertia in include/go2_model_data.h has ixy, iyz != 0: a mirrored state steps to the mirror
image within ~2e-3, tests/test_symmetry_host.py), and nothing here makes a policy equivariant — PPO is only trained on both images."""
from collections import namedtuple

import numpy as np

LEGS = ("FL", "FR", "RL", "RR")
LEG_MIRROR = {"FL": "FR", "FR": "FL", "RL": "RR", "RR": "RL"}
JOINTS = (("hip", -1.0), ("thigh", 1.0), ("calf", 1.0))          # (name, sign under the reflection), in the order of the joints within a leg

# (block name, kind) in column order
ACTOR_BLOCKS = (("ang_vel", "axial"), ("gravity", "polar"), ("commands", "command"), ("dof_pos", "joint"), ("dof_vel", "joint"), ("actions", "joint"))
PRIVILEGED_BLOCKS = (("lin_vel", "polar"),) + ACTOR_BLOCKS + (("foot_force", "foot"), ("torques", "joint"), ("dof_acc", "joint"), ("heights", "heights"))
ACTION_BLOCKS = (("actions", "joint"),)

_FIXED = {"polar": ((0, 1, 2), (1.0, -1.0, 1.0)), "axial": ((0, 1, 2), (-1.0, 1.0, -1.0)), "command": ((0, 1, 2), (1.0, -1.0, -1.0))}

MirrorTables = namedtuple("MirrorTables", ("obs", "privileged_obs", "action", "action_std"))          # each a (perm int16 [W], sign float32 [W]) pair


def _leg_block(per_leg):
    """per_leg: the signs of one leg's entries -> (perm, sign) of the block [4 legs x len(per_leg)]"""
    n = len(per_leg)
    perm = [LEGS.index(LEG_MIRROR[leg]) * n + j for leg in LEGS for j in range(n)]
    return perm, [s for _ in LEGS for s in per_leg]


def height_permutation(xs, ys):
    """-> perm of the height grid's columns (column ix * ny + iy is the sample at (xs[ix], ys[iy])): the column of (x, -y).  Raises when ys is not symmetric about 0."""
    ys = [float(y) for y in ys]
    ny = len(ys)
    back = []
    for y in ys:
        hit = [k for k, other in enumerate(ys) if abs(other + y) < 1e-6]
        if len(hit) != 1:
            raise ValueError("terrain.measured_points_y is not symmetric about 0 (no unique sample at y = %g): %s" % (-y, ys))
        back.append(hit[0])
    return [ix * ny + back[iy] for ix in range(len(xs)) for iy in range(ny)]


def block_table(kind, terrain_cfg=None):
    """-> (perm, sign) of one block, columns counted from the block's start"""
    if kind in _FIXED:
        return list(_FIXED[kind][0]), list(_FIXED[kind][1])
    if kind == "joint":
        return _leg_block([s for _, s in JOINTS])
    if kind == "foot":
        return _leg_block([1.0])
    if kind == "heights":
        perm = height_permutation(terrain_cfg.measured_points_x, terrain_cfg.measured_points_y)
        return perm, [1.0] * len(perm)
    raise ValueError("unknown block kind %r" % (kind,))


def layout_table(blocks, terrain_cfg=None, signed=True):
    """The (perm int16, sign float32) of a row made of `blocks` (name, kind) in order.  signed False: the permutation alone (sign +1 everywhere)."""
    perm, sign = [], []
    for _, kind in blocks:
        p, s = block_table(kind, terrain_cfg)
        base = len(sign)
        perm += [base + k for k in p]
        sign += s if signed else [1.0] * len(s)
    return np.asarray(perm, np.int16), np.asarray(sign, np.float32)


def mirror_tables(env_cfg):
    """-> MirrorTables for the task's actor observation, privileged observation, action mean and action std.  ValueError for any layout but the Go2 tasks'
    45 / 263 columns with 12 actions (envs/go2/go2_config.py)."""
    env, terrain = env_cfg.env, env_cfg.terrain
    n_obs, n_priv, n_act = env.num_observations, env.num_privileged_obs, env.num_actions
    obs, act = layout_table(ACTOR_BLOCKS), layout_table(ACTION_BLOCKS)
    if n_obs != len(obs[0]):
        raise ValueError("no mirror table for an actor observation of %s columns: the declared layout (%s) has %d" % (n_obs, ", ".join(n for n, _ in ACTOR_BLOCKS), len(obs[0])))
    if n_act != len(act[0]):
        raise ValueError("no mirror table for %s actions: the declared layout (FL FR RL RR x hip, thigh, calf) has %d" % (n_act, len(act[0])))
    if n_priv is None:
        raise ValueError("no mirror table for a task without a privileged observation: the declared critic layout is (%s)" % ", ".join(n for n, _ in PRIVILEGED_BLOCKS))
    priv = layout_table(PRIVILEGED_BLOCKS, terrain)
    if n_priv != len(priv[0]):
        raise ValueError("no mirror table for a privileged observation of %s columns: the declared layout (%s) with the %d x %d height grid has %d"
                         % (n_priv, ", ".join(n for n, _ in PRIVILEGED_BLOCKS), len(terrain.measured_points_x), len(terrain.measured_points_y), len(priv[0])))
    return MirrorTables(obs, priv, act, layout_table(ACTION_BLOCKS, signed=False))


def history_table(obs_table, H):
    """The table of a row of H observation frames side by side [H * W] (the CTS student's history): the actor table tiled H times, frame h's columns staying in frame h."""
    perm, sign = np.asarray(obs_table[0], np.int64), np.asarray(obs_table[1], np.float32)
    W, H = len(perm), int(H)
    if H < 1 or H * W > 32767:
        raise ValueError("history_table: %r frames of %d columns (1 <= H, H * W <= 32767)" % (H, W))
    return (np.concatenate([perm + h * W for h in range(H)]).astype(np.int16), np.tile(sign, H))


def joint_sides():
    """-> int32 [12]: +1 for a joint of a left leg, -1 of a right leg, in the joint block's order (LEGS x JOINTS)"""
    return np.asarray([leg_side(leg) for leg in LEGS for _ in JOINTS], np.int32)


def joint_kinds():
    """-> int32 [12]: the joint's index in JOINTS (0 hip, 1 thigh, 2 calf), in the joint block's order"""
    return np.asarray([k for _ in LEGS for k in range(len(JOINTS))], np.int32)


def leg_side(name):
    """+1 / -1 for a name that starts with a left / right leg of LEGS ("FL", "RL_foot", ...): the side is the leg name's second letter, as LEG_MIRROR swaps it"""
    leg = str(name).upper()[:2]
    if leg not in LEGS or leg[1] not in "LR" or LEG_MIRROR[leg][1] == leg[1]:
        raise ValueError("%r does not start with one of the legs %s" % (name, ", ".join(LEGS)))
    return 1 if leg[1] == "L" else -1


def mirror_rows(x, table):
    """numpy: the mirror image of the rows of x [..., W]"""
    perm, sign = table
    return x[..., perm.astype(np.int64)] * sign
