"""Read a trace file (scripts/play.py --record, evaluation.record) and print the per-foot duty factors:  python tools/trace_example.py logs/.../trace_500.npz"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from go2_rl_gym_amd.utils.recorder import read_trace  # noqa: E402

trace = read_trace(sys.argv[1])
print("%d steps of %d robots, dt %.3f s; qpos for MuJoCo: %s" % (trace["frames"].shape[0], trace["frames"].shape[1], trace["dt"], trace["qpos"].shape))
for k, env_id in enumerate(trace["env_ids"]):
    print("env %d: " % env_id + "  ".join("%s %.2f" % (foot, duty) for foot, duty in zip(trace["foot_names"], trace["gait"]["duty_factor"][k])))
