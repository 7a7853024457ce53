"""Read a trace file (scripts/play.py --record, evaluation.record) and print the per-foot duty factors, or a falls file (evaluation.blackbox) and print one line per kept
fall:  python tools/trace_example.py logs/.../trace_500.npz   |   python tools/trace_example.py logs/.../falls_500.npz"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from go2_rl_gym_amd.utils.recorder import fall_summary, format_falls, read_falls, read_trace  # noqa: E402

if os.path.basename(sys.argv[1]).startswith("falls"):
    falls = read_falls(sys.argv[1])
    print("%d robots fell, %d kept (%d per cell), rings of %d steps, dt %.3f s" % (falls["fell_total"], len(falls["env_ids"]), falls.get("kept_per_cell", -1),
                                                                                 falls["frames"].shape[1], falls["dt"]))
    print("\n".join(format_falls(falls, fall_summary(falls))))
    sys.exit(0)
trace = read_trace(sys.argv[1])
print("%d steps of %d robots, dt %.3f s; qpos for MuJoCo: %s" % (trace["frames"].shape[0], trace["frames"].shape[1], trace["dt"], trace["qpos"].shape))
for k, env_id in enumerate(trace["env_ids"]):
    print("env %d: " % env_id + "  ".join("%s %.2f" % (foot, duty) for foot, duty in zip(trace["foot_names"], trace["gait"]["duty_factor"][k])))
