"""The bootstrap of the modes' and add-ons' figures on a real MI355X: the device build of go2nn_{robust,maneuver,ladder,gait,asym}_bootstrap against the integer draws and
the fp64 sums of tests/test_bootstrap_modes_host.py over the DEVICE's own per-robot terms — the same cases, bit for bit —, the refusals, and evaluations with
`evaluation.bootstrap_all` on.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_bootstrap_host as tb  # noqa: E402
import test_bootstrap_modes_host as tm  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402

DEV = "cuda:0"
SMALL = dict(enabled=True, interval=1, num_envs=64, seconds=1.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None)


class DeviceBackend:
    """how the checks of test_bootstrap_modes_host reach the device library: torch tensors on the GPU"""
    name = "device"

    def __init__(self, lib):
        self.lib = lib

    up = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV))
    ptr = staticmethod(lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    down = staticmethod(lambda t: t.cpu().numpy())
    stream = staticmethod(lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream))
    full = staticmethod(lambda shape, v: torch.full(shape, v, dtype=torch.float64, device=DEV))


@pytest.fixture(scope="module")
def dev():
    load_hip()
    from go2_rl_gym_amd._nn import load_nn
    return DeviceBackend(load_nn())


@pytest.mark.parametrize("B", tb.BS)
@pytest.mark.parametrize("N", sorted(tb.CASES))
@pytest.mark.parametrize("fam", tm.FAMS)
def test_kernel_equals_the_restatement_bit_for_bit(dev, fam, N, B):
    tm.check_kernel_case(dev, tm.FAMILIES[fam], N, B)


@pytest.mark.parametrize("fam", tm.FAMS)
def test_same_robots_prefix_seed_and_constant_cell(dev, fam):
    tm.check_same_robots(dev, tm.FAMILIES[fam])
    tm.check_prefix_and_seed(dev, tm.FAMILIES[fam])
    tm.check_constant_cell(dev, tm.FAMILIES[fam])


@pytest.mark.parametrize("fam", tm.FAMS)
def test_refusals(dev, fam):
    tm.check_refusals(dev, tm.FAMILIES[fam], sync=torch.cuda.synchronize)


def _evaluator(**over):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    env_cfg, train_cfg = task_registry.get_cfgs("go2_flat")
    ev = dict(class_to_dict(train_cfg.evaluation), **dict(SMALL, **over))
    return PolicyEvaluator(env_cfg, ev, task_class=task_registry.get_task_class("go2_flat"), device=DEV)


def check_tables_against_the_devices_own_terms(dev, ev, res):
    """every family's bootstrap table is the restatement — the integer draws over the evaluator's cells, one fp64 add per draw — of the device's own per-robot terms: its
    reduce with singleton groups on the evaluator's table"""
    B = ev.bootstrap
    per_cell = tm.drawn(ev.cell_start_host.copy(), ev.cell_envs_host.copy(), B, ev.bootstrap_seed)
    assert list(res["bootstrap"]["tables"]) == [t.name for t in ev.tables]
    for t in ev.tables:
        fam = tm.FAMILIES[t.name]
        fam = tm.Family(fam.name, fam.rows, fam.cols, fam.n_col, fam.whole, fam.max_col, tuple(C.c_float(x) for x in t.reduce_args))
        want = tm.restate(tm.own_terms(dev, fam, t.table.cpu().numpy()), per_cell, fam.max_col)
        got = res["bootstrap"]["tables"][t.name]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (t.name, np.nanmax(np.abs(got - want)))
        assert (got[:, :, fam.n_col] == np.diff(ev.cell_start_host)[None]).all()


@pytest.mark.parametrize("mode", ["robust", "maneuvers"])
def test_evaluation_with_every_family_resampled(dev, monkeypatch, mode):
    """go2_flat, 64 robots, bootstrap = 257 (two workgroups along the replicates, the second with one lane), eager: the tables against the device's own terms, the
    replicate figures against the row functions, and a replayed evaluation with the same bytes — the launches sit after the replayed chunks"""
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    over = dict(perturbations=tm.PERTURBATIONS, gait=True, asymmetry=True) if mode == "robust" else dict(maneuvers=[["brake", [[0.0, 1.0, 0.0, 0.0], [0.4, 0.0, 0.0, 0.0]]],
                                                                                                                       ["turn", [[0.0, 0.0, 0.0, 1.0], [0.5, 0.0, 0.0, -1.0]]]],
                                                                                                            maneuver_window_s=0.3, maneuver_hold_s=0.1)
    ac = tb.small_actor_critic().to(DEV)
    ev_ci, ev = _evaluator(bootstrap=257, **over), _evaluator(bootstrap=257, bootstrap_all=True, **over)
    ci, on = ev_ci.evaluate(ac, use_graph=False), ev.evaluate(ac, use_graph=False)
    assert (ci["mode"], on["mode"]) == ("eager", "eager") and ev.num_envs == 64 and not hasattr(ev_ci, "boot_outs")
    assert tb.same_value(tm.strip(on), tm.strip(ci)) and "tables" not in ci["bootstrap"]
    check_tables_against_the_devices_own_terms(dev, ev, on)
    monkeypatch.setattr(tm, "B", 257)
    monkeypatch.setattr(tm, "CONF", ev.confidence)
    tm.check_leaves(ev, on, mode)
    for name, c in tm.all_ci(on):
        for k, (lo, hi) in c.items():
            assert lo <= hi or (np.isnan(lo) and np.isnan(hi)), (name, k)
    replay = ev.evaluate(ac, use_graph=True)
    assert replay["mode"] == "graph" and tb.same_value(replay["bootstrap"], on["bootstrap"]) and str(tm.all_ci(replay)) == str(tm.all_ci(on))
    ev_ci.close(); ev.close()


def test_ladder_evaluation_with_the_ladder_resampled(dev, monkeypatch):
    """the terrain task at the size tests/test_gpu_ladder.py uses (256 robots, 2 s): the ladder's table against the device's own terms, the summary's replicates by the
    loop rule"""
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    args = get_args(["--task", "go2", "--num_envs", "64", "--headless"])
    env, _ = task_registry.make_env("go2", args)
    runner, _ = task_registry.make_alg_runner(env, "go2", args, log_root=None)
    cfg = dict(enabled=True, interval=1, num_envs=256, seconds=2.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None, ladder=True, ladder_distance=0.1, bootstrap=257,
               bootstrap_all=True)
    ev = PolicyEvaluator(env.cfg, cfg, task_class=type(env), sim_params=env.sim_params, device=env.sim_device)
    on = ev.evaluate(runner.alg.actor_critic, use_graph=False)
    check_tables_against_the_devices_own_terms(dev, ev, on)
    monkeypatch.setattr(tm, "B", 257)
    monkeypatch.setattr(tm, "CONF", ev.confidence)
    tm.check_ladder_summary(ev, on)
    assert set(on["overall"]["ci"]) == set(tb.leaves(on)[1][1]["ci"]) | {"cleared", "mean_level_cleared"}
    ev.close(); env.close()
