"""The evaluator's bootstrap on a real MI355X: the device build of go2nn_eval_bootstrap against the integer / float64 restatement of tests/test_bootstrap_host.py — the same
cases, bit for bit —, its refusals, and one go2_flat evaluation with `evaluation.bootstrap` on, eager and with the steps replayed from a captured graph.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_bootstrap_host as tb  # noqa: E402
from go2_rl_gym_amd.envs import task_registry  # noqa: E402

DEV = "cuda:0"
SMALL = dict(enabled=True, interval=1, num_envs=64, seconds=1.0, warmup_s=0.5, terrain_level=3, seed=77, scenarios=None)


@pytest.fixture(scope="module")
def nn():
    load_hip()
    from go2_rl_gym_amd._nn import load_nn
    return load_nn()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def device_call(nn):
    def call(acc, start, envs, B, seed):
        a, s, e = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (acc, start, envs))
        assert nn.go2nn_eval_bootstrap_check(tb.p(start), tb.p(envs), acc.shape[1], len(start) - 1) == 0, nn.go2nn_last_error()
        out = torch.full((B, len(start) - 1, tb.COLS), -7.0, dtype=torch.float64, device=DEV)
        assert nn.go2nn_eval_bootstrap(ptr(a), ptr(s), ptr(e), acc.shape[1], len(start) - 1, B, seed, ptr(out), _st()) == 0, nn.go2nn_last_error()
        return out.cpu().numpy()
    return call


@pytest.mark.parametrize("B", tb.BS)
@pytest.mark.parametrize("N", sorted(tb.CASES))
def test_kernel_equals_the_restatement_bit_for_bit(nn, N, B):
    tb.check_kernel_case(device_call(nn), N, B)


def test_prefix_seed_constant_cell_and_statistics(nn):
    call = device_call(nn)
    tb.check_prefix_and_seed(call)

    def reduce(acc, cell, G):
        out = torch.zeros(G, tb.COLS, dtype=torch.float64, device=DEV)
        a, c = torch.from_numpy(acc).to(DEV), torch.from_numpy(cell).to(DEV)
        assert nn.go2nn_eval_reduce(ptr(a), ptr(c), acc.shape[1], G, ptr(out), _st()) == 0
        return out.cpu().numpy()
    tb.check_constant_cell(call, reduce)
    tb.check_statistics(call)


def test_refusals(nn):
    acc, start, envs, _ = tb.reference(37)
    N, G = 37, len(start) - 1
    a, s, e = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (acc, start, envs))
    out = torch.full((4, G, tb.COLS), -3.0, dtype=torch.float64, device=DEV)
    base = dict(acc=ptr(a), start=ptr(s), envs=ptr(e), N=N, G=G, B=4, out=ptr(out))
    for what, over in tb.refusal_cases(N, G, 4):
        k = dict(base, **over)
        rc = nn.go2nn_eval_bootstrap(k["acc"], k["start"], k["envs"], k["N"], k["G"], k["B"], 1, k["out"], _st())
        assert rc == tb.EINVAL and nn.go2nn_last_error(), what
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
    bad = envs.copy(); bad[5] = N          # the device library's check is host code too: what the launch cannot see is refused before the upload
    assert nn.go2nn_eval_bootstrap_check(tb.p(start), tb.p(bad), N, G) == tb.EINVAL and nn.go2nn_eval_bootstrap_check(tb.p(start), tb.p(envs), N, G) == 0


def _evaluator(**over):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    env_cfg, train_cfg = task_registry.get_cfgs("go2_flat")
    ev = dict(class_to_dict(train_cfg.evaluation), **dict(SMALL, **over))
    return PolicyEvaluator(env_cfg, ev, task_class=task_registry.get_task_class("go2_flat"), device=DEV)


def test_evaluation_with_the_option_on(nn, monkeypatch):
    """go2_flat, 64 robots, bootstrap = 257 (two workgroups along the replicates, the second with one lane): the table is the restatement of the device's own accumulators,
    every other result is that of the option-off run, and a replayed evaluation gives the same bytes — the launch sits after the replayed chunks"""
    monkeypatch.setenv("GO2_STRICT_GRAPHS", "1")
    ac = tb.small_actor_critic().to(DEV)
    ev_off, ev_on = _evaluator(), _evaluator(bootstrap=257)
    off, on = ev_off.evaluate(ac, use_graph=False), ev_on.evaluate(ac, use_graph=False)
    assert (off["mode"], on["mode"]) == ("eager", "eager") and ev_on.num_cells == 6 and ev_on.num_envs == 64
    tb.check_on_against_off(ev_on, on, off, ev_on.acc.cpu().numpy())
    replay = ev_on.evaluate(ac, use_graph=True)
    assert replay["mode"] == "graph" and replay["table"].tobytes() == on["table"].tobytes()
    assert replay["bootstrap"]["table"].tobytes() == on["bootstrap"]["table"].tobytes() and tb.same_value(replay["overall"], on["overall"])
    ev_off.close(); ev_on.close()
