"""The recurrent actor-critic (ActorCriticRecurrent: an LSTM / GRU memory in front of each MLP head) on the CPU: the runner builds it with the reference's
parameter names; the host build of the memory kernels (include/go2nn.h ABI 7) against float64 torch; the cell kernels called directly at ragged shapes and the
stacked memory under the device tests' fp32 rule (check_* / rollout_steps / update_sequence: tests/test_gpu_recurrent.py runs the same functions on the GPU); the
fixed-shape update recurrence against the reference's split / pad / unpad generator; two PPO iterations against the reference's own (tests/golden/ppo_recurrent_iterations.npz, tools/gen_recurrent_golden.py);
the TorchScript / pkl export."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import ROOT, load_nn_emu, load_oracle
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd.rsl_rl.algorithms import PPO
from go2_rl_gym_amd.rsl_rl.modules import ActorCritic, ActorCriticRecurrent, fused
from go2_rl_gym_amd.rsl_rl.modules import fused_rnn
from go2_rl_gym_amd.rsl_rl.storage import RolloutStorage

GOLDEN = os.path.join(ROOT, "tests", "golden", "ppo_recurrent_iterations.npz")


@pytest.fixture
def kernels():
    """the memory (and the MLP nodes) on the host build of the library's kernels; restored afterwards"""
    was = (fused._LIB, fused._NN)
    fused.set_library(load_oracle())
    fused.set_nn_library(load_nn_emu())
    yield fused._NN
    fused._LIB, fused._NN = was


@pytest.fixture
def reference():
    was = (fused._LIB, fused._NN)
    fused._LIB, fused._NN = None, None
    yield
    fused._LIB, fused._NN = was


def _ref_keys(L, heads=None):
    """the reference's state_dict keys (recorded by tools/gen_recurrent_golden.py) — heads: other MLP head widths (the names of the heads as ActorCritic's)"""
    keys = [str(k) for k in np.load(GOLDEN)["lstm_keys"]]
    if heads is not None:
        keys = [k for k in keys if k.startswith("memory_")] + list(ActorCritic(16, 16, 12, actor_hidden_dims=heads, critic_hidden_dims=heads).state_dict())
    for l in range(1, L):
        keys += ["memory_%s.rnn.%s_l%d" % (m, n, l) for m in "ac" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return keys


@pytest.mark.parametrize("rnn_type,layers", [("lstm", 1), ("gru", 1), ("lstm", 2), ("gru", 2)])
def test_runner_builds_the_recurrent_policy(tmp_path, rnn_type, layers):
    """task go2_flat_rnn (and its GRU / 2-layer variants) through make_alg_runner: ActorCriticRecurrent with the reference's state_dict keys"""
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat_rnn", "--num_envs", "8", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"])
    env_cfg, train_cfg = task_registry.get_cfgs("go2_flat_rnn")
    assert train_cfg.runner.policy_class_name == "ActorCriticRecurrent" and train_cfg.policy.rnn_hidden_size == 256
    train_cfg.policy.rnn_type, train_cfg.policy.rnn_num_layers = rnn_type, layers
    env, _ = task_registry.make_env("go2_flat_rnn", args, env_cfg=env_cfg, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat_rnn", args, train_cfg=train_cfg, log_root=str(tmp_path))
    ac = runner.alg.actor_critic
    assert isinstance(ac, ActorCriticRecurrent) and ac.is_recurrent
    assert sorted(ac.state_dict()) == sorted(_ref_keys(layers, heads=train_cfg.policy.actor_hidden_dims))
    assert isinstance(ac.memory_a.rnn, nn.LSTM if rnn_type == "lstm" else nn.GRU) and ac.memory_a.rnn.input_size == 45 and ac.memory_c.rnn.input_size == 263
    assert ac.actor[0].in_features == 256 and _nn.mlp_layers(ac.actor) is not None and _nn.mlp_layers(ac.critic) is not None
    assert runner.alg.storage.saved_hidden_states_a[0].shape == (24, layers, 8, 256)
    env.close()


def test_heads_of_512_input_are_accepted_by_the_policy_kernel():
    """a 512-wide memory: the heads' input width is GO2NN_MAX_WIDTH, which mlp_layers and go2nn_pack take"""
    lib = load_nn_emu()
    ac = ActorCriticRecurrent(45, 263, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], rnn_hidden_size=512)
    assert _nn.PolicyKernel.supports(ac)
    pk = _nn.PolicyKernel(lib, ac)
    pk.pack()
    x = torch.randn(5, 512)
    np.testing.assert_allclose(pk.actor.forward(x).numpy(), ac.actor(x).detach().numpy(), atol=1e-5)


def test_abi_7_symbols_and_structs(tmp_path):
    """every new entry point is exported by the host build (and the HIP library when it is built); the ctypes structs have the header's layout"""
    names = ["go2nn_rnn_cell_forward", "go2nn_rnn_cell_backward", "go2nn_rnn_reset"]
    lib = load_nn_emu()
    assert lib.go2nn_abi_version() == 7 == _nn.GO2NN_ABI_VERSION
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + ([_nn.NN_LIB] if os.path.exists(_nn.NN_LIB) else [])
    for path in libs:
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
        assert set(names) <= syms, (path, set(names) - syms)
    structs = ["Go2nnRnnCellJob", "Go2nnRnnCellBwdJob"]
    lines = []
    for s in structs:
        lines.append('printf("%s %%zu", sizeof(%s));' % (s, s))
        for f, _ in getattr(_nn, s)._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (s, f))
        lines.append('printf("\\n");')
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/go2nn.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    subprocess.run(["gcc", "-I", ROOT, "-o", str(tmp_path / "probe"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.split("\n")
    for s, line in zip(structs, out):
        got = line.split()
        cs = getattr(_nn, s)
        assert got[0] == s and int(got[1]) == C.sizeof(cs)
        assert [int(x) for x in got[2:]] == [getattr(cs, f).offset for f, _ in cs._fields_], s


# ---- the accuracy rule of the device tests (tests/test_gpu_recurrent.py), usable on either build -----------------------------------------------------------

class Rule:
    """error against float64 <= 4 x the error of the same evaluation in fp32 torch + 2e-7, in units of max(1, |reference|) per element.  add() records, report()
    prints every figure and then asserts them all."""

    def __init__(self):
        self.rows = []

    def add(self, name, got, f32, f64):
        """rows of one name are ONE evaluation: their figures are the maxima over all of them (a chained sequence is held as a whole — at 4 .. 8 elements per
        step the fp32 yardstick of a single step is a draw from a handful of roundings and can be next to 0)"""
        unit = f64.abs().clamp(min=1.0)
        e, e32 = ((got.double() - f64).abs() / unit).max().item(), ((f32.double() - f64).abs() / unit).max().item()
        for k, r in enumerate(self.rows):
            if r[0] == name:
                self.rows[k] = (name, e if e != e or e > r[1] else r[1], max(e32, r[2]))          # (a NaN stays)
                return
        self.rows.append((name, e, e32))

    def worst(self, prefix=""):
        rows = [r for r in self.rows if r[0].startswith(prefix)]
        return max(r[1] for r in rows), max(r[2] for r in rows)

    def report(self, label):
        bad = [r for r in self.rows if not r[1] <= 4 * r[2] + 2e-7]          # (not <=: a NaN fails)
        print("[fp32 rule] %s: worst %.3g (fp32 torch %.3g)%s" % ((label,) + self.worst() + ("".join("; MISS %s %.3g (fp32 %.3g)" % r for r in bad),)))
        assert not bad, (label, bad)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- the host build of the kernels against float64 torch ----------------------------------------------------------------------------------------------------

def _ac(typ, H, L, K_a=45, K_c=60, seed=0):
    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(K_a, K_c, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type=typ, rnn_hidden_size=H, rnn_num_layers=L)
    with torch.no_grad():
        for p in ac.parameters():
            p.mul_(2.0)          # (larger weights than the default init: saturated gates and real state updates)
    return ac


def _twins(mems, H, L, dtype, device):
    """nn.LSTM / nn.GRU of the memories' parameters in `dtype`"""
    out = [type(m.rnn)(m.rnn.input_size, H, L).to(device, dtype) for m in mems]
    for r, m in zip(out, mems):
        r.load_state_dict({k: v.to(dtype) for k, v in m.rnn.state_dict().items()})
    return out


def rollout_steps(device, typ, H, L, N, rule=False, T=5, p_done=0.3):
    """RolloutMemory.step (both memories grouped, every layer, the storage slot of the state before the step) and .reset over T chained steps against nn.LSTM /
    nn.GRU in float64.  rule False: the host test's absolute bounds.  rule True: every state tensor of every layer under the fp32 rule (nn.LSTM / nn.GRU in
    fp32 as the yardstick), slots bit-equal to the state before the step, reset rows exactly 0, and at the end the critic-only step of compute_returns.
    -> every output of the sequence (for run-to-run comparison)"""
    ac = _ac(typ, H, L).to(device)
    ac.init_hidden_states(N, device)
    mems = (ac.memory_a, ac.memory_c)
    st = RolloutStorage(N, T, [45], [60], [12], device)
    st.init_hidden_states(len(ac.memory_a.states()), len(ac.memory_c.states()), L, H)
    rm = fused_rnn.RolloutMemory(ac)
    rm.images()
    lstm = typ == "lstm"
    dts = (torch.float64, torch.float32) if rule else (torch.float64,)
    refs = {dt: _twins(mems, H, L, dt, device) for dt in dts}
    z = lambda dt: torch.zeros(L, N, H, dtype=dt, device=device)
    states = {dt: [(z(dt), z(dt)) if lstm else z(dt) for _ in range(2)] for dt in dts}
    tup = lambda s: s if lstm else (s,)
    g = torch.Generator().manual_seed(1)
    check, outs = Rule(), []

    def advance(j, x):
        res = {}
        for dt in dts:
            res[dt], states[dt][j] = refs[dt][j](x.to(dt).unsqueeze(0), states[dt][j])
        return res

    def compare(j, s, h):
        out64 = res[torch.float64][0]
        if not rule:
            np.testing.assert_allclose(h.cpu().numpy(), out64.cpu().numpy(), atol=2e-5)
            return
        assert h.data_ptr() == mems[j].states()[0][L - 1].data_ptr()
        for k, name in enumerate("hc"[:len(mems[j].states())]):
            check.add("%s memory %s" % (("actor", "critic")[j], name), mems[j].states()[k], tup(states[torch.float32][j])[k], tup(states[torch.float64][j])[k])

    with torch.no_grad():
        for s in range(T):
            xs = [torch.randn(N, 45, generator=g).to(device), torch.randn(N, 60, generator=g).to(device)]
            before = [[t.clone() for t in m.states()] for m in mems]
            prev = [[t.clone() for t in tup(sts)] for sts in states[torch.float64]]
            hs = rm.step(xs, slots=[(st.saved_hidden_states_a, s), (st.saved_hidden_states_c, s)])
            for j in range(2):
                res = advance(j, xs[j])
                compare(j, s, hs[j])
                saved = st.saved_hidden_states_a if j == 0 else st.saved_hidden_states_c
                for k in range(len(saved)):
                    if rule:
                        assert same_bits(saved[k][s], before[j][k]), ("slot", s, j, k)
                    else:
                        np.testing.assert_allclose(saved[k][s].cpu().numpy(), prev[j][k].cpu().numpy(), atol=2e-5)
            done = (torch.rand(N, generator=g) < p_done).to(torch.uint8).to(device)
            rm.reset(done)
            keep = (done == 0).view(1, N, 1)
            for dt in dts:
                states[dt] = [tuple(x * keep for x in sts) if lstm else sts * keep for sts in states[dt]]
            for j, m in enumerate(mems):
                for a, b in zip(m.states(), tup(states[torch.float64][j])):
                    if not rule:
                        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=2e-5)
                    assert (a[:, done.bool()] == 0).all() and a.shape == (L, N, H)
            outs += [h.clone() for h in hs] + [t.clone() for m in mems for t in m.states()]
        if rule:          # compute_returns: the critic memory alone, one more step; the actor's state stays as it is
            x = torch.randn(N, 60, generator=g).to(device)
            actor = [t.clone() for t in mems[0].states()]
            h = rm.step([x], which=(1,))[0]
            res = advance(1, x)
            compare(1, T, h)
            assert all(same_bits(a, b) for a, b in zip(actor, mems[0].states()))
            outs += [h.clone()] + [t.clone() for t in mems[1].states()]
            for k in range(len(st.saved_hidden_states_a)):          # (and wrote no slot)
                outs.append(st.saved_hidden_states_a[k].clone())
            check.report("rollout %s H=%d L=%d N=%d on %s split=%s" % (typ, H, L, N, device, fused._SPLIT))
    return outs


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L", [(16, 1), (16, 2), (256, 1)])
def test_rollout_step_matches_float64(kernels, typ, H, L):
    """RolloutMemory.step (both memories, every layer, storage slot of the state before the step) and .reset against nn.LSTM / nn.GRU in float64, 5 chained steps"""
    rollout_steps("cpu", typ, H, L, 24)


ROLLOUT_CASES = [(16, 2, 24), (20, 1, 37), (100, 3, 257), (256, 2, 1000), (4, 2, 1)]          # (H, L, N)


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L,N", [c for c in ROLLOUT_CASES if c != (256, 2, 1000)])
def test_stacked_ragged_rollout_follows_the_fp32_rule(kernels, typ, H, L, N):
    """up to three layers, row counts and widths that fill no tile and no workgroup, one env: layer l is fed from the state layer l - 1 has just written
    (the 1000-env case runs on the device only: the host build's plain-loop products take most of a minute there)"""
    rollout_steps("cpu", typ, H, L, N, rule=True)


def _reference_sequence(rnn64, x, saved, dones):
    """float64 autograd through nn.LSTM / nn.GRU, step by step with the carried state replaced by the saved one after a done (the reference's semantics)"""
    T = x.shape[0]
    lstm = isinstance(rnn64, nn.LSTM)
    saved = [s.to(x.dtype).contiguous() for s in saved]          # (torch's fp32 RNN on the device takes contiguous states only)
    st = (saved[0][0], saved[1][0]) if lstm else saved[0][0]
    ys = []
    for t in range(T):
        if t > 0:
            d = dones[t - 1].bool().view(1, -1, 1)
            st = tuple(torch.where(d, s[t], c) for s, c in zip(saved, st)) if lstm else torch.where(d, saved[0][t], st)
        y, st = rnn64(x[t:t + 1], st)
        ys.append(y[0])
    return torch.stack(ys)


def _update_dones(T, B, g=None):
    """dones at t = 0, mid-sequence and t = T - 2, several per env, one env done at every step (each where the block has that env and step); g: plus 20 % random"""
    dones = torch.zeros(T, B, dtype=torch.uint8)
    for t, b in ((0, 1), (3, 2), (T - 2, 3), (1, 4), (2, 4), (5, 4)):
        if 0 <= t < T and b < B:
            dones[t, b] = 1
    if B > 6:
        dones[:, 6] = 1
    if g is not None:
        dones |= (torch.rand(T, B, generator=g) < 0.2).to(torch.uint8)
    return dones


def update_sequence(device, typ, H, L, T, B, K, rule=False):
    """memory_sequence (RnnFunction: cell forward / backward + the GEMMs): the output and all 4 L parameter gradients against float64 autograd through nn.LSTM /
    nn.GRU.  rule False: the host test's inputs and absolute bounds.  rule True: the saved states and the dones are handed over as RolloutStorage.
    recurrent_fixed_batches does (the middle third of the envs of [T, L, 3B, H] and [T, 3B, 1]: strided views at an offset), 20 % random dones on top of the
    pattern, everything under the fp32 rule.  -> [y, gradients...] (for run-to-run comparison)"""
    torch.manual_seed(3)
    mem = _ac(typ, H, L, K_a=K).memory_a.to(device)
    lstm = typ == "lstm"
    x = torch.randn(T, B, K).to(device)
    if rule:
        g = torch.Generator().manual_seed(5)
        dones = torch.zeros(T, 3 * B, 1, dtype=torch.uint8)
        dones[:, B:2 * B, 0] = _update_dones(T, B, g)
        dones[:, :B] = 1 - dones[:, B:2 * B]          # (the neighbouring slices hold what this one must not read)
        dones = dones.to(device)[:, B:2 * B][..., 0]
        saved = [(torch.randn(T, L, 3 * B, H, generator=g) * 0.5).to(device)[:, :, B:2 * B] for _ in range(2 if lstm else 1)]
        gy = torch.randn(T, B, H, generator=g).to(device)
        assert not saved[0].is_contiguous() and saved[0].storage_offset() > 0 and dones.storage_offset() > 0
    else:
        dones = _update_dones(T, B).to(device)
        saved = [(torch.randn(T, L, B, H) * 0.5).to(device) for _ in range(2 if lstm else 1)]
        gy = torch.randn(T, B, H).to(device)
    y = fused_rnn.memory_sequence(mem, x, saved, dones)
    (y * gy).sum().backward()
    res = {}
    for dt in (torch.float64, torch.float32) if rule else (torch.float64,):
        r = _twins([mem], H, L, dt, device)[0]
        yr = _reference_sequence(r, x.to(dt), saved, dones)
        (yr * gy.to(dt)).sum().backward()
        res[dt] = (yr.detach(), {n: p.grad for n, p in r.named_parameters()})
    y64, g64 = res[torch.float64]
    names = [n for n, _ in mem.rnn.named_parameters()]
    assert len(names) == 4 * L and all(p.grad is not None for p in mem.rnn.parameters())
    if rule:
        check = Rule()
        check.add("y", y.detach(), res[torch.float32][0], y64)
        for n, p in mem.rnn.named_parameters():
            check.add("d" + n, p.grad, res[torch.float32][1][n], g64[n])
        check.report("update %s H=%d L=%d T=%d B=%d K=%d on %s split=%s: y %.3g (fp32 torch %.3g), gradients %.3g (%.3g)"
                     % ((typ, H, L, T, B, K, device, fused._SPLIT) + check.worst("y") + check.worst("d")))
    else:
        np.testing.assert_allclose(y.detach().cpu().numpy(), y64.cpu().numpy(), atol=3e-5)
        for n, p in mem.rnn.named_parameters():
            scale = max(1.0, g64[n].abs().max().item())
            np.testing.assert_allclose(p.grad.cpu().numpy(), g64[n].cpu().numpy(), atol=5e-5 * scale, err_msg=n)
    return [y.detach()] + [p.grad for p in mem.rnn.parameters()]


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L", [(16, 1), (16, 2), (256, 1)])
def test_update_recurrence_forward_backward_matches_float64(kernels, typ, H, L):
    """RnnFunction (cell forward / backward + the GEMMs) against float64 autograd: dones at t = 0, mid-sequence, t = T - 2, several per env"""
    update_sequence("cpu", typ, H, L, 7, 12, 20)


UPDATE_CASES = [(16, 2, 7, 12, 20), (20, 1, 7, 37, 45), (20, 3, 5, 37, 45), (100, 2, 7, 13, 263), (4, 2, 3, 1, 5)]          # (H, L, T, B, K)


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L,T,B,K", UPDATE_CASES)
def test_stacked_ragged_update_follows_the_fp32_rule(kernels, typ, H, L, T, B, K):
    """up to three layers (a lower layer's gradient is dgi W_ih of the layer above), ragged rows and widths, one env; states and dones as strided views"""
    update_sequence("cpu", typ, H, L, T, B, K, rule=True)


# ---- the cell kernels called directly (csrc/go2nn_rnn.h through the ctypes structs of _nn); the same functions run on the HIP kernels in tests/test_gpu_recurrent.py --

GO2NN_EINVAL = -22                                                                                  # include/go2nn.h
CELL_SHAPES = [(1, 1), (1, 4), (51, 5), (64, 4), (257, 1), (3, 20), (37, 36), (257, 100), (5, 512)]          # (B, H): 255, 256, 257 elements; H odd, ragged, the maximum
RESET_SHAPES = [(1, 4), (37, 20), (257, 100), (64, 256)]
DONE_PATTERNS = ("none", "all", "first", "last", "random")
TYPES = {"lstm": _nn.GO2NN_RNN_LSTM, "gru": _nn.GO2NN_RNN_GRU}
PAD, SENTINEL = 64, -12345.678


class Outs:
    """output buffers with PAD sentinel floats behind each; tails() compares them bit for bit after the calls"""

    def __init__(self, device):
        self.device, self.bufs = device, []

    def new(self, *shape):
        n = int(np.prod(shape))
        full = torch.full((n + PAD,), SENTINEL, device=self.device)
        self.bufs.append((full, n))
        return full[:n].view(*shape)

    def of(self, t):
        """a padded copy of t (a buffer the kernel updates in place)"""
        o = self.new(*t.shape)
        o.copy_(t)
        return o

    def tails(self):
        want = bits(torch.full((PAD,), SENTINEL, device=self.device))
        for full, n in self.bufs:
            assert torch.equal(bits(full[n:]), want), "write past the end of a %d-float output" % n

    def untouched(self):
        want = bits(torch.full((1,), SENTINEL, device=self.device))
        return all(bool((bits(full) == want).all()) for full, _ in self.bufs)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if torch.device(device).type == "cuda" else None


def fwd_job(typ, B, H, **ptrs):
    q = _nn.Go2nnRnnCellJob()
    for k, t in ptrs.items():
        setattr(q, k, _ptr(t))
    q.B, q.H, q.type = B, H, TYPES.get(typ, typ)
    return q


def bwd_job(typ, B, H, **ptrs):
    q = _nn.Go2nnRnnCellBwdJob()
    for k, t in ptrs.items():
        setattr(q, k, _ptr(t))
    q.B, q.H, q.type = B, H, TYPES.get(typ, typ)
    return q


def cell_forward(lib, device, jobs, n=None):
    return lib.go2nn_rnn_cell_forward((_nn.Go2nnRnnCellJob * max(len(jobs), 1))(*jobs), len(jobs) if n is None else n, _stream(device))


def cell_backward(lib, device, jobs, n=None):
    return lib.go2nn_rnn_cell_backward((_nn.Go2nnRnnCellBwdJob * max(len(jobs), 1))(*jobs), len(jobs) if n is None else n, _stream(device))


def done_rows(pattern, B, g):
    d = torch.zeros(B, dtype=torch.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "first":
        d[0] = 1
    elif pattern == "last":
        d[B - 1] = 1
    elif pattern == "random":
        d = (torch.rand(B, generator=g) < 0.5).to(torch.uint8)
    return d


def cell_reference(typ, gi, gh, hp, cp):
    """one step by torch's documented formulas (nn.LSTM: i, f, g, o; nn.GRU: r, z, n with r applied to W_hn h + b_hn) in the arguments' dtype
    -> h, c (None for a GRU), the four blocks the kernel saves"""
    if typ == "lstm":
        i, f, g, o = (gi + gh).chunk(4, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * cp + i * g
        return o * torch.tanh(c), c, [i, f, g, o]
    (ir, iz, in_), (hr, hz, hn) = gi.chunk(3, dim=1), gh.chunk(3, dim=1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(in_ + r * hn)
    return (1 - z) * n + z * hp, None, [r, z, n, hn]


def cell_inputs(typ, B, H, device, seed=0):
    """gate pre-activations 3 N(0, 1) (saturated and open gates), states N(0, 1)"""
    g = torch.Generator().manual_seed(1000 * B + H + seed)
    G = 4 if typ == "lstm" else 3
    s = 3.0 / np.sqrt(2.0)
    t = {"gi": torch.randn(B, G * H, generator=g) * s, "gh": torch.randn(B, G * H, generator=g) * s, "h_prev": torch.randn(B, H, generator=g), "sub_h": torch.randn(B, H, generator=g)}
    if typ == "lstm":
        t.update(c_prev=torch.randn(B, H, generator=g), sub_c=torch.randn(B, H, generator=g))
    return {k: v.to(device) for k, v in t.items()}, g


def full_forward(lib, device, typ, B, H, inp, done, together=None):
    """the job with every optional pointer set, on fresh padded outputs -> dict of outputs (launched, unless `together` collects the job for a grouped launch)"""
    lstm = typ == "lstm"
    o = Outs(device)
    out = {k: o.new(B, H) for k in ("h", "save_h", "next_h") + (("c", "save_c", "next_c") if lstm else ())}
    out["gates"] = o.new(B, 4 * H)
    job = fwd_job(typ, B, H, done=done, **inp, **out)
    if together is None:
        rc = cell_forward(lib, device, [job])
        assert rc == 0, lib.go2nn_last_error().decode()
    else:
        together.append(job)
    out["_outs"] = o
    return out


def check_cell_forward(lib, device, typ, B, H):
    """-> Rule with the figures of h, c and the four saved blocks"""
    lstm = typ == "lstm"
    inp, g = cell_inputs(typ, B, H, device)
    state = [inp["h_prev"]] + ([inp["c_prev"]] if lstm else [])
    args = (typ, inp["gi"], inp["gh"], inp["h_prev"], inp.get("c_prev"))
    h64, c64, gates64 = cell_reference(args[0], *[None if a is None else a.double() for a in args[1:]])
    h32, c32, gates32 = cell_reference(*args)
    check, first = Rule(), None
    for pattern in DONE_PATTERNS:
        done = done_rows(pattern, B, g).to(device)
        out = full_forward(lib, device, typ, B, H, inp, done)
        if first is None:
            first = out
            check.add("h", out["h"], h32, h64)
            if lstm:
                check.add("c", out["c"], c32, c64)
            for k in range(4):
                check.add("gates[%d]" % k, out["gates"][:, k * H:(k + 1) * H], gates32[k], gates64[k])
            if not lstm:
                assert same_bits(out["gates"][:, 3 * H:], inp["gh"][:, 2 * H:])          # (hn is W_hn h + b_hn itself)
        else:
            assert all(same_bits(out[k], first[k]) for k in ("h", "c", "gates") if k in out), pattern
        assert same_bits(out["save_h"], inp["h_prev"]) and (not lstm or same_bits(out["save_c"], inp["c_prev"])), pattern
        d = done.bool().view(B, 1)
        assert same_bits(out["next_h"], torch.where(d, inp["sub_h"], out["h"])), pattern
        assert not lstm or same_bits(out["next_c"], torch.where(d, inp["sub_c"], out["c"])), pattern
        out["_outs"].tails()
    # the minimal job: every optional pointer NULL
    o = Outs(device)
    new = [o.new(B, H) for _ in state]
    rc = cell_forward(lib, device, [fwd_job(typ, B, H, gi=inp["gi"], gh=inp["gh"], h_prev=inp["h_prev"], c_prev=inp.get("c_prev"), h=new[0], c=new[1] if lstm else None)])
    assert rc == 0, lib.go2nn_last_error().decode()
    assert same_bits(new[0], first["h"]) and (not lstm or same_bits(new[1], first["c"]))
    # in place, as the rollout calls it: h over h_prev, c over c_prev, the state before the step into the slot
    cur, slot = [o.of(t) for t in state], [o.new(B, H) for _ in state]
    rc = cell_forward(lib, device, [fwd_job(typ, B, H, gi=inp["gi"], gh=inp["gh"], h_prev=cur[0], c_prev=cur[1] if lstm else None, h=cur[0], c=cur[1] if lstm else None,
                                            save_h=slot[0], save_c=slot[1] if lstm else None)])
    assert rc == 0, lib.go2nn_last_error().decode()
    assert same_bits(cur[0], first["h"]) and (not lstm or same_bits(cur[1], first["c"]))
    assert all(same_bits(a, b) for a, b in zip(slot, state))
    o.tails()
    check.report("cell forward %s B=%d H=%d on %s" % (typ, B, H, device))
    return check


def check_cell_two_jobs(lib, device, specs):
    """specs: [(B, H, typ)] x 2, unequal sizes and mixed types: each job's outputs from the grouped launch are bit-equal to the same job launched alone"""
    cases = []
    for k, (B, H, typ) in enumerate(specs):
        inp, g = cell_inputs(typ, B, H, device, seed=7 + k)
        cases.append((typ, B, H, inp, done_rows("random", B, g).to(device)))
    alone = [full_forward(lib, device, *c) for c in cases]
    jobs = []
    grouped = [full_forward(lib, device, *c, together=jobs) for c in cases]
    rc = cell_forward(lib, device, jobs)
    assert rc == 0, lib.go2nn_last_error().decode()
    for a, b, spec in zip(alone, grouped, specs):
        for k in a:
            if k != "_outs":
                assert same_bits(a[k], b[k]), (spec, k)
                assert not bool((bits(b[k]) == bits(torch.full((1,), SENTINEL, device=device))).any()), (spec, k, "an element was left unwritten")
        b["_outs"].tails()


def check_cell_backward(lib, device, typ, B, H):
    """the forward kernel's own gates and c, then go2nn_rnn_cell_backward against autograd through the float64 (and fp32) restatement with gi, gh, h_prev, c_prev
    as leaves.  Variants: the last step (dh_rec NULL; the carry buffer is then not read: it holds NaN), done NULL, a random done.  -> Rule"""
    lstm = typ == "lstm"
    inp, g = cell_inputs(typ, B, H, device)
    G = 4 if lstm else 3
    o = Outs(device)
    h, gates, c = o.new(B, H), o.new(B, 4 * H), (o.new(B, H) if lstm else None)
    rc = cell_forward(lib, device, [fwd_job(typ, B, H, gi=inp["gi"], gh=inp["gh"], h_prev=inp["h_prev"], c_prev=inp.get("c_prev"), h=h, c=c, gates=gates)])
    assert rc == 0, lib.go2nn_last_error().decode()
    dy, dh_rec, carry_in = (torch.randn(B, H, generator=g).to(device) for _ in range(3))
    check = Rule()
    for variant in ("last step", "no done", "random done"):
        rec = None if variant == "last step" else dh_rec
        done = done_rows("random", B, g).to(device) if variant == "random done" else None
        flows = torch.zeros(B, 1, device=device) if rec is None else (torch.ones(B, 1, device=device) if done is None else (done == 0).float().view(B, 1))
        carry = o.of(carry_in if rec is not None else torch.full((B, H), float("nan"), device=device))
        dgi, dgh = o.new(B, G * H), o.new(B, G * H)
        job = bwd_job(typ, B, H, gates=gates, dy=dy, dh_rec=rec, done=done, dgi=dgi, dgh=dgh, **(dict(c=c, c_prev=inp["c_prev"], dc=carry) if lstm else dict(h_prev=inp["h_prev"], dh_carry=carry)))
        rc = cell_backward(lib, device, [job])
        assert rc == 0, lib.go2nn_last_error().decode()
        want = {}
        for dt in (torch.float64, torch.float32):
            leaves = {k: inp[k].detach().to(dt).clone().requires_grad_(True) for k in ("gi", "gh", "h_prev") + (("c_prev",) if lstm else ())}
            h_, c_, _ = cell_reference(typ, leaves["gi"], leaves["gh"], leaves["h_prev"], leaves.get("c_prev"))
            up = dy.to(dt) + flows.to(dt) * ((dh_rec if lstm else dh_rec + carry_in).to(dt))          # (dy, plus dh_rec and the GRU's incoming carry on not-done rows)
            loss = (h_ * up).sum() + ((c_ * flows.to(dt) * carry_in.to(dt)).sum() if lstm else 0.0)      # (the LSTM's incoming carry is the gradient at c_t)
            loss.backward()
            want[dt] = (leaves["gi"].grad, leaves["gh"].grad, leaves["c_prev" if lstm else "h_prev"].grad)          # (gh is a leaf: h_prev's gradient is the direct path dh z)
        for name, got, k in (("dgi", dgi, 0), ("dgh", dgh, 1), ("dc" if lstm else "dh_carry", carry, 2)):
            check.add("%s: %s" % (variant, name), got, want[torch.float32][k], want[torch.float64][k])
        if lstm:
            assert same_bits(dgh, dgi), variant
        else:          # dgh's n block is dgi_n r: one fp32 product of two stored values
            assert same_bits(dgh[:, :2 * H], dgi[:, :2 * H]) and same_bits(dgh[:, 2 * H:], dgi[:, 2 * H:] * gates[:, :H]), variant
    o.tails()
    check.report("cell backward %s B=%d H=%d on %s" % (typ, B, H, device))
    return check


def check_reset(lib, device, B, H):
    """go2nn_rnn_reset over 1 .. 4 states, 1 .. 3 layers and every done pattern: bit-equal to s[:, done] = 0; -0.0 and NaN in rows that are not done stay"""
    g = torch.Generator().manual_seed(B * 1000 + H)
    for nstates in (1, 2, 3, 4):
        for L in (1, 2, 3):
            for pattern in DONE_PATTERNS:
                done = done_rows(pattern, B, g)
                o = Outs(device)
                states, want = [], []
                for _ in range(nstates):
                    s = torch.randn(L, B, H, generator=g)
                    live = torch.nonzero(done == 0).view(-1)
                    if len(live):
                        s[:, live[0], 0], s[:, live[-1], H - 1] = -0.0, float("nan")
                    w = s.clone()
                    w[:, done.bool()] = 0
                    states.append(o.of(s.to(device)))
                    want.append(w.to(device))
                arr = (C.c_void_p * nstates)(*[s.data_ptr() for s in states])
                rc = lib.go2nn_rnn_reset(arr, nstates, L, B, H, C.c_void_p(done.to(device).data_ptr()), _stream(device))
                assert rc == 0, lib.go2nn_last_error().decode()
                for k, (s, w) in enumerate(zip(states, want)):
                    assert same_bits(s, w), (nstates, L, pattern, k)
                o.tails()


def check_refusals(lib, device):
    """what the entry points refuse: GO2NN_EINVAL, a message, and no output touched"""
    B, H = 3, 4
    inp, g = cell_inputs("lstm", B, H, device)
    done = done_rows("random", B, g).to(device)
    o = Outs(device)
    out = {k: o.new(B, H) for k in ("h", "c", "save_h", "save_c", "next_h", "next_c")}
    out["gates"] = o.new(B, 4 * H)
    full = dict(done=done, **inp, **out)
    less = lambda *drop: {k: v for k, v in full.items() if k not in drop}
    ok = fwd_job("lstm", B, H, **full)
    bad = [("0 jobs", [ok], 0), ("3 jobs", [ok, ok, ok], 3),
           ("H = 0", [fwd_job("lstm", B, 0, **full)], 1), ("H = 513", [fwd_job("lstm", B, _nn.GO2NN_MAX_WIDTH + 1, **full)], 1), ("type 2", [fwd_job(2, B, H, **full)], 1),
           ("B = 0", [fwd_job("lstm", 0, H, **full)], 1),
           ("LSTM without c", [fwd_job("lstm", B, H, **less("c"))], 1), ("next_h without sub_h", [fwd_job("lstm", B, H, **less("sub_h"))], 1),
           ("next_h without sub_h (GRU)", [fwd_job("gru", B, H, **less("sub_h", "c", "c_prev", "sub_c", "next_c", "save_c"))], 1),
           ("save_h without save_c", [fwd_job("lstm", B, H, **less("save_c"))], 1), ("the second job is bad", [ok, fwd_job("lstm", B, H, **less("c"))], 2)]
    for what, jobs, n in bad:
        assert cell_forward(lib, device, jobs, n) == GO2NN_EINVAL and b"rnn cell forward" in lib.go2nn_last_error(), what
        assert o.untouched(), what
    dy = torch.randn(B, H, generator=g).to(device)
    outb = {"dgi": o.new(B, 4 * H), "dgh": o.new(B, 4 * H), "dc": o.new(B, H)}
    fullb = dict(gates=inp["gi"], c=inp["c_prev"], c_prev=inp["c_prev"], dy=dy, **outb)
    okb = bwd_job("lstm", B, H, **fullb)
    for what, jobs, n in [("0 jobs", [okb], 0), ("3 jobs", [okb] * 3, 3), ("H = 513", [bwd_job("lstm", B, _nn.GO2NN_MAX_WIDTH + 1, **fullb)], 1), ("type 2", [bwd_job(2, B, H, **fullb)], 1),
                          ("LSTM without dc", [bwd_job("lstm", B, H, **{k: v for k, v in fullb.items() if k != "dc"})], 1)]:
        assert cell_backward(lib, device, jobs, n) == GO2NN_EINVAL and b"rnn cell backward" in lib.go2nn_last_error(), what
        assert o.untouched(), what
    states = [o.new(2, B, H) for _ in range(5)]
    ptrs = [s.data_ptr() for s in states]
    ones = C.c_void_p(torch.ones(B, dtype=torch.uint8).to(device).data_ptr())          # (every row done: a reset that ran would show)
    for what, ps, n in [("0 states", ptrs[:1], 0), ("5 states", ptrs, 5), ("a NULL state", [ptrs[0], None, ptrs[2]], 3)]:
        assert lib.go2nn_rnn_reset((C.c_void_p * len(ps))(*ps), n, 2, B, H, ones, _stream(device)) == GO2NN_EINVAL and b"rnn reset" in lib.go2nn_last_error(), what
        assert o.untouched(), what
    assert cell_forward(lib, device, [ok]) == 0 and not o.untouched()          # (the job the refused ones were derived from is a good one)
    o.tails()


def check_shape_refusal(sim_lib, device):
    """a hidden size the kernels do not take is refused where ppo.py says: PPO.init_storage (fused_rnn.check_shape), not at the first step"""
    assert fused_rnn.available()
    for H in (18, 516):
        ac = ActorCriticRecurrent(45, 60, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_hidden_size=H)
        alg = PPO(ac, device=device, lib=sim_lib)
        with pytest.raises(ValueError, match="multiple of 4 up to 512"):
            alg.init_storage(8, 4, [45], [60], [12])
        with pytest.raises(ValueError, match="multiple of 4 up to 512"):
            fused_rnn.check_shape(ac.memory_c)


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_forward_against_float64(typ, B, H):
    check_cell_forward(load_nn_emu(), "cpu", typ, B, H)


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_backward_against_float64_autograd(typ, B, H):
    check_cell_backward(load_nn_emu(), "cpu", typ, B, H)


TWO_JOBS = [[(37, 36, "lstm"), (257, 100, "gru")], [(257, 100, "gru"), (37, 36, "lstm")]]


@pytest.mark.parametrize("specs", TWO_JOBS, ids=["small-first", "large-first"])
def test_two_unequal_cell_jobs_in_one_launch(specs):
    check_cell_two_jobs(load_nn_emu(), "cpu", specs)


@pytest.mark.parametrize("B,H", RESET_SHAPES)
def test_reset_zeroes_the_done_rows_of_every_layer(B, H):
    check_reset(load_nn_emu(), "cpu", B, H)


def test_cell_entry_points_refuse_bad_arguments():
    check_refusals(load_nn_emu(), "cpu")


def test_unsupported_hidden_size_is_refused_at_init_storage(kernels):
    check_shape_refusal(load_oracle(), "cpu")


# ---- the fixed-shape update against the reference's split / pad / unpad generator ---------------------------------------------------------------------------

@pytest.mark.parametrize("typ", ["lstm", "gru"])
def test_fixed_shape_generator_equals_split_pad_generator(reference, typ):
    """Same mini-batches, same initial states (the LSTM critic starting from the actor's states included), same memory outputs after unpad: the torch memory over the
    reference's padded trajectories vs the same memory run over [T, B] with the saved state substituted after every done"""
    T, N, H = 8, 16, 16
    ac = _ac(typ, H, 1)
    st = RolloutStorage(N, T, [45], [60], [12], "cpu")
    st.init_hidden_states(len(ac.memory_a.states() or ([0, 0] if typ == "lstm" else [0])), 2 if typ == "lstm" else 1, 1, H)
    g = torch.Generator().manual_seed(4)
    st.observations.copy_(torch.randn(T, N, 45, generator=g))
    st.privileged_observations.copy_(torch.randn(T, N, 60, generator=g))
    d = (torch.rand(T, N, generator=g) < 0.25)
    d[:, 0] = False
    st.dones.copy_(d.to(torch.uint8).unsqueeze(-1))
    for s in st.saved_hidden_states_a + st.saved_hidden_states_c:
        s.copy_(torch.randn(s.shape, generator=g))
        s[1:].mul_((st.dones[:-1, :, 0] == 0).float().view(T - 1, 1, N, 1))          # (after a done the rollout saved a reset state)
    nmb = 2
    ref = list(st.reccurent_mini_batch_generator(nmb, 1))
    fixed = st.recurrent_fixed_batches(nmb)
    with torch.no_grad():
        for rb, fb in zip(ref, fixed):
            for j, mem in enumerate((ac.memory_a, ac.memory_c)):
                y_ref = mem(rb[j], rb[10], rb[9][j])
                saved = fb[9][j]
                y_fix = _reference_sequence(mem.rnn, fb[j], list(saved), fb[10])
                np.testing.assert_allclose(y_fix.numpy(), y_ref.numpy(), atol=1e-5)
            if typ == "lstm":
                assert fb[9][1] is fb[9][0]          # rollout_storage.py:230 of the reference: the critic starts from the actor's states
            for k in range(2, 9):
                np.testing.assert_array_equal(fb[k].numpy(), rb[k].numpy())


# ---- two PPO iterations against the reference's -------------------------------------------------------------------------------------------------------------

def _golden_run(monkeypatch, typ, formulation):
    g = np.load(GOLDEN)
    p = typ + "_"
    T, N = g[p + "it0_rew"].shape
    ac = ActorCriticRecurrent(45, 60, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type=typ, rnn_hidden_size=16, rnn_num_layers=1)
    sd = {k[len(p) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p + "w0_")}
    assert set(sd) == set(ac.state_dict()) == set(g[p + "keys"])
    ac.load_state_dict(sd)
    alg = PPO(ac, num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3,
              max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01, device="cpu", lib=load_oracle(),
              fused_rollout=formulation == "kernels", fused_loss=formulation == "kernels")
    if formulation == "kernels":
        alg.nn_lib = fused._NN
    alg.init_storage(N, T, [45], [60], [12])
    worst = {}
    for it in range(2):
        q = p + "it%d_" % it
        obs, cobs, noise = torch.from_numpy(g[q + "obs"]), torch.from_numpy(g[q + "cobs"]), torch.from_numpy(g[q + "noise"])
        for t in range(T):
            monkeypatch.setattr(ActorCritic, "_noise", lambda self, like, _t=t: noise[_t])
            a = alg.act(obs[t], cobs[t])
            np.testing.assert_allclose(a.numpy(), g[q + "actions"][t], atol=1e-6)
            np.testing.assert_allclose(alg.storage.values[t].numpy(), g[q + "values"][t], atol=1e-6)
            np.testing.assert_allclose(alg.storage.actions_log_prob[t].view(-1).numpy(), g[q + "logp"][t], atol=1e-5)
            alg.process_env_step(torch.from_numpy(g[q + "rew"][t]), torch.from_numpy(g[q + "dones"][t]).bool(), {"time_outs": torch.from_numpy(g[q + "time_outs"][t]).bool()})
        for name, saved in (("hid_a", alg.storage.saved_hidden_states_a), ("hid_c", alg.storage.saved_hidden_states_c)):
            for j, s in enumerate(saved):
                np.testing.assert_allclose(s.numpy(), g[q + "%s%d" % (name, j)], atol=1e-5, err_msg=name)
        alg.compute_returns(cobs[T])
        np.testing.assert_allclose(alg.storage.returns.numpy(), g[q + "returns"], atol=2e-6)
        np.testing.assert_allclose(alg.storage.advantages.numpy(), g[q + "advantages"], atol=2e-5)
        mvl, msl = alg.update()
        assert abs(mvl - float(g[q + "mean_value_loss"])) < 1e-5 and abs(msl - float(g[q + "mean_surrogate_loss"])) < 1e-5
        assert abs(alg.learning_rate - float(g[q + "lr"])) < 1e-12
        for k, v in ac.state_dict().items():
            ref = g[q + "w_" + k]
            worst[(it, k)] = float(np.max(np.abs(v.numpy() - ref)))
            np.testing.assert_allclose(v.numpy(), ref, atol=2e-6, rtol=1e-5, err_msg="iteration %d: %s" % (it, k))
    return worst


@pytest.mark.parametrize("typ", ["lstm", "gru"])
def test_two_iterations_match_reference_torch_formulation(monkeypatch, reference, typ):
    """GO2_FUSED_MLP=0's formulation: nn.LSTM / nn.GRU over the split / pad generator"""
    _golden_run(monkeypatch, typ, "reference")


@pytest.mark.parametrize("typ", ["lstm", "gru"])
def test_two_iterations_match_reference_kernel_formulation(monkeypatch, kernels, typ):
    """the product's formulation on the host build: the memory kernels, the fixed-shape update, the policy kernel and the fused loss"""
    _golden_run(monkeypatch, typ, "kernels")


# ---- export -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typ", ["lstm", "gru"])
def test_exported_recurrent_policy_reproduces_act_inference(tmp_path, reference, typ):
    """TorchScript with hidden_state (/ cell_state) buffers and reset(), and the pkl state dict, against act_inference over 50 steps with a reset in the middle"""
    from go2_rl_gym_amd.utils.exporter import export_policy_as_jit, export_policy_as_onnx, export_policy_as_pkl
    ac = _ac(typ, 16, 2)
    jit = torch.jit.load(export_policy_as_jit(ac, str(tmp_path)))
    assert hasattr(jit, "hidden_state") and hasattr(jit, "cell_state") == (typ == "lstm")
    ac2 = _ac(typ, 16, 2, seed=9)
    ac2.load_state_dict(torch.load(export_policy_as_pkl(ac, str(tmp_path))))
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for t in range(50):
            if t == 25:
                jit.reset(); ac.reset(); ac2.reset()
            x = torch.randn(1, 45, generator=g)
            want = ac.act_inference(x)
            np.testing.assert_allclose(jit(x).numpy(), want.numpy(), atol=1e-6)
            np.testing.assert_allclose(ac2.act_inference(x).numpy(), want.numpy(), atol=1e-6)
    with pytest.raises(NotImplementedError, match="recurrent"):
        export_policy_as_onnx(ac, str(tmp_path))
