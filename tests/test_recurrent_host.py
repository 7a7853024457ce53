"""The recurrent actor-critic (ActorCriticRecurrent: an LSTM / GRU memory in front of each MLP head) on the CPU: the runner builds it with the reference's
parameter names; the host build of the memory kernels (include/go2nn.h ABI 7) against float64 torch; the fixed-shape update recurrence against the reference's
split / pad / unpad generator; two PPO iterations against the reference's own (tests/golden/ppo_recurrent_iterations.npz, tools/gen_recurrent_golden.py);
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


# ---- the host build of the kernels against float64 torch ----------------------------------------------------------------------------------------------------

def _ac(typ, H, L, K_a=45, K_c=60, seed=0):
    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(K_a, K_c, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_type=typ, rnn_hidden_size=H, rnn_num_layers=L)
    with torch.no_grad():
        for p in ac.parameters():
            p.mul_(2.0)          # (larger weights than the default init: saturated gates and real state updates)
    return ac


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L", [(16, 1), (16, 2), (256, 1)])
def test_rollout_step_matches_float64(kernels, typ, H, L):
    """RolloutMemory.step (both memories, every layer, storage slot of the state before the step) and .reset against nn.LSTM / nn.GRU in float64, 5 chained steps"""
    N, T = 24, 5
    ac = _ac(typ, H, L)
    ac.init_hidden_states(N, "cpu")
    st = RolloutStorage(N, T, [45], [60], [12], "cpu")
    st.init_hidden_states(len(ac.memory_a.states()), len(ac.memory_c.states()), L, H)
    rm = fused_rnn.RolloutMemory(ac)
    rm.images()
    torch.set_grad_enabled(False)
    ref = [type(m.rnn)(m.rnn.input_size, H, L).double() for m in (ac.memory_a, ac.memory_c)]
    for r, m in zip(ref, (ac.memory_a, ac.memory_c)):
        r.load_state_dict({k: v.double() for k, v in m.rnn.state_dict().items()})
    lstm = typ == "lstm"
    z = lambda: torch.zeros(L, N, H, dtype=torch.float64)
    states = [(z(), z()) if lstm else z() for _ in range(2)]
    g = torch.Generator().manual_seed(1)
    for s in range(T):
        xs = [torch.randn(N, 45, generator=g), torch.randn(N, 60, generator=g)]
        prev = [tuple(x.clone() for x in sts) if lstm else sts.clone() for sts in states]
        ha, hc = rm.step(xs, slots=[(st.saved_hidden_states_a, s), (st.saved_hidden_states_c, s)])
        for j, (r, x) in enumerate(zip(ref, xs)):
            out, states[j] = r(x.double().unsqueeze(0), states[j])
            np.testing.assert_allclose([ha, hc][j].numpy(), out[0].numpy(), atol=2e-5)
            saved = st.saved_hidden_states_a if j == 0 else st.saved_hidden_states_c
            p = prev[j] if lstm else (prev[j],)
            for k in range(len(saved)):
                np.testing.assert_allclose(saved[k][s].numpy(), p[k].numpy(), atol=2e-5)
        done = (torch.rand(N, generator=g) < 0.3).to(torch.uint8)
        rm.reset(done)
        keep = (done == 0).double().view(1, N, 1)
        states = [tuple(x * keep for x in sts) if lstm else sts * keep for sts in states]
        for j, m in enumerate((ac.memory_a, ac.memory_c)):
            for a, b in zip(m.states(), states[j] if lstm else (states[j],)):
                np.testing.assert_allclose(a.numpy(), b.numpy(), atol=2e-5)
                assert (a[:, done.bool()] == 0).all()
    torch.set_grad_enabled(True)


def _reference_sequence(rnn64, x, saved, dones):
    """float64 autograd through nn.LSTM / nn.GRU, step by step with the carried state replaced by the saved one after a done (the reference's semantics)"""
    T = x.shape[0]
    lstm = isinstance(rnn64, nn.LSTM)
    saved = [s.to(x.dtype) for s in saved]
    st = (saved[0][0], saved[1][0]) if lstm else saved[0][0]
    ys = []
    for t in range(T):
        if t > 0:
            d = dones[t - 1].bool().view(1, -1, 1)
            st = tuple(torch.where(d, s[t], c) for s, c in zip(saved, st)) if lstm else torch.where(d, saved[0][t], st)
        y, st = rnn64(x[t:t + 1], st)
        ys.append(y[0])
    return torch.stack(ys)


@pytest.mark.parametrize("typ", ["lstm", "gru"])
@pytest.mark.parametrize("H,L", [(16, 1), (16, 2), (256, 1)])
def test_update_recurrence_forward_backward_matches_float64(kernels, typ, H, L):
    """RnnFunction (cell forward / backward + the GEMMs) against float64 autograd: dones at t = 0, mid-sequence, t = T - 2, several per env"""
    T, B, K = 7, 12, 20
    torch.manual_seed(3)
    mem = _ac(typ, H, L, K_a=K).memory_a
    lstm = typ == "lstm"
    x = torch.randn(T, B, K)
    dones = torch.zeros(T, B, dtype=torch.uint8)
    dones[0, 1] = dones[3, 2] = dones[T - 2, 3] = 1
    dones[1, 4] = dones[2, 4] = dones[5, 4] = 1
    dones[:, 6] = 1
    saved = [torch.randn(T, L, B, H) * 0.5 for _ in range(2 if lstm else 1)]
    gy = torch.randn(T, B, H)
    y = fused_rnn.memory_sequence(mem, x, saved, dones)
    (y * gy).sum().backward()
    r64 = type(mem.rnn)(K, H, L).double()
    r64.load_state_dict({k: v.double() for k, v in mem.rnn.state_dict().items()})
    y64 = _reference_sequence(r64, x.double(), [s.transpose(1, 2).transpose(1, 2) for s in saved], dones)
    (y64 * gy.double()).sum().backward()
    np.testing.assert_allclose(y.detach().numpy(), y64.detach().numpy(), atol=3e-5)
    for (n, p), (_, p64) in zip(mem.rnn.named_parameters(), r64.named_parameters()):
        scale = max(1.0, p64.grad.abs().max().item())
        np.testing.assert_allclose(p.grad.numpy(), p64.grad.numpy(), atol=5e-5 * scale, err_msg=n)


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
