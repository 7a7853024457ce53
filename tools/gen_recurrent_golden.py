"""Generate tests/golden/ppo_recurrent_iterations.npz by running the REFERENCE's recurrent PPO (rsl_rl: ActorCriticRecurrent, PPO's is_recurrent branches,
RolloutStorage.reccurent_mini_batch_generator) on tiny networks: per memory type (LSTM, GRU) two full iterations — rollout with explicit sampling noise,
compute_returns, update — so that the carried hidden state and the critic memory's extra step in compute_returns are pinned.

GENERATION TIME ONLY: needs a checkout of the reference (the directory holding rsl_rl/); tests read the fixture alone.
    python tools/gen_recurrent_golden.py <reference checkout>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, H, SEED = 6, 16, 16, 7
NC = 60                # critic observation width (the fixture stays small)


def gen(rnn_type, seed):
    from rsl_rl.algorithms import PPO
    from rsl_rl.modules import ActorCriticRecurrent
    from rsl_rl.utils import split_and_pad_trajectories
    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(45, NC, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", rnn_type=rnn_type, rnn_hidden_size=H,
                              rnn_num_layers=1, init_noise_std=1.0)
    alg = PPO(ac, num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0, entropy_coef=0.01,
              learning_rate=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01, device="cpu")
    alg.init_storage(N, T, [45], [NC], [12])
    out = {"keys": np.array(list(ac.state_dict().keys()))}
    for k, v in ac.state_dict().items():
        out["w0_" + k] = v.detach().numpy().copy()
    g = torch.Generator().manual_seed(seed)
    for it in range(2):
        obs = torch.randn(T + 1, N, 45, generator=g); cobs = torch.randn(T + 1, N, NC, generator=g)
        rew = torch.randn(T, N, generator=g) * 0.05
        dones = torch.rand(T, N, generator=g) < 0.2
        dones[:, 0] = False                    # env 0 never ends: the longest trajectory is T (the reference's unpad_trajectories needs it)
        dones[0, 1] = dones[T - 2, 2] = True   # a done at t = 0 and at t = T - 2
        dones[1, 3] = dones[3, 3] = True       # several per env
        _, masks = split_and_pad_trajectories(obs[:T], dones.unsqueeze(-1))
        assert int(masks.sum(0).max()) == T, "the longest trajectory must span the rollout (the reference's unpad_trajectories reshapes by it)"
        touts = dones & (torch.rand(T, N, generator=g) < 0.5)
        noise = torch.randn(T, N, 12, generator=g)
        acts, vals, logps = [], [], []
        ctx = torch.inference_mode()          # the reference's runner collects the rollout and computes the returns under inference mode (on_policy_runner.py:135)
        ctx.__enter__()
        for t in range(T):
            # PPO.act (ppo.py:90-102) with the sampling noise made explicit: a = mu + std * eps
            alg.transition.hidden_states = ac.get_hidden_states()
            input_a = ac.memory_a(obs[t])
            ac.update_distribution(input_a.squeeze(0))
            a = (ac.action_mean + ac.action_std * noise[t]).detach()
            alg.transition.actions = a
            alg.transition.values = ac.evaluate(cobs[t]).detach()
            alg.transition.actions_log_prob = ac.get_actions_log_prob(a).detach()
            alg.transition.action_mean = ac.action_mean.detach(); alg.transition.action_sigma = ac.action_std.detach()
            alg.transition.observations = obs[t]; alg.transition.critic_observations = cobs[t]
            acts.append(a.numpy().copy()); vals.append(alg.transition.values.numpy().copy()); logps.append(alg.transition.actions_log_prob.numpy().copy())
            alg.process_env_step(rew[t], dones[t], {"time_outs": touts[t]})
        alg.compute_returns(cobs[T])
        ctx.__exit__(None, None, None)
        st = alg.storage
        p = "it%d_" % it
        out.update({p + "obs": obs.numpy(), p + "cobs": cobs.numpy(), p + "rew": rew.numpy(), p + "dones": dones.numpy().astype(np.uint8),
                    p + "time_outs": touts.numpy().astype(np.uint8), p + "noise": noise.numpy(), p + "actions": np.stack(acts), p + "values": np.stack(vals),
                    p + "logp": np.stack(logps), p + "returns": st.returns.numpy().copy(), p + "advantages": st.advantages.numpy().copy()})
        for name, saved in (("hid_a", st.saved_hidden_states_a), ("hid_c", st.saved_hidden_states_c)):
            for j, s in enumerate(saved):
                out[p + "%s%d" % (name, j)] = s.detach().numpy().copy()
        mvl, msl = alg.update()
        out[p + "mean_value_loss"], out[p + "mean_surrogate_loss"], out[p + "lr"] = np.float64(mvl), np.float64(msl), np.float64(alg.learning_rate)
        for k, v in ac.state_dict().items():
            out[p + "w_" + k] = v.detach().numpy().copy()
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    sys.path.insert(0, os.path.join(ref, "rsl_rl"))
    out = {}
    for typ in ("lstm", "gru"):
        for k, v in gen(typ, SEED).items():
            out[typ + "_" + k] = v
    path = os.path.join(ROOT, "tests", "golden", "ppo_recurrent_iterations.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
