"""[T, N, .] rollout tensors, GAE(lambda), advantage normalisation, shuffled mini-batches
(rsl_rl/rsl_rl/storage/rollout_storage.py:36-183).

compute_returns runs the library's GAE kernel (one lane per env, reverse scan over T) and normalises with the
mean / unbiased std of ALL advantages of ALL shards: the fp64 partial sums {sum a, sum a^2, n} are all-reduced over
torch.distributed (RCCL over xGMI on a multi-GPU node) — the one data-path collective of the rollout.
"""
import ctypes as C
import os

import torch
import torch.distributed as dist


class RolloutStorage:
    class Transition:
        def __init__(self):
            self.observations = None
            self.critic_observations = None
            self.actions = None
            self.rewards = None
            self.dones = None
            self.values = None
            self.actions_log_prob = None
            self.action_mean = None
            self.action_sigma = None
            self.hidden_states = None

        def clear(self):
            self.__init__()

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, device="cpu", lib=None):
        self.device = device
        self.lib = lib
        T, N = num_transitions_per_env, num_envs
        z = lambda *s, **k: torch.zeros(T, N, *s, device=device, **k)
        self.observations = z(*obs_shape)
        self.privileged_observations = z(*privileged_obs_shape) if privileged_obs_shape[0] is not None else None
        self.rewards, self.actions = z(1), z(*actions_shape)
        self.dones = z(1, dtype=torch.uint8)
        self.actions_log_prob, self.values, self.returns, self.advantages = z(1), z(1), z(1), z(1)
        self.mu, self.sigma = z(*actions_shape), z(*actions_shape)
        self._partials = torch.zeros(3, dtype=torch.float64, device=device)
        self.num_transitions_per_env, self.num_envs = T, N
        self.saved_hidden_states_a = self.saved_hidden_states_c = None          # recurrent policies: init_hidden_states
        self.step = 0

    def init_hidden_states(self, n_a, n_c, num_layers, hidden_size):
        """the recurrent policy's saved states (rollout_storage.py:103-117 of the reference): n_a (n_c) tensors [T, num_layers, N, H] — [h] for a GRU, [h, c] for an
        LSTM; slot t holds the state BEFORE step t (PPO.act writes it)"""
        z = lambda: torch.zeros(self.num_transitions_per_env, num_layers, self.num_envs, hidden_size, device=self.device)
        self.saved_hidden_states_a = [z() for _ in range(n_a)]
        self.saved_hidden_states_c = [z() for _ in range(n_c)]

    def add_transitions(self, transition):
        if self.step >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        s = self.step
        self.observations[s].copy_(transition.observations)
        if self.privileged_observations is not None:
            self.privileged_observations[s].copy_(transition.critic_observations)
        self.actions[s].copy_(transition.actions)
        self.rewards[s].copy_(transition.rewards.view(-1, 1))
        self.dones[s].copy_(transition.dones.view(-1, 1))
        self.values[s].copy_(transition.values)
        self.actions_log_prob[s].copy_(transition.actions_log_prob.view(-1, 1))
        self.mu[s].copy_(transition.action_mean)
        self.sigma[s].copy_(transition.action_sigma)
        self.step += 1

    def clear(self):
        self.step = 0

    def _stream(self):
        if self.lib.go2sim_is_device_library() == 1:
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    def compute_returns(self, last_values, gamma, lam):
        """rollout_storage.py:123-137.  [T,N,1] tensors are contiguous, i.e. exactly the kernel's [T][N] layout."""
        if self.lib is None:
            raise RuntimeError("RolloutStorage needs the go2sim library for its GAE kernel (no torch fallback in the product)")
        T, N = self.num_transitions_per_env, self.num_envs
        last = last_values.reshape(-1).contiguous().float()
        self._partials.zero_()
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = self.lib.go2sim_gae(p(self.rewards), p(self.dones), p(self.values), p(last), p(self.returns), p(self.advantages), p(self._partials),
                                 T, N, float(gamma), float(lam), self._stream())
        if rc != 0:
            raise RuntimeError("go2sim_gae failed: %s" % self.lib.go2sim_last_error().decode())
        if dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("GO2_FORCE_COLLECTIVES", "0") == "1"):
            dist.all_reduce(self._partials, op=dist.ReduceOp.SUM)       # {sum adv, sum adv^2, count}: 24 bytes over RCCL
        rc = self.lib.go2sim_normalize_advantages(p(self.advantages), p(self._partials), T * N, self._stream())
        if rc != 0:
            raise RuntimeError("go2sim_normalize_advantages failed: %s" % self.lib.go2sim_last_error().decode())

    def get_statistics(self):
        done = self.dones.clone()
        done[-1] = 1
        flat = done.permute(1, 0, 2).reshape(-1, 1)
        idx = torch.cat((flat.new_tensor([-1], dtype=torch.int64), flat.nonzero(as_tuple=False)[:, 0]))
        return (idx[1:] - idx[:-1]).float().mean(), self.rewards.mean()

    def mini_batch_generator(self, num_mini_batches, num_epochs=8):
        batch_size = self.num_envs * self.num_transitions_per_env
        mini_batch_size = batch_size // num_mini_batches
        indices = torch.randperm(num_mini_batches * mini_batch_size, requires_grad=False, device=self.device)
        flat = lambda t: t.flatten(0, 1)
        obs = flat(self.observations)
        cobs = flat(self.privileged_observations) if self.privileged_observations is not None else obs
        acts, vals, rets = flat(self.actions), flat(self.values), flat(self.returns)
        logp, adv, mu, sig = flat(self.actions_log_prob), flat(self.advantages), flat(self.mu), flat(self.sigma)
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                b = indices[i * mini_batch_size:(i + 1) * mini_batch_size]
                yield obs[b], cobs[b], acts[b], vals[b], adv[b], rets[b], logp[b], mu[b], sig[b], (None, None), None

    # ---- env-block mini-batches (the smoothness loss: algorithms/ppo.py) ---------------------------------------------------------------------------------
    def env_block_indices(self, num_mini_batches, env_perm):
        """-> (idx int64 [nmb, T, n], w uint8 [nmb, T, n]): mini-batch i holds all T steps of the envs env_perm[i n : (i + 1) n], time-major — idx[i, t, j] = t N +
        env_perm[i n + j] is a row of the flattened [T N, .] rollout —, w[i, t, j] = (t < T - 1 and dones[t, that env] == 0): the pair (t, t + 1) is compared"""
        T, N = self.num_transitions_per_env, self.num_envs
        if N % num_mini_batches != 0:
            raise ValueError("env-block mini-batches: %d envs are not a multiple of %d mini-batches" % (N, num_mini_batches))
        n = N // num_mini_batches
        envs = env_perm.to(torch.int64).view(num_mini_batches, 1, n)
        idx = (torch.arange(T, device=envs.device, dtype=torch.int64).view(1, T, 1) * N + envs).contiguous()
        w = (self.dones.view(-1)[idx] == 0).to(torch.uint8)
        w[:, T - 1] = 0
        return idx, w

    def env_block_mini_batch_generator(self, num_mini_batches, num_epochs=8, env_perm=None):
        """mini_batch_generator's tuple over env blocks (one env permutation per update, torch.randperm(N) unless given), followed by the pair weights w [T n] (uint8)"""
        if env_perm is None:
            env_perm = torch.randperm(self.num_envs, requires_grad=False, device=self.device)
        idx, w = self.env_block_indices(num_mini_batches, env_perm)
        flat = lambda t: t.flatten(0, 1)
        obs = flat(self.observations)
        cobs = flat(self.privileged_observations) if self.privileged_observations is not None else obs
        rows = (obs, cobs, flat(self.actions), flat(self.values), flat(self.advantages), flat(self.returns), flat(self.actions_log_prob), flat(self.mu), flat(self.sigma))
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                b = idx[i].reshape(-1)
                yield tuple(t[b] for t in rows) + ((None, None), None, w[i].reshape(-1))

    # ---- recurrent policies ------------------------------------------------------------------------------------------------------------------------------
    def reccurent_mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """The reference formulation of the recurrent update's mini-batches (GO2_FUSED_MLP=0, the CPU; the name is the reference's): contiguous env slices, every
        epoch in the same order, each slice's episode segments zero-padded into a batch of sequences (utils.EpisodeLayout, which reads the segment count back to
        the host) with the state every segment starts from.  Tuple: obs, critic obs (padded [T_pad, S, .]), actions ... sigma ([T, B, .]), (actor states, critic
        states) — [L, S, H], an (h, c) pair for an LSTM — and the validity mask [T_pad, S]."""
        from ..modules.actor_critic_recurrent import LSTM_CRITIC_STARTS_FROM_ACTOR_STATES
        from ..utils import EpisodeLayout
        lay = EpisodeLayout(self.dones)
        obs = lay.pad(self.observations)
        cobs = lay.pad(self.privileged_observations) if self.privileged_observations is not None else obs
        first = lambda saved: [lay.initial_states(s) for s in saved]
        init_a, init_c = first(self.saved_hidden_states_a), first(self.saved_hidden_states_c)
        if len(init_a) == 2 and LSTM_CRITIC_STARTS_FROM_ACTOR_STATES:
            init_c = init_a
        states = lambda init, seg: init[0][:, seg] if len(init) == 1 else tuple(x[:, seg] for x in init)
        width = self.num_envs // num_mini_batches
        batches = []
        for i in range(num_mini_batches):
            envs, seg = slice(i * width, (i + 1) * width), lay.segments_of(i * width, (i + 1) * width)
            rows = [t[:, envs] for t in (self.actions, self.values, self.advantages, self.returns, self.actions_log_prob, self.mu, self.sigma)]
            batches.append((obs[:, seg], cobs[:, seg], *rows, (states(init_a, seg), states(init_c, seg)), lay.valid[:, seg]))
        for _ in range(num_epochs):
            yield from batches

    def recurrent_fixed_batches(self, num_mini_batches):
        """The same mini-batches at fixed shapes (what modules/fused_rnn.py:RnnFunction takes): per contiguous env slice the [T, B, ...] views of the rollout, the
        saved states [T, L, B, H] of both memories and the dones [T, B] (uint8).  No host read, no padding; the slices are views (the update graph reads them in place)."""
        from ..modules.actor_critic_recurrent import LSTM_CRITIC_STARTS_FROM_ACTOR_STATES
        mb = self.num_envs // num_mini_batches
        cobs = self.privileged_observations if self.privileged_observations is not None else self.observations
        out = []
        for i in range(num_mini_batches):
            sl = lambda t, i=i: t[:, i * mb:(i + 1) * mb]
            hid_a = [s[:, :, i * mb:(i + 1) * mb] for s in self.saved_hidden_states_a]
            hid_c = [s[:, :, i * mb:(i + 1) * mb] for s in self.saved_hidden_states_c]
            if len(hid_c) == 2 and LSTM_CRITIC_STARTS_FROM_ACTOR_STATES:
                hid_c = hid_a
            out.append((sl(self.observations), sl(cobs), sl(self.actions), sl(self.values), sl(self.advantages), sl(self.returns), sl(self.actions_log_prob),
                        sl(self.mu), sl(self.sigma), (hid_a, hid_c), sl(self.dones)[..., 0]))
        return out
