"""PPO with clipped surrogate / clipped value loss / adaptive-KL learning rate (rsl_rl/rsl_rl/algorithms/ppo.py:38-187).

Two execution modes with identical arithmetic:
  * eager  — the reference's control flow, Python-side learning-rate decision (`.item()` syncs); used on CPU and as the
             numerical reference (tests/test_ppo_golden.py pins it against the reference's own update).
  * graphs — on a GPU: one mini-batch update (gather, forward, losses, backward, gradient clip, Adam step, KL -> learning
             rate) is captured once into a HIP graph and replayed 20x per iteration; the learning rate lives in a device
             tensor, so there is no host sync and no per-op launch overhead inside the update.

Multi-GPU (one process per GPU, torch.distributed backend 'nccl' = RCCL): each rank owns an env shard and a full policy
replica; gradients are averaged across ranks before the clip/step and the mean KL before the learning-rate decision, so
every rank takes the same branch; advantage statistics are all-reduced in RolloutStorage.compute_returns.

Symmetry augmentation (`symmetry=`, off by default; feed-forward policies only): every mini-batch is followed by its left-right mirror image — torch indexing in
eager mode, ONE go2nn_mirror_rows launch per update inside the captured permutation step in graph mode (the `symmetry augmentation` section below; utils/symmetry.py).

Empirical observation normalisation (children `obs_normalizer` / `critic_obs_normalizer` of the actor-critic, attached by the runner for
`runner.empirical_normalization`; feed-forward policies only): act() normalises storage row s in place — ONE go2nn_obs_norm_apply launch per policy step for both
streams, inside the replayed rollout —, so the update reads normalised rows and does not change; the statistics move once per iteration, at the end of update()
(the `observation normalisation` section below; modules/normalizer.py).

The env's observation buffers are persistent device buffers that the step kernel overwrites IN PLACE (the reference
rebinds `obs_buf` to fresh tensors every step), so `act()` copies the observations into the rollout storage immediately
instead of keeping a reference until `process_env_step`.
"""
import math
import os

import torch

from ..modules.actor_critic import ActorCritic as _AC
from ..storage import RolloutStorage
from ._base import _RANDPERM, _FusedPPOLoss, _RolloutHeads, _collectives_on, _world
from ._graph import CapturedStep, GradBucket, all_captured


class PPO(_RolloutHeads):
    def __init__(self, actor_critic, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95, value_loss_coef=1.0,
                 entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01,
                 device="cpu", lib=None, use_graphs=None, fused_loss=None, fused_rollout=None, symmetry=False, mirror_loss_coef=0.0, diagnostics=False,
                 normalize_value=False, normalize_value_eps=1e-2, normalize_value_until=None, normalize_value_preserve=False, smooth_loss_coef=0.0):
        mirror_loss_coef = 0.0 if mirror_loss_coef is None else float(mirror_loss_coef)
        if not (math.isfinite(mirror_loss_coef) and mirror_loss_coef >= 0.0):
            raise ValueError("PPO(mirror_loss_coef=...) takes a finite weight >= 0, got %r" % (mirror_loss_coef,))
        smooth_loss_coef = 0.0 if smooth_loss_coef is None else float(smooth_loss_coef)
        if not (math.isfinite(smooth_loss_coef) and smooth_loss_coef >= 0.0):
            raise ValueError("PPO(smooth_loss_coef=...) takes a finite weight >= 0, got %r" % (smooth_loss_coef,))
        self.desired_kl, self.schedule, self.learning_rate = desired_kl, schedule, learning_rate
        self.actor_critic = actor_critic
        self.actor_critic.to(device)
        self.storage = None
        on_gpu = self._init_modes(device, lib, learning_rate, use_graphs, fused_loss, fused_rollout)
        self._params = list(self.actor_critic.parameters())
        self.optimizer = self._make_adam(self._params)
        self.transition = RolloutStorage.Transition()
        self.clip_param, self.num_learning_epochs, self.num_mini_batches = clip_param, num_learning_epochs, num_mini_batches
        self.value_loss_coef, self.entropy_coef, self.gamma, self.lam = value_loss_coef, entropy_coef, gamma, lam
        self.max_grad_norm, self.use_clipped_value_loss = max_grad_norm, use_clipped_value_loss
        self._graph = None
        # PPO.act as ONE fp32-MFMA launch (include/go2nn.h): both MLPs + the sampling head; on the GPU by default when the modules are plain
        # Linear / ELU stacks (GO2_FUSED_POLICY=0 restores the hipBLASLt chains + go2sim_act_head).  nn_lib: tests hand in the host build.
        self.nn_lib = None
        self._pk_on = on_gpu and lib is not None and os.environ.get("GO2_FUSED_POLICY", "1") == "1"
        # a recurrent policy (modules/actor_critic_recurrent.py), the is_recurrent branches of the reference (ppo.py:90-93,123-126): its memories' outputs take the
        # place of the observations in front of the same heads (_sample, _value); what is specific to it is in the _rnn_* methods below
        self._rnn, self._rm = bool(getattr(actor_critic, "is_recurrent", False)), None
        if self._rnn and _world() > 1:
            raise NotImplementedError("recurrent policies (ActorCriticRecurrent) train on one rank only: multi-rank recurrent PPO is not implemented")
        # left-right symmetry augmentation: every mini-batch of the update is followed by its mirror image (utils/symmetry.py holds the tables and what this is not);
        # off: nothing is loaded, allocated or launched.  The rollout, GAE, the storage and the checkpoints do not know about it; with several ranks it is rank-local.
        self._sym, self._sym_t, self._aug = self._symmetry_tables(symmetry), None, None
        if self._sym is not None and self._rnn:
            raise NotImplementedError("symmetry augmentation with a recurrent policy is not implemented (the mirrored hidden state is a different piece of work)")
        # the mirror (equivariance) loss on the augmented mini-batches (the `mirror loss` section below): 0 = off, and then nothing is loaded, allocated or launched.
        # mirror_loss: the last update's mean of L_mirror / coef (= equivariance_rmse^2 of its mini-batches) over its mini-batch steps
        self.mirror_loss_coef, self.mirror_loss, self._ml, self._ml_dev = mirror_loss_coef, 0.0, None, None
        if mirror_loss_coef > 0.0 and self._rnn:
            raise NotImplementedError("the mirror loss with a recurrent policy is not implemented (it is a term on the mini-batches of symmetry augmentation)")
        if mirror_loss_coef > 0.0 and self._sym is None:
            raise ValueError("PPO(mirror_loss_coef > 0) is a term on the mirror-augmented mini-batches: it needs symmetry=mirror_tables(env_cfg) (algorithm.symmetry = True; "
                             "--mirror_loss sets both)")
        # the temporal action-smoothness loss on env-block mini-batches (the `smoothness loss` section below): 0 = off, and then the mini-batches, every launch and the
        # state dict are what they are without it.  smooth_loss: the last update's mean of L_smooth / coef over its mini-batch steps
        self.smooth_loss_coef, self.smooth_loss, self._sl, self._sw, self._sw_all = smooth_loss_coef, 0.0, None, None, None
        if smooth_loss_coef > 0.0 and self._rnn:
            raise NotImplementedError("the smoothness loss with a recurrent policy is not implemented: its heads run in modules/fused_rnn.py, on the memories' outputs of "
                                      "whole episode segments")
        # empirical observation normalisation: present iff the actor-critic has the children (the runner attaches them; a checkpoint that carries them too).  Absent:
        # nothing is loaded, allocated or launched.
        self._on_state, self._on_merged = None, False
        self._obs_norm()
        # the update's diagnostics (_diag.py): off, nothing is loaded, allocated or launched; on, they read what the update reads and write tables of their own
        if diagnostics and self._rnn:
            raise NotImplementedError("algorithm.diagnostics with a recurrent policy is not implemented: its heads run in modules/fused_rnn.py, on the memories' outputs "
                                      "of whole episode segments")
        self._init_diagnostics(diagnostics, ("all",), [(self.optimizer, "")])
        # value normalisation (_base.py): off, nothing is loaded, allocated or launched, and the state dict keeps its keys
        self._init_value_norm(self.actor_critic, normalize_value, normalize_value_eps, normalize_value_until, normalize_value_preserve)
        self._sync_replicas(self.actor_critic)

    def rebind_lr(self):
        """After optimizer.load_state_dict (which may bring a float lr, e.g. from a reference checkpoint): put the device-resident
        learning-rate tensor the captured graph reads and writes back into the param groups."""
        lr = self.optimizer.param_groups[0]["lr"]
        self.learning_rate = float(lr)
        if self._lr_t is not None:
            self._lr_t.fill_(self.learning_rate)
            for g in self.optimizer.param_groups:
                g["lr"] = self._lr_t

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape):
        if self.smooth_loss_coef > 0.0:          # env-block mini-batches: whole environments, at least one pair of successive steps
            if num_envs % self.num_mini_batches != 0:
                raise ValueError("smooth_loss_coef > 0 takes mini-batches of whole environments: %d envs are not a multiple of %d mini-batches" % (num_envs, self.num_mini_batches))
            if num_transitions_per_env < 2:
                raise ValueError("smooth_loss_coef > 0 compares successive steps of a rollout: %d step per env holds no pair" % num_transitions_per_env)
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape, self.device, lib=self.lib)
        if self._sym is not None:
            st = self.storage
            for key, t in (("obs", st.observations), ("cobs", st.privileged_observations), ("act", st.actions)):
                if t is not None and len(self._sym_table(key)[0]) != t.shape[-1]:
                    raise ValueError("symmetry: the rollout's %s rows have %d columns, their mirror table %d" % (key, t.shape[-1], len(self._sym_table(key)[0])))
        if self._rnn:
            ac = self.actor_critic
            ac.init_hidden_states(num_envs, self.device)
            self.storage.init_hidden_states(len(ac.memory_a.states()), len(ac.memory_c.states()), ac.memory_a.rnn.num_layers, ac.memory_a.rnn.hidden_size)
            self._rnn_memory()          # (on the library's kernels: checks the memory's shape now, not at the first step)

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    # The heads on x, the observations — of a recurrent policy its memories' outputs: ActorCriticRecurrent's own act() / evaluate() would step the memories first.
    def _sample(self, x):
        return _AC.act(self.actor_critic, x) if self._rnn else self.actor_critic.act(x)

    def _value(self, x):
        return self.actor_critic.critic(x) if self._rnn else self.actor_critic.evaluate(x)

    # ------------------------------------------------------------------ rollout half (ppo.py:90-118)
    def act(self, obs, critic_obs):
        st, ac = self.storage, self.actor_critic
        s = self._begin_step()
        self._store_obs_rows(obs, critic_obs, s)
        on = self._obs_norm()
        if on is not None:          # storage row s becomes the normalised row, whoever wrote it (the env's step kernel, the sensor kernel, the copy above)
            obs, critic_obs = self._obs_norm_rows(on, s)
        x_a, x_c = self._rnn_step(obs, critic_obs, s) if self._rnn else (obs, critic_obs)
        if not self.fused_rollout:
            return self._transition_to_rows(ac, self._sample(x_a), self._value(x_c), s)
        pk = self._policy_kernel()
        if not (x_a.is_contiguous() and x_c.is_contiguous() and x_a.dtype == torch.float32 and x_c.dtype == torch.float32):
            pk = None
        self._ensure_packed(pk, s)
        if pk is not None:
            actions = pk.act(x_a, x_c, self._rollout_noise(ac, st, s), st.actions[s], st.mu[s], st.sigma[s], st.actions_log_prob[s].view(-1), st.values[s].view(-1))
            self._vn_rows_raw(pk, s)
            return self._transition_from_rows(actions, s)
        mu, value = self._pair(lambda: ac.actor(x_a), lambda: self._value(x_c), enabled=self._capture)
        return self._act_head(mu, ac.std, self._rollout_noise(ac, st, s), value, s)

    def _policy_kernel(self):
        """-> the fused policy kernel for this actor-critic, or None (not asked for / modules it does not cover).  On a GPU the library must
        be there: a missing libgo2nn_hip.so raises (no silent fallback to the slower path)."""
        if self._pk is None:
            lib = self.nn_lib
            if lib is None and self._pk_on:
                from ... import _nn
                lib = _nn.load_nn()
            ok = False
            if lib is not None:
                from ... import _nn
                ok = _nn.PolicyKernel.supports(self.actor_critic) and self.storage is not None and (self.storage.privileged_observations is not None or self._rnn)
            self._pk = _nn.PolicyKernel(lib, self.actor_critic, value_fold=self._vn_fold()) if ok else False
        return self._kernel()

    def process_env_step(self, rewards, dones, infos):
        s = self._record_env_step(rewards, dones, infos)
        rm = self._rnn_memory() if self._rnn else None
        if rm is not None:
            rm.reset(self.storage.dones[s].view(-1))          # (uint8 done row of the step: written by the env kernel or the store above)
        else:
            self.actor_critic.reset(dones)

    def compute_returns(self, last_critic_obs):
        rm = self._rnn_memory() if self._rnn else None
        if self._rnn and rm is None:          # (the torch formulation of a recurrent policy: evaluate() advances the critic memory itself)
            last_values = self.actor_critic.evaluate(last_critic_obs).detach()
        else:
            # (a recurrent policy: the critic memory's extra step, as the reference's evaluate() — its state carries on)
            x_c = rm.step([last_critic_obs.contiguous()], which=(1,))[0] if self._rnn else last_critic_obs
            on = self._obs_norm()
            if on is not None:          # (this observation has no storage row: normalised into a scratch buffer, the env's buffer keeps the raw frame)
                x_c = self._obs_norm_last(on, x_c)
            pk = self._kernel()
            if pk is not None and self._pk_packed and x_c.is_contiguous() and x_c.dtype == torch.float32:
                last_values = self._vn_raw_kernel(pk.critic.forward(x_c), pk)          # the bootstrap value as ONE launch on the weights packed for this rollout (they have not changed since)
            else:
                last_values = self._vn_raw(self._value(x_c).detach())
        self.storage.compute_returns(last_values, self.gamma, self.lam)
        self._vn_after_gae()

    # ------------------------------------------------------------------ update half (ppo.py:120-187)
    def _losses(self, obs_b, cobs_b, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b):
        """-> loss, value_loss, surrogate_loss, kl_mean   (a recurrent policy: obs_b / cobs_b are its memories' outputs)"""
        ac = self.actor_critic
        if self.fused_loss:
            mu_b, val_b = ac.actor(obs_b), self._value(cobs_b)          # under autograd: one node per network (modules/fused.py:_FusedMLP)
            loss, stats = _FusedPPOLoss.apply(mu_b, ac.std, val_b, self, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b)
            self._diag_torch(mu_b, ac.std, val_b, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b)
            if self.mirror_loss_coef > 0.0:
                loss = loss + self._mirror_term(mu_b)
            if self.smooth_loss_coef > 0.0:
                loss = loss + self._smooth_term(mu_b)
            return loss, stats[1], stats[0], stats[2]
        ac.update_distribution(obs_b)     # the reference calls act() here and discards the sample (ppo.py:131)
        lp_b = ac.get_actions_log_prob(act_b)
        val_b = self._value(cobs_b)
        loss, value_loss, surrogate_loss, _, kl_mean = self.ppo_terms(lp_b, val_b, ac.action_mean, ac.action_std, ac.entropy, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b)
        self._diag_torch(ac.action_mean, ac.action_std, val_b, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b)
        if self.mirror_loss_coef > 0.0:
            loss = loss + self._mirror_term(ac.action_mean)
        if self.smooth_loss_coef > 0.0:
            loss = loss + self._smooth_term(ac.action_mean)
        return loss, value_loss, surrogate_loss, kl_mean

    def _update_eager(self):
        mean_value_loss, mean_surrogate_loss, mean_mirror, mean_smooth = 0.0, 0.0, 0.0, 0.0
        if self._rnn:
            batches = self._rnn_batches()
        elif self.smooth_loss_coef > 0.0:          # all T steps of a slice of the permuted environments, time-major, and their pair weights
            batches = self.storage.env_block_mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        else:
            batches = self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        for batch in batches:
            if self._sym is not None:
                batch = self._sym_batch(batch)
            if self.smooth_loss_coef > 0.0:
                self._sw = batch[11]
            loss, value_loss, surrogate_loss, kl_mean = self._rnn_losses(batch) if self._rnn else self._losses(*batch[:9])
            self._eager_step(loss, self.optimizer, self._params, kl_mean)
            mean_value_loss += value_loss.item()
            mean_surrogate_loss += surrogate_loss.item()
            if self.mirror_loss_coef > 0.0:
                mean_mirror += self._ml.item()
            if self.smooth_loss_coef > 0.0:
                mean_smooth += self._sl.item()
        n = self.num_learning_epochs * self.num_mini_batches
        if self.mirror_loss_coef > 0.0:
            self.mirror_loss = mean_mirror / n
        if self.smooth_loss_coef > 0.0:
            self.smooth_loss = mean_smooth / n
        return mean_value_loss / n, mean_surrogate_loss / n

    # ---- symmetry augmentation ---------------------------------------------------------------------------------
    # A mini-batch of B rows becomes 2 B rows: the originals, then their mirror images.  Observations, actions and the old mean go through their tables; the old std is
    # permuted (a magnitude: never negated); old values, advantages and returns are copied, and so is the old log-probability: that of a mirrored action under the mirrored
    # old mean and the permuted std is the original's.  Everything behind the batch (losses, KL -> learning rate, clip, Adam) runs unchanged on 2 B rows; which formulation
    # a mini-batch takes is decided by the modules as before, never by the row count: a kernel that refuses 2 B rows fails its call, and that raises.
    def _symmetry_tables(self, symmetry):
        """-> utils/symmetry.py:MirrorTables, or None (off)"""
        if symmetry is None or symmetry is False:
            return None
        if symmetry is True or not all(hasattr(symmetry, k) for k in ("obs", "privileged_obs", "action", "action_std")):
            raise ValueError("PPO(symmetry=...) takes the task's mirror tables, utils.symmetry.mirror_tables(env_cfg) (the runner builds them for algorithm.symmetry = True), "
                             "got %r" % (symmetry,))
        return symmetry

    def _sym_table(self, key):
        """the (perm, sign) numpy table of the rows of _KEYS entry `key`, None for rows that are copied"""
        s = self._sym
        cobs = s.privileged_obs if (self.storage is None or self.storage.privileged_observations is not None) else s.obs
        return {"obs": s.obs, "cobs": cobs, "act": s.action, "mu": s.action, "sig": s.action_std}.get(key)

    def _sym_tensors(self, dev):
        """the tables as torch tensors (int64 perm, float32 sign) per _KEYS entry, made once"""
        if self._sym_t is None:
            self._sym_t = {k: (torch.as_tensor(self._sym_table(k)[0].astype("int64"), device=dev), torch.as_tensor(self._sym_table(k)[1], device=dev)) for k in ("obs", "cobs", "act", "mu", "sig")}
        return self._sym_t

    def _sym_batch(self, batch):
        """The eager formulation (torch indexing), the numerical yardstick of the kernel path: batch of mini_batch_generator -> the same tuple at twice the rows"""
        tabs = self._sym_tensors(batch[0].device)
        out = []
        for k, x in zip(self._KEYS, batch[:9]):
            tab = tabs.get(k)
            mirror = x if tab is None else x[:, tab[0]] if k == "sig" else x[:, tab[0]] * tab[1]
            out.append(torch.cat([x, mirror]))
        return tuple(out) + tuple(batch[9:])

    def _nn_library(self, required="symmetry augmentation in graph mode runs go2nn_mirror_rows"):
        """the policy-side library: the one the tests handed in, else the device library on a GPU — missing there is an error, there is no quiet torch fallback.  On the
        CPU with none handed in: raises with `required` as the reason, or -> None when `required` is None (the caller has a torch formulation)"""
        if self.nn_lib is not None:
            return self.nn_lib
        if not str(self.device).startswith("cuda"):
            if required is None:
                return None
            raise RuntimeError("%s: on the CPU hand in the host build (nn_lib), or use the eager mode" % required)
        from ... import _nn
        return _nn.load_nn()

    def _sym_setup(self, nmb, mb):
        """Graph mode: the augmented mini-batches self._aug[k] [nmb, 2 mb, ...] and the ONE go2nn_mirror_rows call that fills them from the permuted rollout self._perm —
        it runs inside the captured permutation step, behind the gather.  The tables are uploaded once, here."""
        from ... import _nn
        lib = self._nn_library()
        self._aug = {k: torch.empty((nmb, 2 * mb) + tuple(v.shape[1:]), device=self.device, dtype=v.dtype) for k, v in self._perm.items()}
        tabs = {k: _nn.mirror_table_tensors(lib, self._sym_table(k), self.device) for k in ("obs", "cobs", "act", "mu", "sig")}
        self._sym_dev = tabs          # (kept alive: the captured launch reads them)
        self._mirror_jobs = _nn.mirror_jobs([(self._perm[k], self._aug[k], tabs.get(k)) for k in self._KEYS])
        return lambda: _nn.mirror_rows(lib, self._mirror_jobs, nmb, mb, self._stream(self._acc))

    # ---- mirror loss -------------------------------------------------------------------------------------------
    # Augmentation shows the network both images; this term (`mirror_loss_coef` > 0, needs `symmetry`) penalises the gap between its two answers.  Rows r and B + r of an
    # augmented mini-batch are o and M_o o, so with the action table (perm, sign)
    #     e[r, j] = mu[r, j] - sign[j] mu[B + r, perm[j]],        L_mirror = coef mean(e^2)
    # costs no forward pass, and L_mirror / coef is what scripts/evaluate.py --asymmetry reports as equivariance_rmse^2, on the update's rows.  Both rows receive gradient:
    # upstream rsl_rl detaches the mirrored side.  Eager mode: the torch expression below, the numerical yardstick.  Graph mode on the heads path:
    # go2nn_mirror_loss (csrc/go2nn_mirror_loss.h), one launch behind go2nn_ppo_heads.  KL, the learning rate, clipping, Adam and the rank average do not know about it.
    def _mirror_error(self, mu_b):
        B = mu_b.shape[0] // 2
        perm, sign = self._sym_tensors(mu_b.device)["act"]
        return mu_b[:B] - mu_b[B:][:, perm] * sign

    def _mirror_term(self, mu_b):
        """-> the weighted term of the loss (under autograd); self._ml = L_mirror / coef of this mini-batch"""
        ms = self._mirror_error(mu_b).square().mean()
        self._ml = ms.detach()
        return self.mirror_loss_coef * ms

    def _mirror_grad(self, mu_b):
        """-> d L_mirror / d mu [2 B, A] as a torch expression, for the branch that seeds autograd with the loss kernel's gradients; self._ml as _mirror_term"""
        with torch.no_grad():
            B, A = mu_b.shape[0] // 2, mu_b.shape[1]
            perm, sign = self._sym_tensors(mu_b.device)["act"]
            e = self._mirror_error(mu_b)
            self._ml = e.square().mean()
            g = (2.0 * self.mirror_loss_coef / (B * A)) * e
            return torch.cat([g, -(g * sign)[:, perm]])          # (row B + r, column perm[j]: -sign[j] g[r, j])

    def _mirror_kernel_args(self):
        """-> (coef, perm int16 tensor, sign tensor) of go2nn_mirror_loss: the action table checked (an involution, sign[perm[j]] == sign[j]) and uploaded once"""
        if self._ml_dev is None:
            from ... import _nn
            self._ml_dev = _nn.mirror_loss_table_tensors(self._nn_library(), self._sym_table("act"), self.device)
        return (self.mirror_loss_coef,) + tuple(self._ml_dev)

    # ---- smoothness loss ---------------------------------------------------------------------------------------
    # The temporal half of CAPS on the policy's action mean (`smooth_loss_coef` > 0).  The update's mini-batches then are ENV BLOCKS — all T steps of a slice of the
    # permuted environments, time-major: row t n + j (under symmetry augmentation followed by the mirror images' block) — instead of random rows, so rows (t, j) and
    # (t + 1, j) are both ordinary PPO samples of the mini-batch and the actor's forward has already produced both answers: with w[t, j] = (dones[t, env j] == 0)
    #     e[b, t, j, :] = w[t, j] (mu[b, t, j, :] - mu[b, t + 1, j, :])   (t < T - 1),        L_smooth = coef mean(e^2)   (masked pairs count as 0: a fixed denominator)
    # costs no forward pass.  Both rows of a pair receive gradient, nothing is detached.  Eager mode: the torch expression below, the numerical
    # yardstick.  Graph mode on the heads path: go2nn_smooth_loss (csrc/go2nn_smooth_loss.h), one launch behind go2nn_ppo_heads (and go2nn_mirror_loss); the mini-batch
    # order and the weights come from go2nn_smooth_indices inside the captured permutation step.  KL, the learning rate, clipping, Adam and the rank average do not
    # know about it.
    def _smooth_shape(self, rows):
        """-> (blocks, T, n) of a mini-batch of `rows` rows whose pair weights are self._sw [T n]"""
        T = self.storage.num_transitions_per_env
        n = self._sw.numel() // T
        blocks = rows // (T * n)
        if blocks * T * n != rows or blocks not in (1, 2):
            raise ValueError("smoothness loss: %d rows are not 1 or 2 blocks of %d steps x %d envs" % (rows, T, n))
        return blocks, T, n

    def _smooth_error(self, mu_b):
        blocks, T, n = self._smooth_shape(mu_b.shape[0])
        m = mu_b.view(blocks, T, n, mu_b.shape[1])
        return (m[:, :-1] - m[:, 1:]) * self._sw.view(1, T, n, 1)[:, :-1].to(mu_b.dtype)

    def _smooth_term(self, mu_b):
        """-> the weighted term of the loss (under autograd); self._sl = L_smooth / coef of this mini-batch"""
        ms = self._smooth_error(mu_b).square().mean()          # (over blocks (T - 1) n A elements, masked pairs included)
        self._sl = ms.detach()
        return self.smooth_loss_coef * ms

    def _smooth_grad(self, mu_b):
        """-> d L_smooth / d mu [blocks T n, A] as a torch expression, for the branch that seeds autograd with the loss kernel's gradients; self._sl as _smooth_term"""
        with torch.no_grad():
            e = self._smooth_error(mu_b)
            self._sl = e.square().mean()
            ge = (2.0 * self.smooth_loss_coef / e.numel()) * e
            g = torch.zeros((e.shape[0], e.shape[1] + 1) + tuple(e.shape[2:]), dtype=mu_b.dtype, device=mu_b.device)
            g[:, :-1] += ge          # row t: + e[t]
            g[:, 1:] -= ge           # row t + 1: - e[t]
            return g.view_as(mu_b)

    def _smooth_order(self, nmb):
        """Graph mode, inside the captured permutation step: the env-block index list of the update into self._sidx (what go2sim_shuffle_gather / index_select take) and
        the pair weights into self._sw_all [nmb, T n].  ONE go2nn_smooth_indices call (the keyed bijection over the environments; its second launch advances the counter,
        so a replayed graph draws a new permutation every time); with torch.randperm patched (the tests' hook) or no policy-side library: the same lists with torch ops
        from torch.randperm(N), as the eager generator builds them."""
        st = self.storage
        T, N = st.num_transitions_per_env, st.num_envs
        n = N // nmb
        lib = None if torch.randperm is not _RANDPERM else self._nn_library(required=None)
        if lib is None:
            idx, w = st.env_block_indices(nmb, torch.randperm(N, requires_grad=False, device=self.device))
            self._sidx.copy_(idx.reshape(-1))
            self._sw_all.copy_(w.reshape(nmb, T * n))
            return self._sidx
        if self._shuffle_key is None:
            self._make_shuffle_key()
        p = lambda t: t.data_ptr()
        if lib.go2nn_smooth_indices(p(self._sidx), p(self._sw_all), p(st.dones), nmb, T, N, p(self._shuffle_key), self._stream(self._acc)) != 0:
            raise RuntimeError("go2nn_smooth_indices: %s" % lib.go2nn_last_error().decode())
        return self._sidx

    def _smooth_kernel_args(self, i, rows):
        """-> (coef, pair weights uint8 [T n] of mini-batch i, blocks, T, n) of go2nn_smooth_loss"""
        self._sw = self._sw_all[i]
        return (self.smooth_loss_coef, self._sw) + self._smooth_shape(rows)

    # ---- graph mode -------------------------------------------------------------------------------------------
    _KEYS = ("obs", "cobs", "act", "val", "adv", "ret", "logp", "mu", "sig")

    def _graph_batch(self, i):
        """-> the nine tensors of mini-batch i in _KEYS order.  Mini-batch i is the i-th contiguous chunk of the rollout permuted ONCE per update (the reference reuses
        one permutation for all epochs, rollout_storage.py:150): 4 chunk gathers per iteration instead of 20 mini-batch gathers.  A recurrent policy: the i-th fixed
        env slice, all T steps, its memories' outputs in place of the observations."""
        if self._rnn:
            batch = self._rnn_fixed[i]
            return list(self._rnn_heads_inputs(batch)) + [t.reshape(-1, t.shape[-1]) for t in batch[2:9]]
        if self._aug is not None:          # symmetry: chunk i of the permuted rollout followed by its mirror image (go2nn_mirror_rows, once per update)
            return [self._aug[k][i] for k in self._KEYS]
        mb = self._mb
        return [self._perm[k][i * mb:(i + 1) * mb] for k in self._KEYS]

    def _graph_front(self, i, split=False):
        """Forward, losses, backward of mini-batch i with every decision on the device (same arithmetic as _update_eager).  split: the gradients and the mean
        KL are packed into the all-reduce bucket (more than one rank)."""
        batch = self._graph_batch(i)
        ac = self.actor_critic
        if self.fused_loss and type(ac) is _AC and self._heads_path(batch):
            # a plain ActorCritic: forward, loss and backward of the mini-batch as explicit launches, no autograd graph (modules/fused.py:ppo_pair_grads):
            # grouped hidden layers, go2nn_ppo_heads (heads forward + loss + heads backward in one pass), ONE go2nn_sum_rows; .grad of every parameter is set
            from ..modules import fused
            self.optimizer.zero_grad(set_to_none=True)
            mirror = self._mirror_kernel_args() if self.mirror_loss_coef > 0.0 else None          # (go2nn_mirror_loss behind go2nn_ppo_heads; its weighted loss is added to acc[2])
            smooth = self._smooth_kernel_args(i, batch[0].shape[0]) if self.smooth_loss_coef > 0.0 else None          # (go2nn_smooth_loss behind both; its weighted loss: the last slot of acc)
            stats = fused.ppo_pair_grads(ac, batch[0], batch[1], batch[2], batch[3], batch[4], batch[5], batch[6], batch[7], batch[8], self.clip_param, self.value_loss_coef,
                                         self.entropy_coef, self.use_clipped_value_loss, acc=self._acc, mirror=mirror, diag=self._diag, smooth=smooth)          # (the running loss sums: added by the pass's go2nn_sum_rows launch)
            kl_mean = stats[2]
        elif self.fused_loss:
            # the loss kernel already holds d loss / d (mu, std, value): seed the backward pass of the two networks with them directly
            # (loss.backward() through the autograd.Function costs a clone and three multiplications by the unit upstream gradient)
            mu_b, val_b = ac.actor(batch[0]), self._value(batch[1])
            stats, gmu, gstd, gval = _FusedPPOLoss.kernel(self, mu_b, ac.std, val_b, *batch[2:])
            self._diag_torch(mu_b, ac.std, val_b, *batch[2:])
            self.optimizer.zero_grad(set_to_none=True)
            if self.smooth_loss_coef > 0.0:       # the regularisers' gradients join the kernel's; acc = [surrogate, value loss(, L_mirror), L_smooth]
                self._sw = self._sw_all[i]
                extra = []
                if self.mirror_loss_coef > 0.0:
                    gmu = gmu + self._mirror_grad(mu_b)
                    extra.append(self.mirror_loss_coef * self._ml.reshape(1))
                gmu = gmu + self._smooth_grad(mu_b)
                self._acc.add_(torch.cat([stats[:2]] + extra + [self.smooth_loss_coef * self._sl.reshape(1)]))
            elif self.mirror_loss_coef > 0.0:       # the mirror term's gradient joins the kernel's; acc = [surrogate, value loss, L_mirror]
                gmu = gmu + self._mirror_grad(mu_b)
                self._acc.add_(torch.cat([stats[:2], self.mirror_loss_coef * self._ml.reshape(1)]))
            else:
                self._acc.add_(stats[:2])         # [surrogate, value loss]; read back swapped in _update_graphs (issued before the backward pass: off its tail)
            # std a leaf: the kernel's gradient IS its .grad (autograd would copy it there with one more launch).  The recurrent update has always left that copy to
            # autograd; its captured graph keeps that launch.
            if ac.std.requires_grad and ac.std.grad_fn is None and not self._rnn:
                ac.std.grad = gstd.view_as(ac.std)
                torch.autograd.backward([mu_b, val_b], [gmu, gval])
            else:
                torch.autograd.backward([mu_b, ac.std, val_b], [gmu, gstd.view_as(ac.std), gval])
            kl_mean = stats[2]
        else:
            if self.smooth_loss_coef > 0.0:
                self._sw = self._sw_all[i]
            loss, value_loss, surrogate_loss, kl_mean = self._losses(*batch)
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            self._acc.add_(torch.stack([surrogate_loss.detach(), value_loss.detach()] + ([self.mirror_loss_coef * self._ml] if self.mirror_loss_coef > 0.0 else [])
                                       + ([self.smooth_loss_coef * self._sl] if self.smooth_loss_coef > 0.0 else [])))
        if split:
            if self._bucket is None:
                self._bucket = GradBucket(self._params, 1 if self._adaptive() else 0)
            self._bucket.pack(kl_mean)
        else:
            self._kl = kl_mean

    def _heads_path(self, batch):
        if self.surrogate_split:
            return False
        from ..modules import fused
        return fused.ppo_pair_applicable(self.actor_critic, batch[0], batch[1])

    def _graph_back(self, split=False):
        """LR decision, gradient clipping, Adam.  split: on the all-reduced bucket (shard-mean gradients and KL: every rank takes the
        same LR branch); otherwise on this rank's gradients."""
        self._clip_adam(self.optimizer, self._params, self._bucket.unpack(_world()) if split else self._kl)

    def _graph_step(self, i):
        self._graph_front(i)
        self._graph_back()

    def _update_graphs(self):
        st = self.storage
        nmb, mb = self.num_mini_batches, (st.num_envs * st.num_transitions_per_env) // self.num_mini_batches
        if self._graph is None:
            flat = lambda t: t.flatten(0, 1)
            self._flat = {"obs": flat(st.observations), "cobs": flat(st.privileged_observations) if st.privileged_observations is not None else flat(st.observations),
                          "act": flat(st.actions), "val": flat(st.values), "ret": flat(st.returns), "logp": flat(st.actions_log_prob), "adv": flat(st.advantages),
                          "mu": flat(st.mu), "sig": flat(st.sigma)}
            self._mb = mb
            self._perm = {k: torch.empty((nmb * mb,) + tuple(v.shape[1:]), device=self.device, dtype=v.dtype) for k, v in self._flat.items()}
            smooth = self.smooth_loss_coef > 0.0
            # [surrogate, value loss(, the weighted mirror loss)(, the weighted smoothness loss)]
            self._acc = torch.zeros(2 + (self.mirror_loss_coef > 0.0) + smooth, device=self.device)
            if smooth:          # (init_storage has checked that the mini-batches are whole environments: nmb * mb = T N)
                self._sidx = torch.empty(nmb * mb, dtype=torch.int64, device=self.device)
                self._sw_all = torch.zeros(nmb, mb, dtype=torch.uint8, device=self.device)
            self._bucket = None
            mirror =self._sym_setup(nmb, mb) if self._sym is not None else None
            if _collectives_on():
                self._graph = self._reduced_steps(self._graph_front, self._graph_back, (lambda: self._bucket), "PPO mini-batch")
            else:
                self._graph = self._whole_update_step(self._graph_step, "PPO update")
            self._graph_reps = self.num_learning_epochs if _collectives_on() else 1
            # ONE permutation for the whole update, reused by every epoch, as in the reference (rollout_storage.py:150), and the nine storage tensors gathered
            # into mini-batch order: ONE launch (go2sim_shuffle_gather: a keyed sort-free shuffle computed per output row + all gathers + the loss accumulators'
            # reset) instead of torch.randperm's 12-kernel radix sort, 9 index_select launches and the fills between them (~0.36 ms of launch chain per update)
            from ..._abi import Go2GatherJob
            keys = self._KEYS
            use_lib = self.lib is not None and hasattr(self.lib, "go2sim_shuffle_gather") and all(self._flat[k].dtype == torch.float32 and self._flat[k].is_contiguous() for k in keys)
            if use_lib:
                row = lambda t: int(t[0].numel()) if t.dim() > 1 else 1
                self._gather_jobs = (Go2GatherJob * len(keys))(*[Go2GatherJob(self._flat[k].data_ptr(), self._perm[k].data_ptr(), row(self._flat[k]), 0) for k in keys])
                self._make_shuffle_key()
            rows = nmb * mb

            def gather():
                if not use_lib:
                    self._acc.zero_()
                    indices = self._smooth_order(nmb) if smooth else torch.randperm(rows, requires_grad=False, device=self.device)
                    for k in self._KEYS:
                        torch.index_select(self._flat[k], 0, indices, out=self._perm[k])
                    return
                idx = None
                if smooth:          # env blocks: the index list comes from go2nn_smooth_indices, in front of the gather in the same captured step
                    idx = self._smooth_order(nmb)
                elif torch.randperm is not _RANDPERM:
                    idx = torch.randperm(rows, requires_grad=False, device=self.device).to(torch.int64).contiguous()
                p = self._ptr
                self._call("go2sim_shuffle_gather", self._gather_jobs, len(keys), rows, p(idx), p(self._shuffle_key), p(self._acc), int(self._acc.numel()), self._stream(self._acc))

            def permute():
                gather()
                if mirror is not None:          # symmetry: the one go2nn_mirror_rows launch, in the same captured step
                    mirror()
            self._permute = CapturedStep(permute, enabled=self._capture, warmup=2, name="PPO rollout permutation", optional=True)
        self._permute()
        for _ in range(self._graph_reps):
            for g in self._graph:
                g()
        self._obs_norm_finish()          # (enqueued behind the last optimizer step and in front of the read-back's host synchronisation: no idle gap in front of it)
        self._vn_finish()
        surrogate, value, *rest = self._read_back(self._acc, self.num_learning_epochs * nmb)
        if self.mirror_loss_coef > 0.0:
            self.mirror_loss = rest.pop(0) / self.mirror_loss_coef
        if self.smooth_loss_coef > 0.0:
            self.smooth_loss = rest.pop(0) / self.smooth_loss_coef
        return value, surrogate

    def graphs_captured(self):
        """True iff every mini-batch step of the update is being replayed from a HIP graph (bench.py reports it and refuses to quote a
        number from a silently degraded run)."""
        # (the permutation step is a CapturedStep too — `optional`, a failed capture keeps it eager even under GO2_STRICT_GRAPHS — and counts here: a run
        #  whose update replays but whose permutation fell back to ten eager launches does not report "update": true)
        head = getattr(self, "_permute", None)
        return bool(self.use_graphs and self._capture and all_captured(self._graph) and (head is None or head.calls == 0 or head.graph is not None))

    def update(self):
        self.parameters_changed()          # the optimizer steps below change the parameters: the next rollout re-packs
        self._on_merged = False
        self._vn_merged = False
        if self._diag is not None:
            self._diag.begin()          # the slot cursors: zeroed once per update, in front of its first step
        if self._rnn and self.use_graphs and self._rnn_memory() is not None:
            out = self._rnn_update_graphs()
        elif self.use_graphs and not self._rnn:
            out = self._update_graphs()
        else:
            out = self._update_eager()
        self._obs_norm_finish()
        self._vn_finish()
        self._diag_finish()
        self.storage.clear()
        return out

    # ---- observation normalisation -----------------------------------------------------------------------------
    # Statistics k serve the rollout AND the update of iteration k — upstream updates them before every forward —, so old_log_prob, mu, sigma and
    # values in the storage are what the update's forward computes from the stored rows, no host state enters the captured graphs, and a run is deterministic.  The
    # storage holds NORMALISED rows; the raw moments of the rollout (sums of x - mean32 and of its square, fp64, one table row per step and 64 storage rows) are merged
    # into the state by one go2nn_obs_norm_update launch per stream at the end of update(), a plain launch behind the captured update.  With fused_rollout off, or no
    # library, modules/normalizer.py does the same job in torch (forward / merge on a kept copy of the raw rows): the numerical yardstick.
    def _obs_norm(self):
        """-> (actor stream's normaliser, critic stream's or None: one normaliser for the shared rows), or None (off)"""
        ac = self.actor_critic
        na = getattr(ac, "obs_normalizer", None)
        if na is None:
            return None
        nc = getattr(ac, "critic_obs_normalizer", None)
        if self._on_state is None or self._on_state["norms"] != (id(na), id(nc)):
            if self._sym is not None or self.mirror_loss_coef > 0.0:
                raise NotImplementedError("empirical observation normalisation with symmetry augmentation or the mirror loss is not implemented (the mirror image of a "
                                          "normalised row is the normalised mirror image only under symmetrised statistics)")
            if self._rnn:
                raise NotImplementedError("empirical observation normalisation with a recurrent policy is not implemented (the hidden state that crosses an iteration "
                                          "boundary was computed under the old statistics)")
            if _world() > 1 or _collectives_on():
                raise NotImplementedError("empirical observation normalisation trains on one rank only (the moments would need an fp64 all-reduce)")
            self._on_state = {"norms": (id(na), id(nc))}
        return na, nc

    def normalizers_changed(self):
        """the normalisers' eps / clip may have changed (a checkpoint was loaded): the job arrays, which hold the clip by value, are rebuilt at the next step — the caller
        drops the captured rollout with them (the runner does)"""
        if self._on_state is not None:
            self._on_state.pop("storage", None)

    def _obs_norm_setup(self, on):
        """The streams [(normaliser, storage tensor [T, N, D])], and per formulation: the partial tables and the job array of every step (the pointers are fixed: the
        captured rollout bakes one launch per step, the step's table row chosen here on the host), or the raw copies the torch merge reads."""
        st, os_ = self.storage, self._on_state
        if os_.get("storage") is st:
            return os_
        na, nc = on
        if (nc is None) != (st.privileged_observations is None):
            raise ValueError("observation normalisation: the actor-critic has %s normaliser for the privileged observation, the rollout storage %s such rows"
                             % (("no", "has") if nc is None else ("a", "no")))
        streams = [(na, st.observations)] + ([(nc, st.privileged_observations)] if nc is not None else [])
        for n, x in streams:
            if n.num_features != x.shape[-1] or x.dtype != torch.float32 or not x.is_contiguous():
                raise ValueError("observation normalisation: a normaliser of %d columns for contiguous fp32 rows of %d" % (n.num_features, x.shape[-1]))
        T, N = st.num_transitions_per_env, st.num_envs
        lib = self._nn_library(required=None) if self.fused_rollout else None          # (None: the torch formulation)
        os_.update(storage=st, streams=streams, lib=lib)
        if lib is not None:
            from ... import _nn
            rows = int(lib.go2nn_obs_norm_partial_rows(N))
            os_["tables"] = [torch.zeros(T, rows, n.num_features, 2, dtype=torch.float64, device=x.device) for n, x in streams]
            os_["jobs"] = [_nn.obs_norm_jobs([(x[s], x[s], n.mean32, n.inv32, tab[s], n.clip) for (n, x), tab in zip(streams, os_["tables"])]) for s in range(T)]
        else:
            os_["raw"] = [torch.empty_like(x) for _, x in streams]
        return os_

    def _obs_norm_rows(self, on, s):
        """storage row s of both streams, raw -> normalised in place.  -> (actor rows, critic rows) of step s"""
        os_ = self._obs_norm_setup(on)
        if os_["lib"] is not None:
            from ... import _nn
            _nn.obs_norm_apply(os_["lib"], os_["jobs"][s], self.storage.num_envs, self._stream(os_["streams"][0][1]))
        else:
            for (n, x), raw in zip(os_["streams"], os_["raw"]):
                raw[s].copy_(x[s])
                x[s].copy_(n(raw[s]))
        rows = [x[s] for _, x in os_["streams"]]
        return rows[0], rows[-1]

    def _obs_norm_last(self, on, x):
        """the bootstrap value's observation (raw, no storage row) -> normalised, in a scratch buffer"""
        os_ = self._obs_norm_setup(on)
        n = os_["streams"][-1][0]
        if os_["lib"] is None or not (x.is_contiguous() and x.dtype == torch.float32):
            return n(x)
        from ... import _nn
        if os_.get("last") is None or os_["last"].shape != x.shape or os_["last"].device != x.device:
            os_["last"] = torch.empty_like(x)
        os_["last_jobs"] = _nn.obs_norm_jobs([(x, os_["last"], n.mean32, n.inv32, None, n.clip)])
        _nn.obs_norm_apply(os_["lib"], os_["last_jobs"], x.shape[0], self._stream(x))
        return os_["last"]

    def _obs_norm_finish(self):
        """once per update(), after its last optimizer step: the rollout and the update of this iteration both ran on the statistics the iteration began with"""
        on = self._obs_norm()
        if on is not None and not self._on_merged:
            self._on_merged = True
            self._obs_norm_merge(on)

    def _obs_norm_merge(self, on):
        """the rollout's raw moments into the statistics (the `until` cap is the host's decision: count grows by N T per iteration, no device read)"""
        os_ = self._obs_norm_setup(on)
        st = self.storage
        samples = st.num_envs * st.num_transitions_per_env
        for i, (n, x) in enumerate(os_["streams"]):
            if not n.accepts():
                continue
            if os_["lib"] is not None:
                from ... import _nn
                _nn.obs_norm_update(os_["lib"], os_["tables"][i], n.state, samples, n.eps, n.mean32, n.inv32, self._stream(x))
                n.note_merged(samples)
            else:
                n.merge(os_["raw"][i].flatten(0, 1))

    # ------------------------------------------------------------------ recurrent policies (the reference's is_recurrent branches)
    # Rollout: the memories' step (the state before it into storage slot s), then the heads as for a feed-forward policy (go2nn_policy_act on the memories' h);
    # process_env_step zeroes the done rows; compute_returns advances the critic memory one more step on the last observations, as the reference's evaluate() does.
    # Update: contiguous env slices, all T steps, no shuffling, the same order every epoch (rollout_storage.py:186-234).  On the library's kernels the memory runs at
    # fixed shapes (modules/fused_rnn.py) and the whole update is one HIP graph; the reference formulation (GO2_FUSED_MLP=0, the CPU) is nn.LSTM / nn.GRU over the
    # padded episode segments of storage.reccurent_mini_batch_generator.
    def _rnn_memory(self):
        """-> modules/fused_rnn.py:RolloutMemory when the library's kernels are in use, else None (the torch formulation)"""
        from ..modules import fused_rnn
        if not fused_rnn.available():
            return None
        if self._rm is None:
            self._rm = fused_rnn.RolloutMemory(self.actor_critic)
        return self._rm

    def _rnn_step(self, obs, critic_obs, s):
        """-> the memories' outputs (h_a, h_c) of rollout step s; the states before it go into storage slot s"""
        st, ac = self.storage, self.actor_critic
        rm = self._rnn_memory()
        if rm is not None:
            if s == 0:
                rm.images()            # the split weight images: once per rollout (inside the captured rollout too)
            return rm.step([obs.contiguous(), critic_obs.contiguous()], slots=[(st.saved_hidden_states_a, s), (st.saved_hidden_states_c, s)])
        for mem, saved in ((ac.memory_a, st.saved_hidden_states_a), (ac.memory_c, st.saved_hidden_states_c)):
            for dst, src in zip(saved, mem.states()):
                dst[s].copy_(src)
        return ac.memory_a(obs).squeeze(0), ac.memory_c(critic_obs).squeeze(0)

    def _rnn_batches(self):
        if self._rnn_memory() is not None:
            fixed = self.storage.recurrent_fixed_batches(self.num_mini_batches)
            return (b for _ in range(self.num_learning_epochs) for b in fixed)
        return self.storage.reccurent_mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)

    def _rnn_heads_inputs(self, batch):
        """-> (actor memory output, critic memory output) [T * B, H] of a mini-batch of either generator"""
        ac = self.actor_critic
        obs, cobs, (hid_a, hid_c), masks = batch[0], batch[1], batch[9], batch[10]
        if self._rnn_memory() is not None:
            from ..modules import fused_rnn
            ya, yc = fused_rnn.memory_sequence(ac.memory_a, obs, hid_a, masks), fused_rnn.memory_sequence(ac.memory_c, cobs, hid_c, masks)
        else:
            ya, yc = ac.memory_a(obs, masks, hid_a), ac.memory_c(cobs, masks, hid_c)
        return ya.reshape(-1, ya.shape[-1]), yc.reshape(-1, yc.shape[-1])

    def _rnn_losses(self, batch):
        ya, yc = self._rnn_heads_inputs(batch)
        flat = lambda t: t.reshape(-1, t.shape[-1])
        return self._losses(ya, yc, *[flat(t) for t in batch[2:9]])

    def _rnn_update_graphs(self):
        """the whole update (every epoch's mini-batch steps on fixed env slices of the rollout: no permutation) as ONE HIP graph after one eager update; the
        learning-rate decision on the device, one host read per update"""
        if self._graph is None:
            self._rnn_fixed = self.storage.recurrent_fixed_batches(self.num_mini_batches)
            self._acc = torch.zeros(2, device=self.device)
            self._graph = self._whole_update_step(self._graph_step, "recurrent PPO update")
        self._acc.zero_()
        self._graph[0]()
        surrogate, value = self._read_back(self._acc, self.num_learning_epochs * self.num_mini_batches)
        return value, surrogate
