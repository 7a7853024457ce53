"""What PPO (ppo.py) and CTS (cts.py, moe_cts.py) share: the execution modes and their Adam construction, the eager PPO loss terms and optimizer step, the graph
mode's optimizer tail and step lists, the per-step rollout bookkeeping and heads, and the calls into the library."""
import ctypes as C
import os

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.optim as optim

from ..modules.actor_critic import ActorCritic as _AC
from ..modules.actor_critic_cts import ActorCriticCTS as _ACC
from ._graph import CapturedStep, FusedClipAdam, ReducedStep


_ADAM_IMPL = {"fused": True}          # torch's capturable Adam where the library's clip + Adam kernel does not serve (GO2_FUSED_ADAM=0, a variant it does not cover)

_RANDPERM = torch.randperm          # (the golden tests replace torch.randperm to replay the reference's permutation: then the update takes that one)

_PLAIN = (_AC._noise, _ACC._noise)          # the modules' own _noise functions as they are at import (the tests replace them to inject the reference's draws: then the rollout asks per step)


def _world():
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def _collectives_on():
    """True when the cross-rank averaging must run: more than one rank, or GO2_FORCE_COLLECTIVES=1 with an initialised process
    group of any size (lets a 1-GPU box exercise the RCCL-inside-HIP-graph path)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("GO2_FORCE_COLLECTIVES", "0") == "1"


def allreduce_mean_bucket(grads, world, extra=None):
    parts = [g.reshape(-1) for g in grads] + ([extra.detach().reshape(1)] if extra is not None else [])
    flat = torch.cat(parts)
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat /= world
    views, off = [], 0
    for g in grads:
        n = g.numel(); views.append(flat[off:off + n].view_as(g)); off += n
    torch._foreach_copy_(grads, views)           # one multi-tensor launch instead of one copy per parameter
    return flat[off] if extra is not None else None


class _RolloutHeads:
    """Shared pieces of the PPO-family algorithms.  A subclass sets device, lib, storage, transition and the hyper-parameters (clip_param, gamma, ...)."""
    _eps_all = None
    surrogate_split = 0         # rows [0, surrogate_split) of a mini-batch take a surrogate mean of their own, the rest another (CTS: the teacher rows); 0: one mean over all rows
    _img_cache = None           # split weight images of the networks a rollout evaluates as torch modules on the library's kernels (modules/fused.py:own_forward(images=...)); emptied with _pk_packed
    _pk = None                  # the fused policy kernel of the rollout: None = not looked for yet, False = not applicable, else the kernel (_policy_kernel() of the subclass decides)
    _pk_packed = False          # the policy kernel's packed weights are those of the current parameters (they change in update() and when a checkpoint is loaded)
    _pk_recorded = False        # the rollout last RUN THROUGH PYTHON (eager, or while being captured) packed at its first step: what a replay of that capture does too
    _vn = None                  # value normalisation (modules/normalizer.py:ValueNormalization) when `algorithm.normalize_value` is on; None: nothing is loaded, allocated or launched
    _vn_state = None            # its formulation and buffers, made at the first compute_returns (_vn_setup)
    _vn_merged = True           # this update has merged its rollout's moments (update() clears it: a replayed compute_returns graph never passes through Python)
    return_stats = None         # (mean, std) of the raw returns as the last update left them: Train/return_mean, Train/return_std
    _diag = None                # the update's diagnostics (_diag.py:UpdateDiagnostics) when `algorithm.diagnostics` is on; None: nothing is loaded, allocated or launched

    # ------------------------------------------------------------------ construction
    def _init_modes(self, device, lib, learning_rate, use_graphs, fused_loss, fused_rollout):
        """The execution mode: eager — the reference's control flow; graphs — every decision of the update on the device, the learning rate in a device tensor (_lr_t),
        the steps captured into HIP graphs (on a GPU).  -> on a GPU?"""
        self.device, self.lib = device, lib
        on_gpu = str(device).startswith("cuda")
        self.use_graphs = on_gpu if use_graphs is None else bool(use_graphs and on_gpu)
        self._capture = self.use_graphs and use_graphs != "uncaptured"
        if use_graphs == "uncaptured":     # the graph-mode update (device-side LR decision, permuted chunks, split all-reduce) run eagerly on any
            self.use_graphs = True         # device: how the CPU tests cover it
        self._lr_t = torch.tensor(float(learning_rate), device=device) if self.use_graphs else None
        # the fused loss kernel is the default on the GPU; on the CPU it is opt-in (tests compare it with the eager formulation)
        self.fused_loss = (on_gpu and lib is not None) if fused_loss is None else bool(fused_loss and lib is not None)
        self.fused_rollout = (on_gpu and lib is not None) if fused_rollout is None else bool(fused_rollout and lib is not None)
        if on_gpu and lib is not None and os.environ.get("GO2_FUSED_MLP", "1") == "1":
            from ..modules import fused
            fused.set_library(lib)         # Linear->ELU pairs: activation + bias gradients in one HBM pass (go2sim_elu_backward_bias), ELU in place
                                           # (+6 % whole-job, measured; GO2_FUSED_MLP=0 restores plain autograd)
        self._clip_adams = {}              # optimizer -> its FusedClipAdam (_clip_adam)
        return on_gpu

    # ------------------------------------------------------------------ the update's diagnostics (_diag.py; off: every hook below is one `is None` test)
    def _init_diagnostics(self, diagnostics, segments, optimizers):
        """segments: the names of a mini-batch's row segments; optimizers: [(optimizer, prefix of its grad_* keys)]"""
        if not diagnostics:
            return
        from ._diag import UpdateDiagnostics
        self._diag = UpdateDiagnostics(self.device, self.num_learning_epochs, self.num_mini_batches, segments, [name for _, name in optimizers], self.clip_param,
                                       self.max_grad_norm)
        self._diag_opt = {id(o): j for j, (o, _) in enumerate(optimizers)}

    def _diag_lib(self):
        """the policy-side library of the diagnostics' kernels: the one the tests handed in, else the device library on a GPU (missing there is an error); None on the
        CPU with none handed in, where the torch statement of the same sums runs"""
        lib = getattr(self, "nn_lib", None)
        if lib is None and str(self.device).startswith("cuda"):
            from ... import _nn
            lib = _nn.load_nn()
        return lib

    def _diag_torch(self, mu, sigma, value, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b, split=0):
        """a formulation that holds mu and value as tensors states the diagnostics' columns in torch (the argument order of the loss functions)"""
        if self._diag is not None:
            self._diag.record_torch(mu, sigma, value, act_b, old_mu_b, old_sig_b, old_lp_b, adv_b, tv_b, ret_b, split)

    def _diag_finish(self):
        """behind the update's own read-back: the tables come to the host with one more copy"""
        if self._diag is not None:
            self._diag.read()

    @property
    def diagnostics(self):
        """the derived figures of the last update (PPO: one dict; the CTS family: per segment "teacher", "student", and pooled "all"); None with the key off"""
        return None if self._diag is None else self._diag.result

    @property
    def diagnostics_table(self):
        """numpy [steps, segments, GO2NN_DIAG_NUM] of the last update; None with the key off"""
        return None if self._diag is None else self._diag.host_table

    @property
    def diagnostics_grad_sq(self):
        """numpy [steps, optimizers]: the squared gradient norm in front of the clip; None with the key off"""
        return None if self._diag is None else self._diag.host_grad_sq

    # ------------------------------------------------------------------ value normalisation (`algorithm.normalize_value`; off: every hook below is one `is None` test)
    # The critic's output is v^ = (v - mean) / std of the raw GAE returns' running statistics.  The ROLLOUT stores raw values v = v^ std32 + mean32 — the time-out
    # bootstrap, GAE and the advantage normalisation run unchanged in raw units —: the fused policy kernels read a critic whose packed last layer is folded
    # (_nn.py:PackedMlp(fold=...), one go2nn_value_head_fold launch in front of go2nn_pack, once per rollout), the torch formulations state v^ * std32 + mean32
    # (_vn_raw).  BEHIND GAE one go2nn_value_norm_apply launch normalises `values` and `returns` in place and leaves the raw returns' moments: the update reads
    # normalised rows and does not change.  The statistics are frozen inside an iteration; ONE go2nn_value_norm_update launch behind the last optimizer step merges the
    # moments (and, with normalize_value_preserve, rewrites the critic's last layer so that every raw value stays what it was).  The eager mode, a rollout without the
    # library (fused_rollout off) and GO2_FUSED_POLICY=0 state all of it in torch (modules/normalizer.py): the numerical yardstick.  Tests hand in the host build
    # (nn_lib) to run the kernels on the CPU.
    def _init_value_norm(self, net, normalize_value=False, eps=1e-2, until=None, preserve=False):
        """switches value normalisation on when the key is set or the module already has the child `value_normalizer` (a loaded checkpoint brought it)"""
        if not normalize_value and getattr(net, "value_normalizer", None) is None:
            return
        if getattr(net, "is_recurrent", False):
            raise NotImplementedError("algorithm.normalize_value with a recurrent policy is not implemented: its heads live in modules/fused_rnn.py, where the value "
                                      "never passes the sites that denormalise it")
        if _world() > 1 or _collectives_on() or os.environ.get("GO2_FORCE_COLLECTIVES", "0") == "1":
            raise NotImplementedError("algorithm.normalize_value trains on one rank only (the three fp64 moments of the returns would need an all-reduce)")
        from ..modules.normalizer import attach_value_normalizer
        had = getattr(net, "value_normalizer", None) is not None
        vn = attach_value_normalizer(net, 1e-2 if eps is None else eps, until, preserve)
        if had and normalize_value:          # (the child came with a checkpoint: the run's own cap and preservation switch hold, eps travels with the statistics)
            vn.until, vn.preserve = (None if until is None else float(until)), bool(preserve)
        self._vn, self._vn_state, self._vn_merged = vn, None, True
        if vn.preserve:
            self._vn_last_layer()          # (refuses here, not at the first merge)
        # the policy kernel is rebuilt with (or without) the folded critic
        self._pk, self._pk_packed, self._pk_recorded = None, False, False

    def enable_value_norm(self, eps=1e-2, until=None, preserve=False):
        """(runner.load) a checkpoint carries value_normalizer.*: the child is attached and this algorithm continues in normalised units, whatever its config said"""
        if self._vn is None:
            self._init_value_norm(self.actor_critic, True, eps, until, preserve)
        return self._vn

    def value_norm_changed(self):
        """the statistics were loaded: the host's copy of count is re-read (the normaliser does that itself), nothing of an earlier rollout is merged into them"""
        self._vn_merged = True

    def _vn_last_layer(self):
        """-> (weight [1, K], bias [1]) of the critic's last layer, for output preservation"""
        critic = getattr(self.actor_critic, "critic", None)
        lin = [m for m in critic.modules() if isinstance(m, nn.Linear)] if isinstance(critic, nn.Module) else []
        if hasattr(self.actor_critic, "critic_experts") or not lin or lin[-1].out_features != 1 or lin[-1].bias is None:
            raise NotImplementedError("algorithm.normalize_value_preserve needs a critic that ends in ONE scalar Linear layer (%s mixes several value heads)"
                                      % type(self.actor_critic).__name__)
        return lin[-1].weight, lin[-1].bias

    def _vn_library(self):
        """the library of the three launches, or None: the torch statement.  The kernels serve the graph mode on the library's rollout; a handed-in nn_lib (tests: the
        host build) runs them in any mode"""
        if self._vn is None or not self.fused_rollout:
            return None
        lib = getattr(self, "nn_lib", None)
        if lib is None and self.use_graphs and str(self.device).startswith("cuda"):
            from ... import _nn
            lib = _nn.load_nn()          # (missing on a GPU is an error: no quiet torch fallback)
        return lib

    def _vn_fold(self):
        """-> stat32 for the policy kernel's folded critic, or None (off / the torch formulation, which denormalises the kernel's rows itself)"""
        return self._vn.stat32 if self._vn_library() is not None else None

    def _vn_raw(self, v):
        """the torch statement: a normalised value v^ (what the critic module answers) -> the raw value"""
        return v if self._vn is None else self._vn.denormalize(v.detach())

    def _vn_raw_kernel(self, v, pk):
        """a value the policy kernel pk computed on its packed critic: raw already when that critic is folded"""
        return v if (self._vn is None or pk.critic.fold is not None) else self._vn.denormalize(v)

    def _vn_rows_raw(self, pk, s):
        """the policy kernel wrote step s's values into the storage row: raw already when its critic is folded, else denormalised there (torch)"""
        if self._vn is not None and pk.critic.fold is None:
            row = self.storage.values[s]
            row.copy_(self._vn.denormalize(row))

    def _vn_setup(self):
        st, vs = self.storage, self._vn_state
        if vs is not None and vs["storage"] is st:
            return vs
        T, N = st.num_transitions_per_env, st.num_envs
        for t in (st.values, st.returns):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != T * N:
                raise ValueError("value normalisation: contiguous fp32 [T, N, 1] values and returns")
        lib = self._vn_library()
        vs = self._vn_state = {"storage": st, "lib": lib, "n": T * N}
        if lib is not None:
            vs["partials"] = torch.zeros(int(lib.go2nn_value_norm_partial_rows(T * N)), 2, dtype=torch.float64, device=st.returns.device)
        else:
            vs["raw"] = torch.empty_like(st.returns)
        return vs

    def _vn_after_gae(self):
        """behind storage.compute_returns (inside the captured compute_returns graph): values and returns become normalised rows, the raw returns' moments are kept"""
        if self._vn is None:
            return
        vs, st, vn = self._vn_setup(), self.storage, self._vn
        if vs["lib"] is not None:
            from ... import _nn
            _nn.value_norm_apply(vs["lib"], st.values.view(-1), st.returns.view(-1), vn.stat32, vs["partials"], self._stream(st.returns))
        else:
            vs["raw"].copy_(st.returns)
            st.values.copy_(vn.normalize(st.values))
            st.returns.copy_(vn.normalize(st.returns))

    def _vn_finish(self):
        """once per update(), behind its last optimizer step: the rollout and the update of this iteration both ran on the statistics the iteration began with.  The
        `until` cap is the host's decision: count grows by T N per iteration, no device read"""
        vn = self._vn
        if vn is None or self._vn_merged:
            return
        self._vn_merged = True
        vs = self._vn_setup()
        if vn.accepts():
            last = self._vn_last_layer() if vn.preserve else None
            if vs["lib"] is not None:
                from ... import _nn
                _nn.value_norm_update(vs["lib"], vs["partials"], vn.state, vs["n"], vn.eps, vn.stat32, last[0] if last else None, last[1] if last else None,
                                      self._stream(vn.state))
                vn.note_merged(vs["n"])
            else:
                vn.merge(vs["raw"], last)
        if not self.use_graphs:          # (the eager mode reads every loss with .item() already; graph mode: _read_back)
            self.return_stats = tuple(vn.stat32[:2].tolist())

    def _make_adam(self, params, lr=None):
        """Adam over params (or param groups).  lr None: the policy's rate — in graph mode the device tensor the captured steps read and write; any other rate is
        fixed and becomes a device tensor of its own there."""
        if not self.use_graphs:
            return optim.Adam(params, lr=self.learning_rate if lr is None else lr)
        lr = self._lr_t if lr is None else torch.tensor(float(lr), device=self.device)
        return optim.Adam(params, lr=lr, capturable=True, **_ADAM_IMPL) if self._capture else optim.Adam(params, lr=lr, foreach=False)

    def _sync_replicas(self, net):
        if _world() > 1:   # identical initial replicas
            for p in net.parameters():
                dist.broadcast(p.data, src=0)

    def _adaptive(self):
        return self.desired_kl is not None and self.schedule == "adaptive"

    def parameters_changed(self):
        """The networks' parameters are no longer those the rollout's kernels hold packed (update() stepped them, a checkpoint was loaded): the next act() re-packs
        the policy kernel's weights and rebuilds the split weight images."""
        self._pk_packed = False
        self._img_cache = None

    # ------------------------------------------------------------------ calls into the library
    def _ptr(self, t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def _stream(self, t):
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None

    def _call(self, fn_name, *args):
        if getattr(self.lib, fn_name)(*args) != 0:
            raise RuntimeError("%s failed: %s" % (fn_name, self.lib.go2sim_last_error().decode()))

    # ------------------------------------------------------------------ eager update: the reference's formulation
    def ppo_terms(self, lp_b, val_b, mu_b, sig_b, ent_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b, n_t=None):
        """Clipped surrogate, clipped value loss, entropy bonus and the KL to the rollout's policy of one mini-batch (ppo.py:133-176) from the new policy's
        log-probabilities, values, means, sigmas and entropies.  n_t: the surrogate is mean(rows [0, n_t)) + mean(the rest) (cts.py:228-231).
        -> loss, value_loss, surrogate_loss, entropy mean, kl_mean"""
        with torch.no_grad():
            kl = torch.sum(torch.log(sig_b / old_sig_b + 1.0e-5) + (torch.square(old_sig_b) + torch.square(old_mu_b - mu_b)) / (2.0 * torch.square(sig_b)) - 0.5, axis=-1)
            kl_mean = torch.mean(kl)
        ratio = torch.exp(lp_b - torch.squeeze(old_lp_b))
        sur = -torch.squeeze(adv_b) * ratio
        sur_clip = -torch.squeeze(adv_b) * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
        sl = torch.max(sur, sur_clip)
        surrogate_loss = sl.mean() if n_t is None else sl[:n_t].mean() + sl[n_t:].mean()
        if self.use_clipped_value_loss:
            v_clip = tv_b + (val_b - tv_b).clamp(-self.clip_param, self.clip_param)
            value_loss = torch.max((val_b - ret_b).pow(2), (v_clip - ret_b).pow(2)).mean()
        else:
            value_loss = (ret_b - val_b).pow(2).mean()
        ent = ent_b.mean()
        loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * ent
        return loss, value_loss, surrogate_loss, ent, kl_mean

    def _decide_lr_host(self, kl_mean, optimizer):
        """the adaptive-KL learning rate (ppo.py:140-155) decided on the host (a sync on kl_mean) and written into the optimizer's param groups"""
        if kl_mean > self.desired_kl * 2.0:
            self.learning_rate = max(1e-5, self.learning_rate / 1.5)
        elif kl_mean < self.desired_kl / 2.0 and kl_mean > 0.0:
            self.learning_rate = min(1e-2, self.learning_rate * 1.5)
        for g in optimizer.param_groups:
            if torch.is_tensor(g["lr"]):
                g["lr"].fill_(self.learning_rate)
            else:
                g["lr"] = self.learning_rate

    def _eager_step(self, loss, optimizer, params, kl_mean=None):
        """Backward of `loss` and one step of `optimizer` on `params`.  More than one rank: the gradients — and the mean KL riding in the same bucket — are averaged over
        the shards with ONE all-reduce (1.96 MB of fp32, latency-bound on xGMI).  kl_mean given and the schedule adaptive: the learning-rate decision; the reference
        decides before backward (ppo.py:140-155), but the rate is only read by optimizer.step(), so it can wait for the backward pass and share its collective."""
        adaptive = kl_mean is not None and self._adaptive()
        optimizer.zero_grad()
        loss.backward()
        if _collectives_on():
            kl_mean = allreduce_mean_bucket([p.grad for p in params if p.grad is not None], _world(), kl_mean if adaptive else None)
        if adaptive:
            self._decide_lr_host(kl_mean, optimizer)
        total_norm = nn.utils.clip_grad_norm_(params, self.max_grad_norm)
        if self._diag is not None:
            self._diag.grad_from_norm(self._diag_opt[id(optimizer)], total_norm)
        optimizer.step()

    # ------------------------------------------------------------------ graph mode
    def _clip_adam(self, optimizer, params, kl_mean=None):
        """The tail of a graph-mode mini-batch step: [adaptive-KL learning rate from kl_mean, decided on the device;] gradient clipping; Adam — as the library's
        clip + Adam call (_graph.py:FusedClipAdam) where that serves, else as torch launches."""
        adaptive = kl_mean is not None and self._adaptive()
        if self._diag is not None:          # the squared norm the clip is about to see (go2sim_adam_clip_step keeps its own to itself)
            self._diag.grad_sqnorm(self._diag_opt[id(optimizer)], params, self._diag_lib(), self._stream(self._lr_t))
        fa = self._clip_adams.get(optimizer)
        if fa is None:
            fa = self._clip_adams[optimizer] = FusedClipAdam(self.lib, optimizer, params, self.max_grad_norm)
        if fa.usable and fa.step(kl_mean if adaptive else None, self.desired_kl if adaptive else 0.0):
            return
        if adaptive:
            lr = self._lr_t
            up = torch.clamp(lr * 1.5, max=1e-2)
            down = torch.clamp(lr / 1.5, min=1e-5)
            kl_mean = kl_mean.reshape(())
            new_lr = torch.where(kl_mean > self.desired_kl * 2.0, down, torch.where((kl_mean < self.desired_kl / 2.0) & (kl_mean > 0.0), up, lr))
            lr.copy_(new_lr)
        nn.utils.clip_grad_norm_(params, self.max_grad_norm, foreach=True)
        optimizer.step()

    def _whole_update_step(self, fn, name):
        """One rank: every epoch's mini-batch steps fn(0), ..., fn(nmb - 1) — each on its own chunk of the rollout in mini-batch order — as ONE graph.  A graph launch
        costs ≈ 9 µs of idle chip between two mini-batches (profiles/r4_timeline…: Adam step -> next split): from 20 launches per update to 5 (one per epoch) was 15.85 -> 15.76 ms per iteration, then to one.  The first
        update runs eagerly."""
        ne, nmb = self.num_learning_epochs, self.num_mini_batches
        return [CapturedStep((lambda: [fn(i) for _ in range(ne) for i in range(nmb)] and None), enabled=self._capture, warmup=1,
                             name="%s (%d epochs x %d mini-batch steps)" % (name, ne, nmb))]

    def _reduced_steps(self, front, back, bucket, name):
        """More than one rank: per mini-batch slot two captured halves with the gradient all-reduce eager between them (_graph.py).  Slot 0 runs 3 eager steps on a side
        stream first (allocator / lazy initialisation settle; they are real steps of the first update), the others one; then each is captured once and replayed."""
        return [ReducedStep((lambda i=i: front(i, True)), (lambda: back(True)), bucket, enabled=self._capture, warmup=3 if i == 0 else 1, name="%s step %d" % (name, i))
                for i in range(self.num_mini_batches)]

    def _read_back(self, acc, n):
        """ONE device -> host read per update: -> the running sums `acc` over n mini-batch steps as means; the learning rate the device decided becomes learning_rate"""
        vn = self._vn          # (value normalisation: the returns' mean32 / std32 ride in the same read)
        out = torch.cat([acc / n] + ([vn.stat32[:2].to(acc.dtype)] if vn is not None else []) + [self._lr_t.reshape(1)]).tolist()
        self.learning_rate = float(out.pop())
        if vn is not None:
            self.return_stats = (out.pop(-2), out.pop())
        return out

    # The update's permutation in graph mode: a keyed bijection computed on the device (include/go2sim_shuffle.h) under (seed, counter).  The seed follows
    # torch.manual_seed at the time the key is made (the first graph-mode update), NOT torch's generator state afterwards; the counter advances by one per update on the
    # device and is set to the iteration number when a checkpoint is loaded (runner.load -> set_shuffle_counter), so a resumed run does not replay the permutations of
    # iterations 0, 1, ....  DESIGN.md section 8 lists this among the deliberate deviations.
    _shuffle_key = None
    _shuffle_counter0 = 0

    def _make_shuffle_key(self):
        seed = int((torch.initial_seed() * 0x9E3779B1 + 0x7F4A7C15) & 0x7FFFFFFF)          # (follows torch.manual_seed without drawing from the generator)
        self._shuffle_key = torch.tensor([seed, int(self._shuffle_counter0) & 0x7FFFFFFF, 0, 0], dtype=torch.int32, device=self.device)
        return self._shuffle_key

    def set_shuffle_counter(self, it):
        self._shuffle_counter0 = int(it)
        if self._shuffle_key is not None:
            self._shuffle_key[1] = int(it) & 0x7FFFFFFF

    def _pair(self, main_fn, side_fn, enabled=True):
        """-> (main_fn(), side_fn()).  Rounds 2-4 ran side_fn on a second HIP stream; with the grouped launches (PPO, CTS, MoE-CTS never reach this in their updates) the fork
        only served network shapes outside the BASELINE configurations, and two hipBLASLt stream-K kernels side by side were the hang of round 3 that was never
        explained — the second stream is gone."""
        return main_fn(), side_fn()

    # ------------------------------------------------------------------ rollout
    def _kernel(self):
        """-> the fused policy kernel if _policy_kernel() has made one, else None (never looks for it)"""
        return self._pk if self._pk not in (None, False) else None

    def rollout_replayed(self):
        """The runner replayed the captured rollout (act() did not run in Python): the weights are packed iff the captured rollout recorded the pack launch at its
        first step — known from the flag act() left when it ran under capture (a rollout that took the non-kernel branch must not claim packed weights)."""
        self._pk_packed = bool(self._pk_recorded)

    def _begin_step(self):
        """-> the storage slot of the step being collected"""
        s = self.storage.step
        if s >= self.storage.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        return s

    def _store_obs_rows(self, obs, critic_obs, s):
        """Record what env.step() is about to overwrite (the env's buffers are updated in place) — unless the env wrote these rows itself: LeggedRobot.step(rollout=...)"""
        st, t = self.storage, self.transition
        if obs.data_ptr() != st.observations[s].data_ptr():
            st.observations[s].copy_(obs)
        if st.privileged_observations is not None and critic_obs.data_ptr() != st.privileged_observations[s].data_ptr():
            st.privileged_observations[s].copy_(critic_obs)
        t.observations, t.critic_observations = obs, critic_obs

    def _ensure_packed(self, pk, s):
        """Step s is about to run on the policy kernel pk: its packed weights (and the split weight images beside them) are made once per rollout — the parameters only
        change in update() — inside the captured rollout graph too; a rollout whose first steps took another branch packs at its first kernel step.  pk None: step s
        does not run on the kernel, and a replay of a rollout that does not START on it must not claim packed weights."""
        if pk is None:
            if s == 0:
                self._pk_recorded = False
        elif s == 0 or not self._pk_packed:
            self._img_cache = {}
            pk.pack()
            self._pk_packed = True
            self._pk_recorded = self._pk_recorded or s == 0

    def _rollout_noise(self, ac, st, s):
        """The standard-normal draws of step s ([N, A], the shape of the action rows).  One launch for the whole rollout at its first step instead of
        one per step (24 small launches on the chain of dependent kernels); the same law as Normal.sample() per step (actor_critic.py:123-125).
        A module whose _noise is overridden — the tests inject the reference's draws step by step — is asked per step as before."""
        if getattr(type(ac), "_noise", None) not in _PLAIN:
            return ac._noise(st.actions[s])
        if s == 0 or self._eps_all is None or self._eps_all.shape != st.actions.shape or self._eps_all.device != st.actions.device:
            self._eps_all = torch.randn_like(st.actions)
        return self._eps_all[s]

    def _transition_from_rows(self, actions, s):
        """a kernel wrote step s into the storage rows: the transition points at them.  -> actions"""
        st, t = self.storage, self.transition
        t.actions, t.values, t.actions_log_prob = actions, st.values[s], st.actions_log_prob[s].view(-1)
        t.action_mean, t.action_sigma = st.mu[s], st.sigma[s]
        return actions

    def _transition_to_rows(self, net, actions, values, s):
        """The eager formulation: `actions` just sampled from net's distribution and `values` become the transition and are copied into the storage rows.  -> actions"""
        st, t = self.storage, self.transition
        t.actions, t.values = actions.detach(), self._vn_raw(values.detach())          # (value normalisation: the storage holds raw values during the rollout)
        t.actions_log_prob = net.get_actions_log_prob(t.actions).detach()
        t.action_mean, t.action_sigma = net.action_mean.detach(), net.action_std.detach()
        st.actions[s].copy_(t.actions)
        st.values[s].copy_(t.values)
        st.actions_log_prob[s].copy_(t.actions_log_prob.view(-1, 1))
        st.mu[s].copy_(t.action_mean)
        st.sigma[s].copy_(t.action_sigma)
        return t.actions

    # The two per-step element-wise heads of the rollout as library kernels (go2sim_act_head, go2sim_store_transition): sampling +
    # log-prob + the storage rows in one launch, reward bootstrap + done copy in another, instead of ~23 small launches.

    def _act_head(self, mu, std, eps, value, s):
        st = self.storage
        mu, eps, value = mu.detach().contiguous(), eps.contiguous(), self._vn_raw(value.detach()).contiguous()
        actions = torch.empty_like(mu)
        p = self._ptr
        self._call("go2sim_act_head", p(mu), p(std.detach()), p(eps), p(value), p(actions), p(st.actions[s]), p(st.mu[s]), p(st.sigma[s]),
                   p(st.actions_log_prob[s]), p(st.values[s]), mu.shape[0], mu.shape[1], self._stream(mu))
        return self._transition_from_rows(actions, s)

    def rollout_targets(self):
        """Destinations for LeggedRobot.step(rollout=...) of the step being collected: the env kernel writes the next observations into the
        next storage rows and this step's reward / done rows itself (None: not applicable)."""
        st = self.storage
        if not self.fused_rollout or st.privileged_observations is None or st.dones.dtype != torch.uint8:
            return None
        s = st.step
        nxt = s + 1 < st.num_transitions_per_env
        return {"obs_out": st.observations[s + 1] if nxt else None, "priv_out": st.privileged_observations[s + 1] if nxt else None,
                "values": st.values[s].view(-1), "rewards_out": st.rewards[s].view(-1), "dones_out": st.dones[s].view(-1), "gamma": self.gamma}

    def _store_transition(self, rewards, dones, infos, s):
        if isinstance(infos, dict) and infos.get("transition_stored"):      # (the env step stored it: go2sim_step_rollout)
            return
        st = self.storage
        touts = infos.get("time_outs") if isinstance(infos, dict) else None
        rewards = rewards.contiguous().float()
        as_u8 = lambda x: None if x is None else (x if x.dtype == torch.uint8 else x.contiguous().view(torch.uint8) if x.dtype == torch.bool else x.to(torch.uint8))
        d, to = as_u8(dones), as_u8(touts.to(self.device) if touts is not None else None)
        p = self._ptr
        self._call("go2sim_store_transition", p(rewards), p(d), p(to), p(st.values[s]), p(st.rewards[s]), p(st.dones[s]), float(self.gamma), rewards.shape[0], self._stream(rewards))

    def _record_env_step(self, rewards, dones, infos):
        """the reward (bootstrapped on time-outs, ppo.py:107-108) and done rows of the step just taken; the storage moves on to the next slot.  -> the slot of that step"""
        st = self.storage
        s = st.step
        if self.fused_rollout:
            self._store_transition(rewards, dones, infos, s)
        else:
            r = rewards.clone()
            if "time_outs" in infos:
                r += self.gamma * torch.squeeze(st.values[s] * infos["time_outs"].unsqueeze(1).to(self.device), 1)
            st.rewards[s].copy_(r.view(-1, 1))
            st.dones[s].copy_(dones.view(-1, 1))
        st.step += 1
        self.transition.clear()
        return s


class _FusedPPOLoss(torch.autograd.Function):
    """loss = surrogate + c_v * value_loss - c_e * entropy through ONE library kernel (go2sim_ppo_loss) that also returns the
    analytic gradients w.r.t. mu, std and value; autograd then continues into the actor / critic MLPs.  Replaces ~150
    element-wise launches of the eager formulation per mini-batch with 2."""

    @staticmethod
    def kernel(alg, mu, std, value, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b):
        """-> stats [surrogate, value loss, kl, entropy, loss], d loss / d mu, / d std, / d value (shaped like `value`)"""
        B, A = mu.shape
        c = lambda t: t.detach().contiguous().float()
        mu_c, std_c, val_c = c(mu), c(std), c(value).view(-1)
        args = [mu_c, std_c, val_c, c(act_b), c(old_mu_b), c(old_sig_b), c(old_lp_b).view(-1), c(adv_b).view(-1), c(tv_b).view(-1), c(ret_b).view(-1)]
        gmu, gstd, gval = torch.empty_like(mu_c), torch.empty_like(std_c), torch.empty_like(val_c)
        stats = torch.empty(5, device=mu.device)
        ws = torch.empty(24 * ((B + 63) // 64), device=mu.device)       # (go2sim.h: 24 floats per block of 64 rows)
        p = alg._ptr
        alg._call("go2sim_ppo_loss", *[p(t) for t in args], p(gmu), p(gstd), p(gval), p(stats), p(ws), B, A, float(alg.clip_param), float(alg.value_loss_coef),
                  float(alg.entropy_coef), int(alg.use_clipped_value_loss), int(alg.surrogate_split), alg._stream(mu))
        return stats, gmu, gstd, gval.view_as(value)

    @staticmethod
    def forward(ctx, mu, std, value, alg, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b):
        stats, gmu, gstd, gval = _FusedPPOLoss.kernel(alg, mu, std, value, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sig_b)
        ctx.save_for_backward(gmu, gstd, gval)
        ctx.mark_non_differentiable(stats)
        return stats[4].clone(), stats

    @staticmethod
    def backward(ctx, g_loss, g_stats):
        gmu, gstd, gval = ctx.saved_tensors
        return gmu * g_loss, gstd * g_loss, gval * g_loss, None, None, None, None, None, None, None, None
