"""Empirical (running mean / std) normalisation of an observation stream — upstream rsl_rl's `empirical_normalization` switch (its class is not part of the reference
imported here), `runner.empirical_normalization` in this package.

State per column, fp64: count | mean | M2 (the sum of squared deviations: var = M2 / count, the population variance); it starts at count 0, mean 0, var 1, and the
initial var is forgotten at the first batch.  From it the two fp32 vectors every formulation reads:
    mean32 = float(mean)        inv32 = float(1 / (sqrt(var) + eps))
    y = (x - mean32) * inv32    then clamped to [-clip, clip] when clip > 0
One fp32 subtraction and one fp32 product: torch, numpy and go2nn_obs_norm_apply (csrc/go2nn_obs_norm.h) agree on y bit for bit.

forward() is the torch statement of y: the eager formulation, the numerical yardstick of the kernel, and what is exported (it scripts).  merge() is the torch fp64 statement
of go2nn_obs_norm_update.  WHEN the statistics move is the algorithm's business (rsl_rl/algorithms/ppo.py: once per iteration, after the last optimizer step); forward()
never updates them.  Deviations from upstream: statistics frozen inside an iteration, and the clamp."""
import math

import torch
import torch.nn as nn


class EmpiricalNormalization(nn.Module):
    def __init__(self, num_features, eps=1e-2, clip=10.0, until=None):
        super().__init__()
        D = int(num_features)
        eps, clip = float(eps), 0.0 if clip is None else float(clip)
        if D < 1 or not (math.isfinite(eps) and eps > 0.0) or not math.isfinite(clip):
            raise ValueError("EmpiricalNormalization(num_features=%r, eps=%r, clip=%r): at least one column, a finite eps > 0, a finite clip (<= 0: no clamp)" % (num_features, eps, clip))
        self.num_features, self.eps, self.clip = D, eps, clip
        self.until = None if until is None else float(until)          # no batch is merged once count >= until (not part of a checkpoint: a property of the run)
        self.register_buffer("state", torch.zeros(1 + 2 * D, dtype=torch.float64))          # count | mean [D] | M2 [D]
        self.register_buffer("mean32", torch.zeros(D))
        self.register_buffer("inv32", torch.full((D,), float(1.0 / (1.0 + eps))))
        self.register_buffer("hyper", torch.tensor([eps, clip], dtype=torch.float64))       # (eps, clip) travel with a checkpoint: what it needs to run
        self._host_count = None          # the host's copy of count (it grows by a known number per merge: no device read per iteration)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + "hyper" in state_dict:
            self.eps, self.clip = (float(v) for v in self.hyper.tolist())
        self._host_count = None

    # ---- the state ---------------------------------------------------------------------------------------------------------------------------------------
    @property
    def count(self):
        return self.state[0]

    @property
    def mean(self):
        return self.state[1:1 + self.num_features]

    @property
    def var(self):
        """the population variance, fp64 [D]; 1 while nothing has been merged"""
        D = self.num_features
        c = self.state[0]
        return torch.where(c > 0, self.state[1 + D:] / torch.clamp(c, min=1.0), torch.ones_like(self.state[1 + D:]))

    def host_count(self):
        if self._host_count is None:
            self._host_count = float(self.state[0].item())          # (once after construction / a load)
        return self._host_count

    def accepts(self):
        """does the next batch still count (the `until` cap; decided on the host)"""
        return self.until is None or self.host_count() < self.until

    def note_merged(self, n):
        """a launch merged n samples into the state on the device"""
        self._host_count = self.host_count() + float(n)

    def _derive(self):
        self.mean32.copy_(self.mean.to(torch.float32))
        self.inv32.copy_((1.0 / (torch.sqrt(self.var) + self.eps)).to(torch.float32))

    @torch.no_grad()
    def set_state(self, count, mean, var):
        """(tests, loading) count samples of the given per-column mean and population variance; count 0: var is not kept"""
        D = self.num_features
        as64 = lambda v: torch.as_tensor(v, dtype=torch.float64, device=self.state.device).reshape(-1).expand(D)
        count = float(count)
        self.state[0] = count
        self.state[1:1 + D] = as64(mean)
        self.state[1 + D:] = as64(var) * count
        self._host_count = count
        self._derive()

    @torch.no_grad()
    def merge(self, batch):
        """Chan's pooled update with the rows of `batch` [n, D] (raw observations), the fp64 statement of go2nn_obs_norm_update: sums centred on the frozen fp32 mean"""
        D = self.num_features
        x = batch.reshape(-1, D)
        n = float(x.shape[0])
        if n == 0:
            return
        m32 = self.mean32.to(torch.float64)
        d = x.to(torch.float64) - m32
        S1, S2 = d.sum(0), (d * d).sum(0)
        mb, M2b = m32 + S1 / n, torch.clamp(S2 - S1 * (S1 / n), min=0.0)
        count = self.host_count()
        ma = self.mean.clone()
        M2a = self.state[1 + D:].clone() if count > 0 else torch.zeros_like(ma)
        tot, delta = count + n, mb - ma
        self.state[0] = tot
        self.state[1:1 + D] = ma + delta * (n / tot)
        self.state[1 + D:] = M2a + M2b + delta * delta * (count * (n / tot))
        self._host_count = tot
        self._derive()

    # ---- y -------------------------------------------------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = (x - self.mean32) * self.inv32
        if self.clip > 0.0:
            y = torch.clamp(y, -self.clip, self.clip)
        return y


class ValueNormalization(nn.Module):
    """Running mean / std of the raw GAE returns (`algorithm.normalize_value`; rl_games' `normalize_value`, PopArt's cousin): the critic predicts v^ = (v - mean) / std.
    State, fp64 [3]: count | mean | M2; it starts at count 0, mean 0, var 1, as EmpiricalNormalization does.  From it the three fp32 scalars every formulation reads,
        stat32 = mean32 | std32 | inv32 = float(mean) | float(sqrt(var) + eps) | float(1 / (sqrt(var) + eps))
        normalize:   x^ = (x - mean32) * inv32        denormalize:   x = x^ * std32 + mean32
    one fp32 subtraction and one fp32 product, no clamp: torch, numpy and go2nn_value_norm_apply (csrc/go2nn_value_norm.h) agree bit for bit.  merge() is the torch fp64
    statement of go2nn_value_norm_update, the output-preserving rewrite of the critic's last layer included.  WHEN the statistics move is the algorithm's business
    (rsl_rl/algorithms/_base.py: once per iteration, behind the last optimizer step)."""

    def __init__(self, eps=1e-2, until=None, preserve=False):
        super().__init__()
        eps = float(eps)
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError("ValueNormalization(eps=%r): a finite eps > 0" % (eps,))
        self.eps, self.preserve = eps, bool(preserve)
        self.until = None if until is None else float(until)          # no batch is merged once count >= until (a property of the run, not of a checkpoint)
        self.register_buffer("state", torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64))          # count | mean | M2
        self.register_buffer("stat32", torch.tensor([0.0, 1.0 + eps, 1.0 / (1.0 + eps)], dtype=torch.float32))
        self.register_buffer("hyper", torch.tensor([eps], dtype=torch.float64))          # eps travels with a checkpoint
        self._host_count = None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + "hyper" in state_dict:
            self.eps = float(self.hyper[0].item())
        self._host_count = None

    @property
    def count(self):
        return self.state[0]

    @property
    def mean(self):
        return self.state[1]

    @property
    def var(self):
        """the population variance, fp64; 1 while nothing has been merged"""
        c = self.state[0]
        return torch.where(c > 0, self.state[2] / torch.clamp(c, min=1.0), torch.ones_like(c))

    def host_count(self):
        if self._host_count is None:
            self._host_count = float(self.state[0].item())          # (once after construction / a load)
        return self._host_count

    def accepts(self):
        return self.until is None or self.host_count() < self.until

    def note_merged(self, n):
        self._host_count = self.host_count() + float(n)

    def _derive(self):
        sd = torch.sqrt(self.var) + self.eps
        self.stat32.copy_(torch.stack([self.mean, sd, 1.0 / sd]).to(torch.float32))

    @torch.no_grad()
    def set_state(self, count, mean, var):
        """(tests, loading) count samples of the given mean and population variance; count 0: var is not kept"""
        count = float(count)
        self.state.copy_(torch.tensor([count, float(mean), float(var) * count], dtype=torch.float64))
        self._host_count = count
        self._derive()

    @torch.no_grad()
    def merge(self, returns, last_layer=None):
        """Chan's pooled update with the RAW returns (any shape), sums centred on the frozen fp32 mean; last_layer = (weight [1, K], bias [1]) of the critic: rewritten
        in fp32 so that its raw value stays what it was (output preservation)"""
        x = returns.reshape(-1)
        n = float(x.numel())
        if n == 0:
            return
        old = self.stat32.clone()
        m32 = old[0].to(torch.float64)
        d = x.to(torch.float64) - m32
        S1, S2 = d.sum(), (d * d).sum()
        mb, M2b = m32 + S1 / n, torch.clamp(S2 - S1 * (S1 / n), min=0.0)
        count = self.host_count()
        ma = self.state[1].clone()
        M2a = self.state[2].clone() if count > 0 else torch.zeros_like(ma)
        tot, delta = count + n, mb - ma
        self.state.copy_(torch.stack([torch.full_like(ma, tot), ma + delta * (n / tot), M2a + M2b + delta * delta * (count * (n / tot))]))
        self._host_count = tot
        self._derive()
        if last_layer is not None:
            w, b = last_layer
            new = self.stat32
            w.mul_(old[1] / new[1])
            b.copy_((old[1] * b + old[0] - new[0]) / new[1])

    def normalize(self, x):
        return (x - self.stat32[0]) * self.stat32[2]

    def denormalize(self, x):
        return x * self.stat32[1] + self.stat32[0]


def attach_value_normalizer(actor_critic, eps=1e-2, until=None, preserve=False):
    """The child `value_normalizer` of an actor-critic (`algorithm.normalize_value`); without this call the module's state dict has the keys it always had."""
    if getattr(actor_critic, "value_normalizer", None) is None:
        dev = next(actor_critic.parameters()).device
        actor_critic.value_normalizer = ValueNormalization(eps, until, preserve).to(dev)
    return actor_critic.value_normalizer


def attach_normalizers(actor_critic, num_actor_obs, num_critic_obs, eps=1e-2, clip=10.0, until=None, shared=False):
    """The children `obs_normalizer` (actor stream) and `critic_obs_normalizer` (privileged stream) of an actor-critic; a task without a privileged observation
    (shared) has one normaliser for the shared rows, under the first name.  Without this call the module's state dict has the keys it always had."""
    dev = next(actor_critic.parameters()).device
    if getattr(actor_critic, "obs_normalizer", None) is None:
        actor_critic.obs_normalizer = EmpiricalNormalization(num_actor_obs, eps, clip, until).to(dev)
    if not shared and getattr(actor_critic, "critic_obs_normalizer", None) is None:
        actor_critic.critic_obs_normalizer = EmpiricalNormalization(num_critic_obs, eps, clip, until).to(dev)
    return actor_critic


def normalizer_widths(state_dict):
    """-> (actor columns, critic columns or None) of the normalisers a checkpoint's model_state_dict carries, or None when it carries none"""
    a, c = state_dict.get("obs_normalizer.mean32"), state_dict.get("critic_obs_normalizer.mean32")
    if a is None:
        return None
    return int(a.numel()), (int(c.numel()) if c is not None else None)
