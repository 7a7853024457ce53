"""The update's diagnostics (`algorithm.diagnostics`, off by default): clip fraction, KL, explained variance, ratio and advantage statistics per mini-batch step, and
the gradient norm in front of the clip, computed on the device inside the update — in graph mode inside the captured graphs — and read back with ONE more device -> host
copy per update.  Read-only: nothing training reads is written, the weights after an update are bit for bit those of the key-off run.

Per mini-batch step and segment (PPO: one; the CTS family: teacher rows, student rows) one row of GO2NN_DIAG_NUM fp64 columns — include/go2nn.h has the one definition
(enum GO2NN_DIAG_*), _nn.DIAG_COLS restates the order.  Two formulations fill it:
  * go2nn_ppo_diag (csrc/go2nn_diag.h) behind go2nn_ppo_heads, where the mini-batch runs without autograd and mu / value never exist as tensors (modules/fused.py:pair_grads);
  * diag_rows_torch below wherever mu and value ARE tensors (the eager mode, the autograd formulations of graph mode): fp32 per-row terms, fp64 accumulation, written
    at the device-side slot cursor with index_copy_, so it captures.  It is also the numerical yardstick of the kernel (tests/test_update_diag_host.py).
The slot is a device-side cursor because the multi-rank step shape replays ONE captured graph per mini-batch slot for every epoch; it is zeroed once per update (begin).
The squared gradient norm: go2nn_grad_sqnorm in front of the clip + Adam call in graph mode, clip_grad_norm_'s own return value in eager mode.

What the figures are not: with several ranks they are this rank's shard's (no collective is added); `approx_kl` (k3) and `approx_kl_k1` are estimators from the ratio,
`kl` is the analytic Gaussian KL the learning-rate schedule uses; `explained_variance` is taken on each mini-batch's CURRENT critic, not on the rollout's."""
import ctypes as C
import math

import numpy as np
import torch

from ..._nn import DIAG_COLS, DIAG_MAX_COLS, DIAG_MIN_COLS, GO2NN_DIAG_NUM, GO2NN_GRAD_SQNORM_MAX, Go2nnPpoDiag

COL = {k: i for i, k in enumerate(DIAG_COLS)}
_KIND = np.array([1 if k in DIAG_MAX_COLS else (2 if k in DIAG_MIN_COLS else 0) for k in DIAG_COLS])
_LOG2PI = 1.8378770664093453


def diag_terms_torch(mu, sigma, value, actions, old_mu, old_sigma, old_logp, adv, old_values, returns, clip):
    """The per-row terms of the GO2NN_DIAG_NUM columns as a torch expression -> [B, GO2NN_DIAG_NUM] in the inputs' precision: fp32 in the kernel's arithmetic
    (float64 inputs stay float64: the tests' reference).  mu [B, A]; sigma [A] or [B, A]; the per-row inputs in any shape of B elements."""
    dt = torch.float64 if mu.dtype == torch.float64 else torch.float32
    f = lambda t: t.detach().to(dt)
    row = lambda t: f(t).reshape(-1)
    mu, actions, old_mu, old_sigma = f(mu), f(actions), f(old_mu), f(old_sigma)
    sigma = f(sigma).expand_as(mu)
    value, old_logp, adv, old_values, returns = row(value), row(old_logp), row(adv), row(old_values), row(returns)
    isg2 = 1.0 / (sigma * sigma)
    d, dm = actions - mu, old_mu - mu
    lp = (-(d * d) * (0.5 * isg2) - torch.log(sigma) - 0.5 * _LOG2PI).sum(-1)
    kl = (torch.log(sigma / old_sigma + 1.0e-5) + (old_sigma * old_sigma + dm * dm) * (0.5 * isg2) - 0.5).sum(-1)
    lr = lp - old_logp
    ratio = torch.exp(lr)
    err, dv = returns - value, value - old_values
    one = torch.ones_like(lr)
    cnt = lambda m: m.to(lr.dtype)
    return torch.stack([one, cnt((ratio - 1.0).abs() > clip), ratio, lr, (ratio - 1.0) - lr, kl, kl, adv, adv * adv, cnt(adv > 0), err, err * err, err.abs(),
                        returns, returns * returns, cnt(dv.abs() > clip), ratio, ratio], dim=1)


def diag_rows_torch(mu, sigma, value, actions, old_mu, old_sigma, old_logp, adv, old_values, returns, clip, split=0):
    """The GO2NN_DIAG_NUM columns of one mini-batch as a torch expression -> float64 [segments, GO2NN_DIAG_NUM] (segments = 2 for split > 0: rows [0, split) and the
    rest): the fp64 sums and extrema of diag_terms_torch's rows."""
    with torch.no_grad():
        terms = diag_terms_torch(mu, sigma, value, actions, old_mu, old_sigma, old_logp, adv, old_values, returns, clip).double()
        kind = torch.as_tensor(_KIND, device=terms.device)
        B = terms.shape[0]
        out = []
        for a, b in ([(0, B)] if split <= 0 else [(0, split), (split, B)]):
            t = terms[a:b]
            out.append(torch.where(kind == 1, t.amax(0), torch.where(kind == 2, t.amin(0), t.sum(0))))
        return torch.stack(out)


def pool_rows(rows):
    """rows [..., GO2NN_DIAG_NUM] (numpy) pooled over every leading axis: sums add, extrema combine -> [GO2NN_DIAG_NUM]"""
    r = np.asarray(rows, np.float64).reshape(-1, GO2NN_DIAG_NUM)
    return np.where(_KIND == 1, r.max(0), np.where(_KIND == 2, r.min(0), r.sum(0)))


def figures(row):
    """one (pooled) table row -> the derived figures"""
    g = lambda k: float(row[COL[k]])
    n = g("rows")
    if not n > 0:
        return {}
    var = lambda s, q: max(q / n - (s / n) ** 2, 0.0)
    var_err, var_ret, var_adv = var(g("verr_sum"), g("verr_sq")), var(g("ret_sum"), g("ret_sq")), var(g("adv_sum"), g("adv_sq"))
    return {"clip_fraction": g("ratio_clipped") / n, "approx_kl": g("k3_sum") / n, "approx_kl_k1": -g("logratio_sum") / n, "kl": g("kl_sum") / n, "kl_max": g("kl_max"),
            "ratio_mean": g("ratio_sum") / n, "ratio_max": g("ratio_max"), "ratio_min": g("ratio_min"),
            "explained_variance": 1.0 - var_err / var_ret if var_ret > 0.0 else float("nan"), "value_err_max": g("verr_abs_max"),
            "value_clip_fraction": g("value_clipped") / n, "adv_mean": g("adv_sum") / n, "adv_std": math.sqrt(var_adv), "adv_pos_share": g("adv_pos") / n}


def grad_figures(grad_sq, max_grad_norm, prefix=""):
    """the squared norms of one optimizer's steps -> grad_norm (mean), grad_norm_max, grad_clipped_share"""
    norm = np.sqrt(np.asarray(grad_sq, np.float64))
    return {prefix + "grad_norm": float(norm.mean()), prefix + "grad_norm_max": float(norm.max()), prefix + "grad_clipped_share": float((norm > max_grad_norm).mean())}


class UpdateDiagnostics:
    """The device buffers of one algorithm's diagnostics and what fills and reads them.  segments: names of the row segments; optimizers: their names ("" first)."""

    def __init__(self, device, epochs, mini_batches, segments, optimizers, clip, max_grad_norm):
        self.device, self.epochs, self.nmb, self.steps = device, int(epochs), int(mini_batches), int(epochs) * int(mini_batches)
        self.segments, self.optimizers, self.clip, self.max_grad_norm = tuple(segments), tuple(optimizers), float(clip), float(max_grad_norm)
        S, O, n = len(self.segments), len(self.optimizers), self.steps
        # (one row more than the update has steps: where the torch formulation's index_copy_ lands when the cursor is out of range — the kernels then write nothing)
        self.table = torch.zeros(n + 1, S, GO2NN_DIAG_NUM, dtype=torch.float64, device=device)
        self.grad_sq = torch.zeros(O, n + 1, dtype=torch.float64, device=device)
        self.cursors = torch.zeros(1 + O, dtype=torch.int32, device=device)          # [the table's | one per optimizer]
        self._partials, self._gpart = None, [None] * O
        self.host_table = self.host_grad_sq = self.result = None

    # ------------------------------------------------------------------ device side
    def begin(self):
        """once per update, in front of its first mini-batch step"""
        self.cursors.zero_()

    def _advance(self, k, value, dst):
        """dst[cursor k] = value (dst's last row when the cursor is out of range); the cursor moves on while it is in range"""
        c = self.cursors[k:k + 1]
        dst.index_copy_(0, c.clamp(0, self.steps).long(), value)
        c.add_((c < self.steps).to(torch.int32))

    def record_torch(self, mu, sigma, value, actions, old_mu, old_sigma, old_logp, adv, old_values, returns, split=0):
        rows = diag_rows_torch(mu, sigma, value, actions, old_mu, old_sigma, old_logp, adv, old_values, returns, self.clip, split)
        if rows.shape[0] != len(self.segments):
            raise ValueError("diagnostics: a mini-batch of %d segments for a table of %d" % (rows.shape[0], len(self.segments)))
        self._advance(0, rows[None], self.table)

    def record_kernel(self, nn, heads, stream):
        """go2nn_ppo_diag on the inputs of the go2nn_ppo_heads call `heads` (its Go2nnPpoHeads), on the same stream behind it"""
        B, A, K, split = heads.B, heads.A, heads.K, heads.surrogate_split
        if (2 if split > 0 else 1) != len(self.segments):
            raise ValueError("diagnostics: a mini-batch of %d segments for a table of %d" % (2 if split > 0 else 1, len(self.segments)))
        rows = nn.go2nn_ppo_diag_rows(B, A, K)
        if rows <= 0:
            raise RuntimeError("go2nn_ppo_diag: %s" % nn.go2nn_last_error().decode())
        need = rows * len(self.segments) * GO2NN_DIAG_NUM
        if self._partials is None or self._partials.numel() < need:
            self._partials = torch.zeros(need, dtype=torch.float64, device=self.device)
        d = Go2nnPpoDiag(*[getattr(heads, k) for k in ("y_a", "y_c", "w_mu", "b_mu", "w_v", "b_v", "std", "actions", "old_mu", "old_sigma", "old_logp", "adv", "old_values",
                                                      "returns")], self._partials.data_ptr(), self.table.data_ptr(), self.cursors.data_ptr(), B, A, K, split, self.steps, self.clip)
        if nn.go2nn_ppo_diag(C.byref(d), stream) != 0:
            raise RuntimeError("go2nn_ppo_diag: %s" % nn.go2nn_last_error().decode())

    def grad_from_norm(self, k, total_norm):
        """eager mode: clip_grad_norm_'s return value is the norm in front of the clip"""
        n = total_norm.detach().double().reshape(1)
        self._advance(1 + k, n * n, self.grad_sq[k])

    def grad_sqnorm(self, k, params, nn, stream):
        """graph mode, in front of the clip + Adam call: go2nn_grad_sqnorm over the gradients where it serves (fp32, contiguous, at most 48 tensors, a library), else the
        same sum as a torch expression"""
        grads = [p.grad for p in params if p.grad is not None]
        if nn is not None and 1 <= len(grads) <= GO2NN_GRAD_SQNORM_MAX and all(g.dtype == torch.float32 and g.is_contiguous() and 0 < g.numel() <= 2 ** 31 - 1 - 4096 for g in grads):
            ptrs = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
            numel = (C.c_int32 * len(grads))(*[g.numel() for g in grads])
            rows = nn.go2nn_grad_sqnorm_rows(numel, len(grads))
            if rows <= 0:
                raise RuntimeError("go2nn_grad_sqnorm: %s" % nn.go2nn_last_error().decode())
            if self._gpart[k] is None or self._gpart[k].numel() < rows:
                self._gpart[k] = torch.zeros(rows, dtype=torch.float64, device=self.device)
            cur = self.cursors.data_ptr() + 4 * (1 + k)
            if nn.go2nn_grad_sqnorm(ptrs, numel, len(grads), self._gpart[k].data_ptr(), self.grad_sq[k].data_ptr(), cur, self.steps, stream) != 0:
                raise RuntimeError("go2nn_grad_sqnorm: %s" % nn.go2nn_last_error().decode())
            return
        sq = torch.stack([g.detach().double().square().sum() for g in grads]).sum().reshape(1)
        self._advance(1 + k, sq, self.grad_sq[k])

    # ------------------------------------------------------------------ host side
    def read(self):
        """ONE device -> host copy: the tables of the update just run -> self.result (the derived figures), host_table [steps, segments, 18], host_grad_sq [steps, optimizers]"""
        n, S, O = self.steps, len(self.segments), len(self.optimizers)
        flat = torch.cat([self.table[:n].reshape(-1), self.grad_sq[:, :n].reshape(-1), self.cursors.double()]).cpu().numpy()
        tab, gsq, cur = flat[:n * S * GO2NN_DIAG_NUM].reshape(n, S, GO2NN_DIAG_NUM), flat[n * S * GO2NN_DIAG_NUM:-(1 + O)].reshape(O, n).T, flat[-(1 + O):]
        if not np.all(cur == n):
            raise RuntimeError("diagnostics: the update filled %s of %d slots (the table's, then one count per optimizer)" % (cur.astype(int).tolist(), n))
        self.host_table, self.host_grad_sq = tab.copy(), gsq.copy()
        spans = (("", slice(0, n)), ("/first_epoch", slice(0, self.nmb)), ("/last_epoch", slice(n - self.nmb, n)))

        def seg_figs(sel):
            out = {}
            for sfx, sp in spans:
                out.update({k + sfx: v for k, v in figures(pool_rows(tab[sp][:, sel])).items()})
            return out

        def grad_figs():
            out = {}
            for j, name in enumerate(self.optimizers):
                for sfx, sp in spans:
                    out.update({k + sfx: v for k, v in grad_figures(gsq[sp, j], self.max_grad_norm, name).items()})
            return out

        if S == 1:
            self.result = dict(seg_figs([0]), **grad_figs())
        else:
            self.result = {name: seg_figs([i]) for i, name in enumerate(self.segments)}
            self.result["all"] = dict(seg_figs(list(range(S))), **grad_figs())
        return self.result


def log_items(result):
    """[(tag under 'Diag/', value)] of an algorithm's `diagnostics` (flat for PPO, nested by segment for the CTS family)"""
    if not result:
        return []
    if all(isinstance(v, dict) for v in result.values()):
        return [("%s/%s" % (seg, k), v) for seg, d in result.items() for k, v in d.items()]
    return list(result.items())


def report_lines(result, pad=35):
    """the two lines of the iteration report: clip fraction / approximate KL / explained variance, and gradient norm / clipped share"""
    if not result:
        return ""
    d = result["all"] if "all" in result and isinstance(result["all"], dict) else result
    return (f"""{'Clip frac / approx KL / EV:':>{pad}} {d['clip_fraction']:.3f} / {d['approx_kl']:.5f} / {d['explained_variance']:.3f}\n"""
            f"""{'Grad norm / clipped share:':>{pad}} {d['grad_norm']:.3f} / {d['grad_clipped_share']:.2f}\n""")
