"""The recurrent memory of ActorCriticRecurrent on the library's kernels (include/go2nn.h ABI 7, csrc/go2nn_rnn.h) — what PPO runs on the GPU in place of nn.LSTM / nn.GRU.

A step of a layer = two products on the split-operand (3 x bf16) GEMMs, gi = x W_ih^T + b_ih and gh = h W_hh^T + b_hh (go2nn_linear_elu_forward_group, act 1), and one
cell launch (go2nn_rnn_cell_forward).  The rollout groups the actor's and the critic's memory into the same launches.  The update (RnnFunction) runs the whole
[T, B] block of a mini-batch at fixed shapes: the input products of all T steps are one GEMM, then per step one gh GEMM and one cell launch, which also hands the next
step its carry — the saved state where the step ended an episode (`done`), else the new state.  After the reference's unpad this is exactly what its split / pad /
unpad computes (storage/rollout_storage.py, tests/test_recurrent_host.py), with no host read, no padding and graph-capturable.  Backward runs the steps in reverse
(go2nn_rnn_cell_backward + one input-gradient GEMM per step), then dW_ih, dW_hh and the biases are one weight-gradient GEMM / column sum each over all T B rows."""
import ctypes as C

import torch

from . import fused
from .fused import _Launch, _LinearView


def _p(t):
    return t.data_ptr() if t is not None else None


def _layers(mem):
    """[(ih, hh)] per layer as _LinearView (weight, bias): the parameters torch's nn.LSTM / nn.GRU registers (weight_ih_l{k}, weight_hh_l{k}, bias_ih_l{k}, bias_hh_l{k})"""
    r = mem.rnn
    return [(_LinearView(getattr(r, "weight_ih_l%d" % l), getattr(r, "bias_ih_l%d" % l)), _LinearView(getattr(r, "weight_hh_l%d" % l), getattr(r, "bias_hh_l%d" % l)))
            for l in range(r.num_layers)]


def _type(mem):
    from ..._nn import GO2NN_RNN_LSTM, GO2NN_RNN_GRU
    return GO2NN_RNN_LSTM if mem.is_lstm else GO2NN_RNN_GRU


def _cell_forward(k, jobs):
    from ..._nn import Go2nnRnnCellJob
    k.check(k.nn.go2nn_rnn_cell_forward((Go2nnRnnCellJob * len(jobs))(*jobs), len(jobs), k.stream), "go2nn_rnn_cell_forward")


def _cell_backward(k, jobs):
    from ..._nn import Go2nnRnnCellBwdJob
    k.check(k.nn.go2nn_rnn_cell_backward((Go2nnRnnCellBwdJob * len(jobs))(*jobs), len(jobs), k.stream), "go2nn_rnn_cell_backward")


def available():
    """the library pair is loaded (the switch of the MLP nodes: GO2_FUSED_MLP=0 leaves it unset and the memory runs as torch's nn.LSTM / nn.GRU)"""
    return fused._LIB is not None and fused._NN is not None


def check_shape(mem):
    """the memory shapes the kernels take: a hidden size that is a multiple of 4 up to GO2NN_MAX_WIDTH (the heads' input; the plain input-gradient GEMM of the
    fp32-MFMA path reads rows of H in 4-float vectors).  Raises instead of falling back: GO2_FUSED_MLP=0 is the formulation for other sizes."""
    from ..._nn import GO2NN_MAX_WIDTH
    H = mem.rnn.hidden_size
    if H % 4 or H > GO2NN_MAX_WIDTH:
        raise ValueError("recurrent memory on the library's kernels: rnn_hidden_size must be a multiple of 4 up to %d (got %d); GO2_FUSED_MLP=0 runs torch's RNN"
                         % (GO2NN_MAX_WIDTH, H))


class RolloutMemory:
    """The rollout side: one step of BOTH memories per call (every layer: one grouped gi launch, one grouped gh launch, one grouped cell launch), the reset
    of the done rows, the critic's extra step of compute_returns.  images(): the split weight images, once per rollout (the parameters change in update() only)."""

    def __init__(self, ac):
        check_shape(ac.memory_a)
        check_shape(ac.memory_c)
        self.ac = ac
        self.mems = [ac.memory_a, ac.memory_c]
        self._imgs = None

    def images(self):
        k = _Launch(self.ac.memory_a.rnn.weight_ih_l0.device)
        lins = [m for mem in self.mems for pair in _layers(mem) for m in pair]
        self._imgs = k.images(lins)
        return self._imgs

    def _img(self, j, l, which):
        L = self.mems[0].rnn.num_layers
        return self._imgs[(j * L + l) * 2 + which]

    def step(self, xs, which=(0, 1), slots=None):
        """xs: the inputs [N, K] of the memories `which` (0 actor, 1 critic); slots: per memory the storage tensors ([T, L, N, H] list, step s) that receive the
        state BEFORE the step, or None.  -> the last layer's new h [N, H] per memory (a view of the persistent state)"""
        if self._imgs is None:
            self.images()
        mems = [self.mems[j] for j in which]
        k = _Launch(xs[0].device)
        L = mems[0].rnn.num_layers
        lays = [_layers(m) for m in mems]
        for l in range(L):
            st = [m.states() for m in mems]
            ins = [x if l == 0 else s[0][l - 1] for x, s in zip(xs, st)]
            gi = k.forward([(x, lays[j][l][0], self._img(which[j], l, 0)) for j, x in enumerate(ins)], act=1)
            gh = k.forward([(s[0][l], lays[j][l][1], self._img(which[j], l, 1)) for j, s in enumerate(st)], act=1)
            jobs = []
            for j, m in enumerate(mems):
                h = st[j][0][l]
                c = st[j][1][l] if m.is_lstm else None
                sl = slots[j] if slots is not None else None
                sh = sl[0][0][sl[1], l] if sl is not None else None
                sc = sl[0][1][sl[1], l] if (sl is not None and m.is_lstm) else None
                jobs.append(_job(gi[j], gh[j], h, c, h, c, save_h=sh, save_c=sc, B=h.shape[0], H=h.shape[1], typ=_type(m)))
            _cell_forward(k, jobs)
        return [m.states()[0][L - 1] for m in mems]

    def reset(self, dones_u8):
        """rows with dones != 0 of every state tensor = 0: one launch"""
        from ..._nn import GO2NN_RNN_MAX_STATES
        sts = [s for m in self.mems for s in m.states()]
        assert len(sts) <= GO2NN_RNN_MAX_STATES and dones_u8.dtype == torch.uint8 and dones_u8.is_contiguous()
        L, N, H = sts[0].shape
        arr = (C.c_void_p * len(sts))(*[s.data_ptr() for s in sts])
        nn_ = fused._NN
        stream = C.c_void_p(torch.cuda.current_stream(sts[0].device).cuda_stream) if sts[0].is_cuda else None
        rc = nn_.go2nn_rnn_reset(arr, len(sts), L, N, H, C.c_void_p(dones_u8.data_ptr()), stream)
        if rc != 0:
            raise RuntimeError("go2nn_rnn_reset failed: %s" % nn_.go2nn_last_error().decode())


def _job(gi, gh, h_prev, c_prev, h, c, gates=None, save_h=None, save_c=None, done=None, sub_h=None, sub_c=None, next_h=None, next_c=None, B=0, H=0, typ=0):
    from ..._nn import Go2nnRnnCellJob
    return Go2nnRnnCellJob(_p(gi), _p(gh), _p(h_prev), _p(c_prev), _p(h), _p(c), _p(gates), _p(save_h), _p(save_c), _p(done), _p(sub_h), _p(sub_c), _p(next_h), _p(next_c),
                           B, H, typ, 0)


class RnnFunction(torch.autograd.Function):
    """y [T, B, H] (the last layer's h of every step) = the memory over x [T, B, K] at fixed shapes.  saved_h / saved_c: per layer the states [T, B, H] the rollout
    stored before each step (saved_c None for a GRU); dones [T, B] uint8: step t ended the episode, so step t + 1 starts from the saved state (and step 0 always does).
    params: weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, ... (torch's order); gradients for them only (obs and the saved states are leaves)."""

    @staticmethod
    def forward(ctx, x, saved_h, saved_c, dones, typ, *params):
        T, B, _ = x.shape
        L = len(params) // 4
        lays = [(_LinearView(params[4 * l], params[4 * l + 2]), _LinearView(params[4 * l + 1], params[4 * l + 3])) for l in range(L)]
        lstm = saved_c is not None
        H = lays[0][1].in_features
        k = _Launch(x.device)
        imgs = k.images([m for pair in lays for m in pair])
        inp = x.reshape(T * B, -1)
        keep = []
        for l in range(L):
            ih, hh = lays[l]
            gi = k.forward([(inp, ih, imgs[2 * l])], act=1)[0].view(T, B, -1)
            hp = torch.empty(T, B, H, device=x.device)
            hp[0].copy_(saved_h[l][0])
            cp = cs = None
            if lstm:
                cp, cs = torch.empty(T, B, H, device=x.device), torch.empty(T, B, H, device=x.device)
                cp[0].copy_(saved_c[l][0])
            y = torch.empty(T, B, H, device=x.device)
            gates = torch.empty(T, B, 4 * H, device=x.device)
            for t in range(T):
                gh = k.forward([(hp[t], hh, imgs[2 * l + 1])], act=1)[0]
                nxt = t + 1 < T
                _cell_forward(k, [_job(gi[t], gh, hp[t], cp[t] if lstm else None, y[t], cs[t] if lstm else None, gates=gates[t], done=dones[t] if nxt else None,
                                       sub_h=saved_h[l][t + 1] if nxt else None, sub_c=saved_c[l][t + 1] if (nxt and lstm) else None,
                                       next_h=hp[t + 1] if nxt else None, next_c=cp[t + 1] if (nxt and lstm) else None, B=B, H=H, typ=typ)])
            keep.append((inp, hp, cp, cs, gates))
            inp = y.view(T * B, H)
        ctx.lays, ctx.imgs, ctx.keep, ctx.dones, ctx.typ, ctx.shape = lays, imgs, keep, dones, typ, (T, B, H, L, lstm)
        ctx.nparams = len(params)
        return y

    @staticmethod
    def backward(ctx, gy):
        T, B, H, L, lstm = ctx.shape
        lays, imgs, dones = ctx.lays, ctx.imgs, ctx.dones
        k = _Launch(gy.device)
        dy = gy.contiguous().view(T, B, H)
        sink = {}
        for l in range(L - 1, -1, -1):
            inp, hp, cp, cs, gates = ctx.keep[l]
            ih, hh = lays[l]
            G = ih.out_features
            dgi, dgh = torch.empty(T, B, G, device=gy.device), torch.empty(T, B, G, device=gy.device)
            carry = torch.empty(B, H, device=gy.device)          # dc (LSTM) / dh z (GRU) of the step after; not read at the last step
            rec = None
            for t in range(T - 1, -1, -1):
                from ..._nn import Go2nnRnnCellBwdJob
                job = Go2nnRnnCellBwdJob(_p(gates[t]), _p(cs[t]) if lstm else None, _p(cp[t]) if lstm else None, None if lstm else _p(hp[t]), _p(dy[t]), _p(rec),
                                         None if lstm else _p(carry), _p(carry) if lstm else None, _p(dones[t]) if t + 1 < T else None, _p(dgi[t]), _p(dgh[t]), B, H, ctx.typ, 0)
                _cell_backward(k, [job])
                if t > 0:
                    rec = k.bwd_in([(dgh[t], hh, None, imgs[2 * l + 1])], plain=True)[0][0]
            k.wgrad([(dgi.view(T * B, G), inp, ih)], sink=sink, tag=(l, "ih"))
            k.wgrad([(dgh.view(T * B, G), hp.view(T * B, H), hh)], sink=sink, tag=(l, "hh"))
            gb_ih, gb_hh = k.new(G), k.new(G)
            k.sums.append((dgi.view(T * B, G), gb_ih, T * B, G))
            k.sums.append((dgh.view(T * B, G), gb_hh, T * B, G))
            sink[((l, "ih"), "b")], sink[((l, "hh"), "b")] = gb_ih, gb_hh
            if l > 0:
                dy = k.bwd_in([(dgi.view(T * B, G), ih, None, imgs[2 * l])], plain=True)[0][0].view(T, B, H)
        k.finish()
        grads = []
        for l in range(L):
            grads += [sink[((l, "ih"), "w")], sink[((l, "hh"), "w")], sink[((l, "ih"), "b")], sink[((l, "hh"), "b")]]
        ctx.keep = None
        return (None, None, None, None, None) + tuple(grads)


def memory_sequence(mem, x, saved, dones):
    """the update's memory output [T, B, H] through RnnFunction.  saved: [h_states] or [h_states, c_states], each [T, L, B, H]"""
    check_shape(mem)
    L = mem.rnn.num_layers
    sh = [saved[0][:, l] for l in range(L)]
    sc = [saved[1][:, l] for l in range(L)] if mem.is_lstm else None
    params = [getattr(mem.rnn, "%s_l%d" % (n, l)) for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return RnnFunction.apply(x.contiguous(), sh, sc, dones, _type(mem), *params)
