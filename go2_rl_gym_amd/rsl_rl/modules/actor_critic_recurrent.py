"""Recurrent actor-critic (rsl_rl/rsl_rl/modules/actor_critic_recurrent.py): an LSTM or GRU memory in front of each MLP head.
Same constructor, same parameter names (`memory_a.rnn.weight_ih_l0`, `memory_c.rnn.bias_hh_l0`, `actor.0.weight`, `std`, ...), so checkpoints move both ways.

The torch nn.LSTM / nn.GRU here is the REFERENCE formulation (GO2_FUSED_MLP=0, act_inference, the exporter); PPO on the GPU runs the memory on the library's
kernels instead (modules/fused_rnn.py).  Both keep the hidden states in the same persistent [num_layers, N, H] tensors, updated in place so that a captured
rollout reads and writes fixed addresses: where the reference rebinds `hidden_states` to fresh tensors after every step, the storage slot of the step is
therefore copied BEFORE the step (PPO.act), which is what the reference's saved references hold."""
import torch
import torch.nn as nn

from .actor_critic import ActorCritic
from ..utils import unpad

# rollout_storage.py:230 of the reference: `hid_c_batch = hid_c_batch[0] if len(hid_c_batch) == 1 else hid_a_batch` — for an LSTM the critic's update recurrence starts
# from the ACTOR's saved (h, c).  Reproduced; False would start it from the critic's own saved states, as the GRU does.
LSTM_CRITIC_STARTS_FROM_ACTOR_STATES = True


class ActorCriticRecurrent(ActorCritic):
    is_recurrent = True

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(256, 256, 256), critic_hidden_dims=(256, 256, 256), activation="elu",
                 rnn_type="lstm", rnn_hidden_size=256, rnn_num_layers=1, init_noise_std=1.0, **kwargs):
        if kwargs:
            print("ActorCriticRecurrent.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs.keys())))
        super().__init__(num_actor_obs=rnn_hidden_size, num_critic_obs=rnn_hidden_size, num_actions=num_actions, actor_hidden_dims=actor_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, activation=activation, init_noise_std=init_noise_std)
        self.memory_a = Memory(num_actor_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_size)
        self.memory_c = Memory(num_critic_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_size)

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def act(self, observations, masks=None, hidden_states=None):
        input_a = self.memory_a(observations, masks, hidden_states)
        return super().act(input_a.squeeze(0))

    def act_inference(self, observations):
        input_a = self.memory_a(observations)
        return super().act_inference(input_a.squeeze(0))

    def evaluate(self, critic_observations, masks=None, hidden_states=None):
        input_c = self.memory_c(critic_observations, masks, hidden_states)
        return super().evaluate(input_c.squeeze(0))

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states

    def init_hidden_states(self, num_envs, device):
        """zero states of num_envs rows (the reference starts from None = zeros); kept when they already have that shape"""
        self.memory_a.init_states(num_envs, device)
        self.memory_c.init_states(num_envs, device)


class Memory(nn.Module):
    def __init__(self, input_size, type="lstm", num_layers=1, hidden_size=256):
        super().__init__()
        self.is_lstm = type.lower() != "gru"
        rnn_cls = nn.LSTM if self.is_lstm else nn.GRU
        self.rnn = rnn_cls(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.hidden_states = None

    def init_states(self, n, device):
        L, H = self.rnn.num_layers, self.rnn.hidden_size
        cur = self.states()
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())          # ('cuda' and 'cuda:0' name the same device: keep the tensors a captured rollout reads)
        if cur and cur[0].shape == (L, n, H) and cur[0].device == dev:
            return
        z = lambda: torch.zeros(L, n, H, device=dev)
        self.hidden_states = (z(), z()) if self.is_lstm else z()

    def states(self):
        """[h] or [h, c]: the persistent state tensors [num_layers, N, H] (empty before the first step)"""
        hs = self.hidden_states
        if hs is None:
            return []
        return list(hs) if isinstance(hs, tuple) else [hs]

    def forward(self, input, masks=None, hidden_states=None):
        if masks is not None:          # batch mode (the reference update over padded trajectories): needs the saved states
            if hidden_states is None:
                raise ValueError("Hidden states not passed to memory module during policy update")
            out, _ = self.rnn(input, hidden_states)
            return unpad(out, masks)
        if self.hidden_states is None:
            self.init_states(input.shape[0], input.device)
        out, new = self.rnn(input.unsqueeze(0), self.hidden_states)
        for dst, src in zip(self.states(), list(new) if isinstance(new, tuple) else [new]):
            dst.copy_(src.detach())
        return out

    def reset(self, dones=None):
        """hidden rows of the done envs = 0 (Memory.reset of the reference; dones None: every row) — as an element-wise product: no host read of `dones`"""
        if self.hidden_states is None:
            return
        if dones is None:
            for s in self.states():
                s.zero_()
            return
        keep = (dones.reshape(1, -1, 1) == 0)
        for s in self.states():
            s.mul_(keep)
