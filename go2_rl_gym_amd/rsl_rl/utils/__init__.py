"""Episode layout of a rollout for the recurrent policy's REFERENCE formulation (GO2_FUSED_MLP=0): the rollout [T, N, ...] cut at its dones into episode
segments, laid out as a zero-padded [T_pad, S, ...] batch of sequences with a validity mask, and back.  Segments are ordered env by env, each env's in time
order — the order the reference's generator hands to its RNN (rsl_rl/rsl_rl/utils/utils.py).  Building the layout reads the segment count and the longest
segment back to the host; the fixed-shape update of modules/fused_rnn.py needs none of this."""
import torch


class EpisodeLayout:
    """Where every (t, env) of a [T, N] rollout lands in the padded segment batch.
    starts[t, n]: an episode begins at step t of env n (t = 0, or the step after a done).  Segment ids count the starts env-major; the position of (t, n) inside
    its segment is t minus the step at which the segment began."""

    def __init__(self, dones):
        d = dones.reshape(dones.shape[0], dones.shape[1]).bool()
        T, N = d.shape
        starts = torch.ones_like(d)
        starts[1:] = d[:-1]
        em = starts.t().reshape(-1)                                    # env-major flags, (n, t) -> n * T + t
        seg = torch.cumsum(em.long(), 0) - 1                           # segment id of every (n, t)
        step = torch.arange(T, device=d.device).repeat(N)
        began = torch.where(em, step, torch.zeros_like(step))
        began = torch.cummax(began + (seg * T), 0).values - seg * T   # step at which the segment of (n, t) began (monotone within an env)
        self.T, self.N = T, N
        self.pos = (step - began).view(N, T).t()                       # [T, N]
        self.seg = seg.view(N, T).t()                                  # [T, N]
        self.num_segments = int(seg[-1]) + 1
        self.length = int(self.pos.max()) + 1                          # the longest episode segment = the padded length
        self.per_env = starts.sum(0)                                   # segments per env [N]
        self.first = torch.cat([torch.zeros(1, dtype=torch.long, device=d.device), torch.cumsum(self.per_env, 0)]).tolist()
        self.valid = torch.zeros(self.length, self.num_segments, dtype=torch.bool, device=d.device)
        self.valid[self.pos, self.seg] = True
        self.start_t = torch.nonzero(starts.t())[:, 1]                 # per segment (env-major): its first step and its env
        self.start_env = torch.nonzero(starts.t())[:, 0]

    def pad(self, x):
        """[T, N, ...] -> [T_pad, S, ...], zeros after each segment's end"""
        out = x.new_zeros((self.length, self.num_segments) + tuple(x.shape[2:]))
        out[self.pos, self.seg] = x
        return out

    def segments_of(self, start, stop):
        """the slice of segment ids that belong to envs [start, stop)"""
        return slice(self.first[start], self.first[stop])

    def initial_states(self, saved):
        """saved [T, L, N, H] (the state before each step) -> [L, S, H]: the state each segment starts from"""
        return saved[self.start_t, :, self.start_env].transpose(0, 1).contiguous()


def unpad(y, valid):
    """the inverse of EpisodeLayout.pad for a block of whole envs: y [T_pad, S, C] over the segments of n envs, valid [T_pad, S] -> [T_pad, n, C]
    (defined when the longest segment spans the whole rollout, T_pad = T — as for the reference's own inverse)"""
    rows = y.transpose(0, 1)[valid.t()]                                # the valid rows, segment by segment = env by env in time order
    T = y.shape[0]
    return rows.reshape(rows.shape[0] // T, T, y.shape[-1]).transpose(0, 1)
