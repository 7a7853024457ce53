"""The update's and the rollout's small "row" kernels of go2_rl_gym_amd/csrc/go2sim_impl.cpp on a real MI355X — go2_gae_kernel / go2_normalize_kernel, go2_ppo_loss_kernel +
its finish kernel, go2_act_head16_kernel / go2_act_head_kernel, go2_store_transition_kernel, go2_history_push_kernel, go2_adam_norm_kernel / go2_adam_step_kernel — at the
smallest shapes that reach each of their tail paths, against float64.  The checkers, their cases, references and bounds are those of tests/test_update_rows.py (the CPU
twin, where they are proved on the two host builds); this file only hands them the HIP library.  Run with -m gpu.

The bound of every compared output is e_kernel <= 4 * e_yardstick + 2^-23 (tests/test_update_rows.py: within).  Measured on an MI355X (largest e_kernel with the
e_yardstick of its case; largest share e_kernel / (4 e_yardstick + 2^-23) of the bound, with its case):
  GAE returns / advantages      2.0e-7 (4.6e-7)   0.22   T=5 N=64
  normalize                     1.7e-7 (8.5e-5)   0.27   T=3 N=63, count 63
  loss head gmu/gstd/gval/stats 8.3e-6 (8.4e-6)   0.49   B=65 A=5 split=64, gstd
  act head log-probability      6.2e-7 (1.7e-7)   0.79   N=1 A=33 (the one-thread-per-row kernel: 33 terms, each with a reciprocal and a hardware log2 under -ffast-math)
  Adam param / moments / lr     1.7e-7 (5.5e-6)   0.54   48 x numel 7, exp_avg_sq of the first step
  store transition              0.78 of its two-rounding bound
On the two host builds the same checkers reach 0.23 / 0.19 / 0.81 / 0.28 / 0.20 of the bound and 0.91 (tests/test_update_rows.py).  No case needs more than the factor 4."""
import pytest

pytestmark = pytest.mark.gpu

from helpers import load_hip  # noqa: E402
import test_update_rows as rows  # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("pattern", rows.GAE_DONES)
@pytest.mark.parametrize("T,N", rows.GAE_SHAPES)
def test_gae_and_normalize_on_gpu(T, N, pattern):
    rows.check_gae(load_hip(), DEV, T, N, pattern)


def test_normalize_grid_stride_on_gpu():
    rows.check_normalize_grid_stride(load_hip(), DEV)


@pytest.mark.parametrize("B,A,use_clip_v,split", rows.LOSS_CASES)
def test_ppo_loss_on_gpu(B, A, use_clip_v, split):
    rows.check_ppo_loss(load_hip(), DEV, B, A, use_clip_v, split)


def test_ppo_loss_refusals_on_gpu():
    rows.check_ppo_loss_refusals(load_hip(), DEV)


@pytest.mark.parametrize("N,A", rows.ACT_CASES)
def test_act_head_on_gpu(N, A):
    rows.check_act_head(load_hip(), DEV, N, A)


@pytest.mark.parametrize("N", rows.STORE_N)
def test_store_transition_on_gpu(N):
    rows.check_store_transition(load_hip(), DEV, N)


@pytest.mark.parametrize("N,H,D", rows.HISTORY_CASES)
def test_history_push_on_gpu(N, H, D):
    rows.check_history_push(load_hip(), DEV, N, H, D)


def test_adam_clip_step_on_gpu():
    rows.check_adam(load_hip(), DEV)


def test_adam_limits_on_gpu():
    rows.check_adam_limits(load_hip(), DEV)
