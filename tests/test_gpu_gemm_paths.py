"""The grouped GEMMs of go2_rl_gym_amd/csrc/go2nn_bx3.h (split-operand bf16 MFMA: go2nn_bx3_kernel<1 / 2 / 3, EPI>, its weight-gradient mode, the fused EPI_DELU_WG epilogue,
go2nn_bx3_split_kernel) and of go2nn_gemm3.h / go2nn_gemm.h (fp32 MFMA: go2nn_gemm3_kernel, go2nn_wgrad_kernel, the single-network fall-backs) on a real MI355X against float64,
at the smallest ragged shapes that reach each tile path.  The checkers, their cases, input families, references and bounds are those of tests/test_gemm_paths.py (the CPU twin,
where they are proved on the host build); this file hands them the HIP library, and every case asserts through go2nn_linear_group_tile_rows resp.
go2nn_linear_backward_weight_group_kernel that it reached the 64- / 128- / 192-row tile or the weight-gradient kernel it is meant for.  Run with -m gpu.

The bound of every compared output is e_kernel <= 4 * e_yardstick + 2^-23, componentwise in S = sum |a| |b| (tests/test_gemm_paths.py: within_s); the exact family is
compared with ==.  Measured on an MI355X (largest e_kernel with the e_yardstick of its case; largest share e_kernel / (4 e_yardstick + 2^-23) of the bound, with its case):
  forward split, 64 / 128 / 192 rows per tile     2.1e-7 (1.4e-7) 0.31 / 2.6e-7 (1.8e-7) 0.31 / 2.4e-7 (2.7e-7) 0.20   gauss M=70 K=33 N=33 / M=129 K=144 N=130 / M=1537 K=20 N=2557
    ... outputs on the ELU's negative branch      2.3e-7 (9.8e-8) 0.44 / 1.6e-7 (1.0e-7) 0.31 / 8.8e-8 (1.2e-7) 0.14   scaled M=70 K=70 N=128 (with the scale S + 1: 0.26 / 0.26 / 0.14)
  forward fp32                                    4.3e-7 (2.8e-7) 0.35   scaled M=191 K=20 N=33;  ELU < 0: 2.2e-7 (1.1e-7) 0.40 (S + 1: 0.34)
  input gradient split, 64 / 128 rows per tile    2.2e-7 (1.6e-7) 0.29 / 1.8e-7 (1.1e-7) 0.33   gauss M=70 C=144 Kin=128 ld=131 / scaled M=129 C=4 Kin=130 plain
    ... its column sums                           1.0e-7 (8.6e-8) 0.22 / 1.3e-7 (1.2e-7) 0.21
  input gradient fp32 / its column sums           2.7e-7 (1.9e-7) 0.31 / 1.7e-7 (1.1e-7) 0.30
  fused: gz_prev, column sums / dW below          1.2e-7 (7.6e-8) 0.27 / 1.6e-7 (1.2e-7) 0.27   gauss M=1 C=7 Kin=45 Kx=64
  weight gradient split 128x128 / fp32 64x128 / fp32 64x64     2.8e-7 (5.5e-7) 0.12 / 2.8e-7 (5.9e-7) 0.11 / 2.3e-7 (3.8e-7) 0.14   scaled M=70
No case needs more than a 0.44 share of the bound: the bf16 pipe's accumulation bias (about a third of an ulp per output, go2nn.h) does not show in this componentwise measure at
these contraction lengths.  EVERY exact case is bit-equal to float64 on the device, the 24-bit plane variants included: at these shapes the bf16 matrix pipe loses no bit of a sum
of products that fp32 can hold, so no exact case had to be moved to the bound.
The host build's figures: tests/test_gemm_paths.py."""
import pytest

pytestmark = pytest.mark.gpu

from go2_rl_gym_amd import _nn  # noqa: E402
import test_gemm_paths as gp  # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M", sorted(gp.FWD_M))
def test_forward_on_gpu(M, act, split):
    """64-row tiles at M = 70, 128-row tiles at 129 (one row in the last tile), 150 (its second half empty), 191, 192; every (K, N) of FWD_K x FWD_N"""
    gp.forward_case(_nn.load_nn(), DEV, M, act, split, gp.FWD_M[M])


def test_forward_unaligned_output_on_gpu():
    """y 4 bytes past a 16-byte boundary: scalar stores although N is a multiple of 4"""
    for kind in ("int", "gauss"):
        gp.check_forward(_nn.load_nn(), DEV, 150, [(20, 132), (48, 128)], 0, True, kind, 128, y_front=1)


def test_forward_two_jobs_on_the_xcd_interleave_on_gpu():
    """both jobs' tile counts multiples of 8: the workgroup -> (job, tile) map that deals each job's tiles to the 8 XCDs"""
    for kind in ("int", "gauss"):
        gp.check_forward(_nn.load_nn(), DEV, 70, [(20, 512), (48, 500)], 0, True, kind, 64)


@pytest.mark.parametrize("K,act", [(20, 0), (7, 1)])
def test_forward_192_row_tiles_on_gpu(K, act):
    """M = 8 x 192 + 1 with 40 column tiles: the smallest ragged shape whose workgroup count picks the 192-row tile"""
    for kind in ("int", "gauss"):
        gp.check_forward(_nn.load_nn(), DEV, 1537, [(K, 2500), (K, 2557)], act, True, kind, 192)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("M", sorted(gp.IG_M))
def test_input_gradient_on_gpu(M, plain, split):
    gp.input_grad_case(_nn.load_nn(), DEV, M, plain, split, gp.IG_M[M])


@pytest.mark.parametrize("M,C_,Kin,kx0,kx1,keep_gz", gp.FUSED_SHAPES)
def test_fused_weight_gradient_below_on_gpu(M, C_, Kin, kx0, kx1, keep_gz):
    for kind in gp.FUSED_KINDS(C_):
        gp.check_fused(_nn.load_nn(), DEV, M, C_, Kin, kx0, kx1, keep_gz, kind)


@pytest.mark.parametrize("M,shapes,split,kernel,slices", gp.WGRAD_CASES)
def test_weight_gradient_on_gpu(M, shapes, split, kernel, slices):
    for kind in gp.WGRAD_KINDS(M):
        gp.check_wgrad(_nn.load_nn(), DEV, M, shapes, split, kernel, slices, kind)


@pytest.mark.parametrize("k", range(len(gp.IMAGE_SHAPES)))
def test_split_image_on_gpu(k):
    """what go2nn_split_weights writes, decoded from the layout go2nn_bx3.h states: plane order, chunk swizzle, zero fill, the transposed image"""
    gp.check_split_image(_nn.load_nn(), DEV, gp.IMAGE_SHAPES[k], gp.IMAGE_SHAPES[(k + 1) % len(gp.IMAGE_SHAPES)])


def test_measured_table_is_printed_on_gpu():
    gp.test_measured_table_is_printed()
