"""The rollout's policy kernels on a real MI355X against float64: go2nn_mlp3_kernel (go2_rl_gym_amd/csrc/go2nn_mlp3.h: split-bf16 planes, both weight rings, the clamped
duplicate tile, the even / odd LDS regions up to the fit boundary), go2nn_mlp_kernel with nn_finish (go2nn_impl.cpp: fp32 MFMA — the in-process fall-back of the shapes that do not
fit, and every small ragged shape in a fresh process with GO2_GEMM_SPLIT=0) and the two images go2nn_pack_kernel writes.  The checkers, their cases, input families, references and
bounds are those of tests/test_policy_paths.py (the CPU twin, where they are proved on the host build); this file hands them the HIP library.  Every network asserts that
go2nn_mlp_arith reports the kernel its case is meant for (3 = planes, 1 = fp32; tests/test_policy_paths.py: Net, CLAIMS — describe() restated, with the (NT, KV3, KB3) each shape
reaches), and a two-network launch counts as planes only if both report 3, the rule of run().  Run with -m gpu.

The bound of every compared output is e_kernel <= 4 * e_yardstick + 2^-23, componentwise in the carried scale S (tests/test_policy_paths.py); the exact families are compared with ==.
Measured on an MI355X (largest e_kernel with the e_yardstick of its case; largest share e_kernel / (4 e_yardstick + 2^-23) of the bound, with its case) — planes / fp32 (the fall-back
shapes in process, the small shapes in the GO2_GEMM_SPLIT=0 child):
  forward / forward_rows(NULL), one layer        8.5e-8 (5.0e-8) 0.26 scaled (1, 1)  /  2.5e-7 (2.3e-7) 0.24 gauss (496, 512); child 1.9e-7 (1.9e-7) 0.22 gauss (17, 33) 257 rows
  forward / forward_rows(NULL), several layers   8.5e-8 (6.8e-8) 0.22 scaled (65, 300, 33)  /  6.6e-8 (6.6e-8) 0.17 scaled (512, 352, 12); child 2.8e-8 (2.6e-8) 0.12 gauss (65, 300, 33)
  forward_rows: staging, pitches, out widths     1.8e-7 (1.5e-7) 0.24 gauss (17, 33)
    ... normalised                               3.4e-7 (2.8e-7) 0.28 scaled (17, 32)
    ... two networks / the normalised one        8.7e-9 (1.3e-8) 0.05 gauss (129, 288, 7) 97 rows / 1.6e-7 (1.4e-7) 0.23 int20 (65, 300, 33) 33 rows
  policy_act mu / value                          3.9e-8 (2.8e-8) 0.17 / 5.1e-8 (4.0e-8) 0.18 scaled  /  child 5.4e-9 (5.8e-9) 0.04 / 1.8e-8 (2.3e-8) 0.09 gauss N=257
  policy_act log-probability                     1.2e-7 (7.7e-8) 0.28 gauss A=12  /  child 1.6e-7 (8.3e-8) 0.35 gauss A=12 through policy_act_latent; the pair of which the critic
                                                 does not fit (both on fp32): 9.4e-8 (9.4e-8) 0.19
No case needs more than a 0.35 share of the bound.  EVERY exact case — integers up to 2^24, 24-bit inputs and 24-bit weights against one-hot partners, at one, two and six layers
and on both rings — is bit-equal to float64 on the device; none was moved to the bound.
Mutants of go2nn_mlp3.h / go2nn_impl.cpp, each built from a scratch copy and run once against this file (the tests that fail):
  (a) the lo . hi term of the six removed        forward int20 / bits_x / bits_w / scaled, every coherent case, rows, staging (bits_x), normalize, heads
  (b) nn3_split2 without its lo plane            forward int20 / bits_x, rows, staging (bits_x), two networks int20, normalize, heads
  (c) the mid plane in the image's lo slot       every packed-image case, forward bits_w / gauss, normalize, heads, same-rows, two networks gauss
  (d) kb < KV - 1                                every shape (int first), all staging widths, rows, two networks, normalize, heads
  (e) the epilogue's rows 4 g and 8 (r >> 2) swapped    every shape with more than 4 rows (rows[1] passes), staging, two networks, normalize, heads
  (f) the normaliser one term short              normalize = 1 at every out_dim, the two-network launch (its second network normalises)
  (g) the log-probability from j = 1             heads at every A, the NULL subsets, the mixed pair, the fp32 child
  the rotation of `wave` removed (an equivalent mutant): everything passes.
The host build's figures: tests/test_policy_paths.py."""
import pytest

pytestmark = pytest.mark.gpu

from go2_rl_gym_amd import _nn  # noqa: E402
import test_policy_paths as pp  # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("dims,kind", pp.FORWARD_CASES, ids=str)
def test_forward_on_gpu(dims, kind):
    """every ring / tile path of the planes kernel and, past the LDS-fit boundary, the same entry point and buffer on the fp32-MFMA kernel (reported as such); every input
    family the shape admits; 33 rows (two workgroups)"""
    d = pp.claim(dims)
    assert pp.want_arith(d) == (1 if pp.FP32_ONLY or dims in pp.FALLBACK_SHAPES else 3)
    pp.check_forward(_nn.load_nn(), DEV, dims, kind, 33)


@pytest.mark.parametrize("dims", pp.COHERENT_SHAPES, ids=str)
def test_forward_on_the_plane_coherent_set_on_gpu(dims):
    """the data on which six kept terms pass and any five fail (tests/test_policy_paths.py: test_coherent_set_tells_six_terms_from_five), on the planes kernel"""
    assert pp.FP32_ONLY or pp.want_arith(pp.claim(dims)) == 3
    pp.check_forward(_nn.load_nn(), DEV, dims, "coherent", 33)


@pytest.mark.parametrize("nrows", pp.ROWS)
def test_rows_on_gpu(nrows):
    pp.rows_case(_nn.load_nn(), DEV, nrows)


@pytest.mark.parametrize("dims", [(129, 288, 7), (65, 300, 33), (480, 512)], ids=str)
def test_every_workgroup_computes_what_workgroup_0_does_on_gpu(dims):
    """289 rows whose row r equals row r mod 32: ten workgroups, each with another rotation of the tiles' owners, bit-equal"""
    pp.check_same_rows(_nn.load_nn(), DEV, dims)


@pytest.mark.parametrize("in_dim", pp.STAGING_IN)
def test_staging_on_gpu(in_dim):
    """lane pairs and the four 128-column quads; two segments split at 1, inside a lane's pair, at in_dim - 1, or one segment; pitched inputs with NaN in the gap; row lists"""
    for kind in ("int", "bits_x"):
        pp.check_staging(_nn.load_nn(), DEV, in_dim, kind)


@pytest.mark.parametrize("kind", ["int", "int20", "gauss"])
def test_two_networks_on_row_subsets_on_gpu(kind):
    pp.check_two_networks(_nn.load_nn(), DEV, (129, 288, 7), (65, 300, 33), 97, 33, kind)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("out_dim", pp.NORMALIZE_OUT)
def test_normalize_on_gpu(out_dim, normalize):
    for kind in ("int", "gauss", "scaled"):
        pp.check_normalize(_nn.load_nn(), DEV, out_dim, normalize, kind)


@pytest.mark.parametrize("A", sorted(pp.HEAD_NETS))
def test_heads_on_gpu(A):
    pp.heads_case(_nn.load_nn(), DEV, A)


def test_heads_with_every_subset_of_optional_outputs_null_on_gpu():
    pp.null_subsets_case(_nn.load_nn(), DEV)


def test_heads_of_a_pair_of_which_one_network_does_not_fit_on_gpu():
    """the actor fits as planes, the critic does not: the launch runs fp32 for both (run()'s rule), and the actor's own forward is the planes kernel"""
    pp.check_act(_nn.load_nn(), DEV, (45, 512, 256, 128, 12), (300, 512, 512, 1), 33, "gauss")


@pytest.mark.parametrize("K,N", pp.IMAGE_SHAPES)
def test_packed_image_on_gpu(K, N):
    """what go2nn_pack writes, read back and decoded from the two layouts the headers state: fp32 operand order, padded bias, plane order, zero fill, zero k-blocks"""
    pp.check_image(_nn.load_nn(), DEV, K, N)


def test_refusals_on_gpu():
    pp.check_refusals(_nn.load_nn(), DEV)


def test_fp32_kernel_at_small_ragged_shapes_in_a_fresh_process():
    """GO2_GEMM_SPLIT=0 is read once per process: one child runs the integer-exact, gauss and bit-equality checkers on the fp32-MFMA kernel"""
    pp.run_fp32_child()


def test_measured_table_is_printed_on_gpu():
    pp.print_table()
