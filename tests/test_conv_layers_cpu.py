"""The fp64 checks of tests/conv_check.py (used by tests/test_conv_layers_gpu.py on every conv plan of the image engine)
against the oracle's own convolutions, and their power to flag the errors a kernel makes: one wrong element, a dropped
row tile, two images swapped."""
import numpy as np
import pytest

from oracle import tf_semantics as S
from conv_check import ConvCheck, LinearConv, bf16_round, bf16_ulp, fp8_round, sample_images, tap_corr, E4M3

SHAPES = [
    # (role, N, H, W, Cin, Cout, k, stride)
    ("fwd", 5, 9, 7, 6, 10, 3, 1),
    ("fwd", 4, 11, 9, 5, 8, 3, 2),        # stride 2, SAME, odd extents
    ("fwd", 3, 13, 10, 3, 16, 7, 2),      # the stem's window on odd extents
    ("fwd", 6, 5, 6, 12, 7, 1, 1),
    ("dgrad", 5, 9, 7, 6, 10, 3, 1),
    ("dgrad", 4, 6, 8, 16, 12, 1, 1),
    ("dgrad", 3, 13, 11, 3, 16, 7, 2),    # the stem's input gradient (Conv2DBackpropInput, stride 2) on odd extents
]


def _case(role, N, H, W, Ci, Co, k, s, seed=0):
    rng = np.random.RandomState(seed)
    w = rng.standard_normal((k, k, Ci, Co)) * 0.2
    op = LinearConv(role, w, s, H, W)
    OH, OW = -(-H // s), -(-W // s)
    if role == "fwd":
        x = np.maximum(rng.standard_normal((N, H, W, Ci)), 0)
        ref = S.conv2d_same(x, w, s)
    else:
        x = rng.standard_normal((N, OH, OW, Co))
        ref = S.conv2d_same_bwd_input(x, w, (N, H, W, Ci), s)
    return op, x, ref, rng


@pytest.mark.parametrize("case", SHAPES)
def test_projection_and_sampled_rows_agree_with_the_oracle(case):
    op, x, ref, rng = _case(*case)
    assert np.allclose(op.ref(x), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    for _ in range(3):
        r = rng.standard_normal(ref.shape[:3])
        want = np.tensordot(r, ref, axes=([0, 1, 2], [0, 1, 2]))
        got = op.project(x, r)
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max(), case
    chk = ConvCheck(op, x, 2e-4, rng, full_below=2)
    assert chk.imgs == sample_images(x.shape[0]) and chk.imgs[-1] == x.shape[0] - 1
    assert chk.rows(ref) <= 1e-8 and chk.projection(ref) <= 1e-6
    assert np.allclose(chk.column_sums(), ref.sum((0, 1, 2)), rtol=1e-11, atol=1e-11 * np.abs(ref).max())
    # rounding of the size fp32 accumulation leaves passes both checks
    noisy = ref * (1 + rng.uniform(-1e-6, 1e-6, size=ref.shape))
    assert chk.rows(noisy) <= 0.1 and chk.projection(noisy) <= 0.1


def test_tap_correlation_is_the_filter_gradient():
    rng = np.random.RandomState(2)
    for (n, h, w, ca, cb, k, s) in ((3, 9, 7, 4, 5, 3, 1), (2, 11, 10, 3, 6, 7, 2), (5, 6, 5, 2, 3, 1, 1)):
        a = rng.standard_normal((n, h, w, ca))
        b = rng.standard_normal((n, -(-h // s), -(-w // s), cb))
        want = S.conv2d_same_bwd_filter(a, b, (k, k, ca, cb), s)
        assert np.abs(tap_corr(a, b, k, s, chunk=2) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("case", [SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[6]])
def test_the_checks_flag_planted_errors(case):
    """As test_fuzz_harness_reports_a_planted_mismatch does for the fuzz harness: the errors a wrong tile index, a skipped
    last tile or a mixed-up image offset make are caught -- by the sampled rows where they land there, by the projection
    anywhere else."""
    op, x, ref, rng = _case(*case, seed=5)
    N = x.shape[0]
    assert N >= 3
    fresh = lambda: ConvCheck(op, x, 2e-4, np.random.RandomState(7), full_below=0)
    chk = fresh()
    outside = [i for i in range(N) if i not in chk.imgs]
    assert chk.rows(ref) <= 1e-8 and chk.projection(ref) <= 1e-6

    # one wrong element, in a sampled image and in one the rows do not see
    for img in (chk.imgs[-1], outside[0] if outside else chk.imgs[0]):
        bad = ref.copy()
        bad[img, -1, -1, -1] += 0.5 * np.abs(ref).max()
        c = fresh()
        assert c.rows(bad) > 1 or c.projection(bad) > 1, img
    bad = ref.copy()
    bad[chk.imgs[-1], -1, -1, -1] += 0.5 * np.abs(ref).max()
    assert fresh().rows(bad) > 1

    # one row tile (128 rows of the flattened output, here the last one: the ragged tile) dropped / left at zero
    flat = ref.reshape(-1, ref.shape[-1]).copy()
    tile = min(128, flat.shape[0] // 2)
    flat[-tile:] = 0.0
    c = fresh()
    assert c.rows(flat.reshape(ref.shape)) > 1 and c.projection(flat.reshape(ref.shape)) > 1
    flat = ref.reshape(-1, ref.shape[-1]).copy()
    m0 = ref.shape[1] * ref.shape[2] * (outside[0] if outside else 1)          # a tile inside an image the rows skip
    flat[m0:m0 + tile] = 0.0
    assert fresh().projection(flat.reshape(ref.shape)) > 1

    # two images swapped
    if len(outside) >= 2:
        a, b = outside[0], outside[1]
    else:
        a, b = 0, 1
    sw = ref.copy()
    sw[[a, b]] = sw[[b, a]]
    assert fresh().projection(sw) > 1


def test_rounding_helpers():
    x = np.array([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -3.14159, 0.0])
    assert list(bf16_round(x)) == [1.0, 1.0, 1.0 + 2 ** -6, -3.140625, 0.0]
    assert bf16_ulp(1.0) == 2 ** -7 and bf16_ulp(1.99) == 2 ** -7 and bf16_ulp(2.0) == 2 ** -6
    assert list(fp8_round(np.array([1000.0, 1.0625, 0.0009765625 * 1.5]), *E4M3)) == [448.0, 1.0, 0.001953125]
