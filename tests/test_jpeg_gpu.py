"""ds_jpeg_reconstruct on the device against ds_jpeg_reconstruct_host AND against Pillow, all bytes equal: the grid of
test_jpeg_cpu.py as one ragged launch per sampling class plus one mixed launch, sentinel bytes around and between the crops,
two runs bitwise equal, and one launch of 256 images of 75 x 100."""
import numpy as np
import pytest
import torch

from test_jpeg_cpu import check_bytes, decode_all, encode, grid, pil_rgb, pixels
from tumblr_emotions_amd import ops

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
MARGIN = 64


def _launch(items):
    """One ragged launch over every (image, crop box) of `items`: checked against the host statement and against PIL."""
    coef, desc, nbytes, expect = decode_all(items)
    desc["out_offset"] += MARGIN
    expect = [(l, b, off + MARGIN, r) for l, b, off, r in expect]
    host = np.full(nbytes + 2 * MARGIN, SENTINEL, np.uint8)
    ops.jpeg_reconstruct_host(coef, desc, host)
    coef_dev = torch.from_numpy(coef).cuda()
    runs = []
    for _ in range(2):
        out = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
        ops.jpeg_reconstruct(coef_dev, desc, out)
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])                      # reproducible: one lane per byte
    assert np.array_equal(runs[0], host)                         # the host statement, sentinels included
    check_bytes(runs[0], nbytes, expect, sentinel=SENTINEL)      # Pillow; gaps and margins untouched
    return len(desc)


@pytest.mark.parametrize("sub", (0, 1, 2, "L"))
def test_one_ragged_launch_per_sampling_class(sub):
    items = [g for g in grid() if g[0].split("-")[1] == str(sub)]
    assert len(items) == 81
    assert _launch(items) == 6 * 81


def test_one_mixed_launch():
    items = grid()[::5] + grid()[1::7]
    assert len({g[0].split("-")[1] for g in items}) == 4
    _launch(items)


def test_a_batch_of_256_images():
    items = []
    for i in range(256):
        sub = (0, 1, 2, "L")[i % 4]
        data = encode(pixels(75, 100, ("noise", "gradient")[(i // 4) % 2], seed=i), sub, (30, 90, 100)[i % 3])
        items.append(("75x100-%s-%d" % (sub, i), data, pil_rgb(data)))
    coef, desc, nbytes, expect = decode_all(items)
    keep = np.arange(1, len(desc), 6)                            # the loader's central crop of every image
    desc, expect = desc[keep].copy(), [expect[k] for k in keep]
    assert len(desc) == 256
    out = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    ops.jpeg_reconstruct(torch.from_numpy(coef).cuda(), desc, out)
    got = out.cpu().numpy()
    for label, box, off, ref in expect:
        assert np.array_equal(got[off:off + ref.size].reshape(ref.shape), ref), label


def test_bad_arguments_are_errors_before_the_launch():
    coef, desc, nbytes, _ = decode_all(grid()[:1])
    out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_reconstruct(torch.from_numpy(coef), desc, out)
    with pytest.raises(ValueError, match="scratch"):
        ops.jpeg_reconstruct(torch.from_numpy(coef).cuda(), desc, out, scratch=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    bad = desc.copy()
    bad["crop_w"][0] = 10 ** 6
    with pytest.raises(ValueError):
        ops.jpeg_reconstruct(torch.from_numpy(coef).cuda(), bad, out)
