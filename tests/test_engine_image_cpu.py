"""Host-side decisions of the image engine that need no device."""
import pytest


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [16, 128, 129, 256])
def test_side_arrangement_by_batch_size(B, dtype):
    """side_mode None: only the Branch_3 chain beside the main one (2) up to 128 fp32 samples, one side stream for Branch_3
    and Branch_2 (1) above that and for the 16-bit configurations at every batch size (the sweeps quoted in
    InceptionV1Engine.__init__); a captured step keeps one side stream."""
    from tumblr_emotions_amd.engine_image import InceptionV1Engine
    want = 2 if (dtype == "f32" and B <= 128) else 1
    assert InceptionV1Engine.side_arrangement(None, B, dtype) == want
    assert InceptionV1Engine.side_arrangement(None, B, dtype, capturing=False) == want
    assert InceptionV1Engine.side_arrangement(None, B, dtype, capturing=True) == 1


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_an_explicit_side_mode_is_returned_as_given(mode):
    from tumblr_emotions_amd.engine_image import InceptionV1Engine
    for B in (16, 256):
        for dtype in ("f32", "bf16"):
            assert InceptionV1Engine.side_arrangement(mode, B, dtype) == mode
            assert InceptionV1Engine.side_arrangement(mode, B, dtype, capturing=True) == 1
