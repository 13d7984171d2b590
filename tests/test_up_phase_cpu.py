"""The identity behind the up-ResBlock phase conv (csrc/nn_gemm.hip, k_conv_igemm<4>), checked on the CPU in float64:
conv3x3(nearest_x2(x), w, pad 1) == the interleave of four 2x2 convs over x whose weights are sums of the 3x3 taps that land on the
same source pixel.  No GPU, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

# output phase p (0 / 1 along one axis), source tap t (0 / 1) -> the 3x3 taps that read that source pixel
TAPS_OF = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def phase_weights(w):
    """w [Cout, Cin, 3, 3] -> [2, 2, Cout, Cin, 2, 2] (py, px, o, c, ty, tx), summed in (ky, kx) order in w's dtype."""
    out = torch.zeros((2, 2) + tuple(w.shape[:2]) + (2, 2), dtype=w.dtype)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    acc = torch.zeros(w.shape[:2], dtype=w.dtype)
                    for ky in TAPS_OF[(py, ty)]:
                        for kx in TAPS_OF[(px, tx)]:
                            acc = acc + w[:, :, ky, kx]
                    out[py, px, :, :, ty, tx] = acc
    return out


def phase_conv(x, wp):
    """x [N, Cin, H, W], wp from phase_weights -> [N, Cout, 2H, 2W]: output pixel (2y + py, 2x + px) reads source rows y - 1 + py + ty."""
    N, _, H, W = x.shape
    y = torch.zeros((N, wp.shape[2], 2 * H, 2 * W), dtype=x.dtype)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            y[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], wp[py, px])
    return y


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 4), (4, 3), (5, 5), (8, 8), (7, 2)])
def test_up2_conv3x3_equals_four_phase_convs_f64(H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn((2, 5, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((6, 5, 3, 3), generator=g, dtype=torch.float64) * 0.2
    up = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    assert torch.equal(up, F.interpolate(x, scale_factor=2, mode='nearest'))
    ref = F.conv2d(up, w, padding=1)
    got = phase_conv(x, phase_weights(w))
    assert got.shape == ref.shape == (2, 6, 2 * H, 2 * W)
    assert (got - ref).abs().max().item() <= 1e-12           # borders included: the zero padding of the x2 image is the zero padding of x


def test_every_tap_is_used_exactly_once_per_phase():
    """Each phase's four tap groups partition the nine 3x3 taps: 4 phases x 4 source taps carry 4 x 9 products' worth of weights."""
    for py in range(2):
        for px in range(2):
            seen = sorted((ky, kx) for ty in range(2) for tx in range(2) for ky in TAPS_OF[(py, ty)] for kx in TAPS_OF[(px, tx)])
            assert seen == [(ky, kx) for ky in range(3) for kx in range(3)]
