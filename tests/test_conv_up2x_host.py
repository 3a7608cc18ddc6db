"""CPU tests of the phase-collapsed upsample conv's host side: the collapse identity in float64 (ops.up2x_collapse, the
arithmetic of ops.conv_up2x_weight with the final fp16 rounding left out), the kernel's weight layout, the U-Net's
per-upsampler cache and the ABI's argument validation. No GPU compute is launched here."""
import pytest
import torch
import torch.nn.functional as F

from sdmoe import _lib, ops
from sdmoe.unet import Conv2d, Sampler


def _phase_convs(wc, x):
    """Four 2x2 convs on the low-resolution image with the geometry the kernel uses: phase (py, px), tap (a, c),
    output pixel (r, q) reads input (r + py + a - 1, q + px + c - 1), zero outside; result at (2r + py, 2q + px).
    wc [4, Cout, 2, 2, Cin], x [n, Cin, H, W] -> [n, Cout, 2H, 2W]."""
    n, _, H, W = x.shape
    y = x.new_zeros((n, wc.shape[1], 2 * H, 2 * W))
    for py in range(2):
        for px in range(2):
            # rows r + py - 1 .. r + py: pad (1 - py) above and py below; columns likewise
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            y[:, :, py::2, px::2] = F.conv2d(xp, wc[2 * py + px].permute(0, 3, 1, 2))
    return y


@pytest.mark.parametrize("n,H,W,Cin,Cout", [(2, 3, 5, 8, 6), (1, 1, 4, 8, 5), (2, 6, 1, 8, 5), (1, 1, 1, 8, 3),
                                            (1, 7, 4, 16, 8)])
def test_collapse_identity_float64(n, H, W, Cin, Cout):
    """nearest-2x upsample + 3x3 conv == four 2x2 phase convs of the collapsed weights, to <= 1e-12 relative in
    float64 (fp16 weights taken as float64, no final rounding), on H != W and on H or W = 1."""
    g = torch.Generator().manual_seed(n * 1000 + H * 100 + W * 10 + Cin)
    w = torch.randn((Cout, 3, 3, Cin), generator=g).half().double()  # taps-last, as ops.conv_weight takes
    x = torch.randn((n, Cin, H, W), generator=g).half().double()
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w.permute(0, 3, 1, 2), padding=1)
    wc = ops.up2x_collapse(w)
    assert wc.dtype == torch.float64 and tuple(wc.shape) == (4, Cout, 2, 2, Cin)
    got = _phase_convs(wc, x)
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"collapse identity {n}x{H}x{W} {Cin}->{Cout}: relative difference {rel:.3e}")
    assert rel <= 1e-12


def test_collapse_rule_and_layout():
    """Row a of phase row py sums kh {0} | {1, 2} (py = 0) or {0, 1} | {2} (py = 1), columns likewise; the kernel operand
    is fp16 [4, Cout, Cin/64, 2, 2, 64]: phase, 64-channel slice, tap, channel; summed in fp32 and rounded once."""
    g = torch.Generator().manual_seed(3)
    Cout, Cin = 5, 128
    w = torch.randn((Cout, 3, 3, Cin), generator=g).half()
    rows = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    wc = ops.conv_up2x_weight(w)
    assert wc.dtype == torch.float16 and tuple(wc.shape) == (4, Cout, Cin // 64, 2, 2, 64) and wc.is_contiguous()
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for c in range(2):
                    exp = sum(w[:, i, j].float() for i in rows[py, a] for j in rows[px, c]).half()
                    got = wc[2 * py + px, :, :, a, c, :].reshape(Cout, Cin)
                    assert torch.equal(got, exp), (py, px, a, c)
    with pytest.raises(ValueError):
        ops.conv_up2x_weight(torch.zeros((4, 3, 3, 96)))
    with pytest.raises(ValueError):
        ops.up2x_collapse(torch.zeros((4, 2, 2, 64)))


def test_unet_cache_invalidates_on_inplace_edit():
    """Sampler._collapsed_weight is made once per weight version: the same object while the filter is untouched, a new
    one (with the new values) after an in-place edit."""
    g = torch.Generator().manual_seed(5)
    Cout, Cin = 8, 64
    w = torch.randn((Cout, 3, 3, Cin), generator=g).half()
    # (a copy: at Cin = 64 conv_weight's result is a view of w, and the edit below must not reach w)
    s = Sampler(Conv2d(ops.conv_weight(w).clone(), torch.zeros(Cout, dtype=torch.float16)))
    first = s._collapsed_weight()
    assert torch.equal(first, ops.conv_up2x_weight(w))  # conv_weight's layout undone correctly
    assert s._collapsed_weight() is first
    with torch.no_grad():
        s.conv.weight.mul_(2.0)
    second = s._collapsed_weight()
    assert second is not first
    assert torch.equal(second, ops.conv_up2x_weight(w * 2))
    assert s._collapsed_weight() is second


def test_abi_validation_and_plan_without_gpu():
    lib = _lib.load()
    up = lib.sdmoe_conv_up2x
    assert up(None, 64, 1, 8, 8, 64, 1, None, 1, 64, 64, None, 0, None) == -1
    assert up(1, 64, 1, 8, 8, 60, 1, None, 1, 64, 64, None, 0, None) == -2      # Cin % 64
    assert up(1, 64, 1, 8, 8, 64, 1, None, 1, 60, 64, None, 0, None) == -2      # ldy % 8
    assert up(1, 64, 1, 8, 8, 64, 1, None, 1, 72, 72, None, 0, None) == -3      # Cout no multiple of the tile's columns
    assert up(1, 64, 0, 8, 8, 64, 1, None, 1, 64, 64, None, 0, None) == 0       # no images: nothing to do
    assert ops.conv_up2x_plan(2, 8, 8, 64, 72) is None
    assert ops.conv_up2x_plan(2, 8, 8, 60, 64) is None
    # the benchmark's three upsamplers at 16 images (256 CUs assumed without a device): tiles whose columns divide Cout
    for H, C in ((8, 1280), (16, 1280), (32, 640)):
        pl = ops.conv_up2x_plan(16, H, H, C, C)
        assert pl is not None and C % pl["tile"][1] == 0 and pl["ksplit"] * pl["kchunk"] >= 4 * C // 64, pl
