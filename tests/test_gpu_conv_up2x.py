"""The phase-collapsed nearest-2x upsample conv (sdmoe_conv_up2x, MODE_CONV_UP2X) on the MI355X.

Reference: fp32 torch (nearest upsample, then F.conv2d) with the `close` bars of tests/test_gpu_kernels.py (max-abs
1e-2 of the scale and rel-L2 2e-3). Outputs are pre-filled with NaN, so a phase or a row that is never written fails.
Against the old fused-upsample kernel: rel-L2(new vs reference) <= 2 x rel-L2(old vs the same reference) -- the one extra
fp16 rounding of the summed weights adds an independent error of the size of the output rounding (a CPU model gives
2.9e-4 against 2.1e-4, 1.4 x); the factor 2 leaves room for accumulation-order differences."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sdmoe import _lib, ops, tune  # noqa: E402
import sdmoe.unet as unet_mod  # noqa: E402

DEV = "cuda"
TOL = 1e-2
REL_L2 = 2e-3


def close(out, ref, tol=TOL, rel=REL_L2):
    """tests/test_gpu_kernels.py's bars; returns the relative L2."""
    out, ref = out.float(), ref.float()
    err = (out - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert math.isfinite(err) and err <= tol * scale, f"max err {err:.4g} vs scale {scale:.4g}"
    r = (out - ref).norm().item() / ref.norm().item()
    assert r <= rel, f"rel L2 {r:.4g} > {rel}"
    return r


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, torch.float16)


def conv_ref(x, nimg, H, W, w, b):
    xc = F.interpolate(x.float().view(nimg, H, W, -1).permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    y = F.conv2d(xc, w.float().permute(0, 3, 1, 2), b.float(), padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


_CASES = {}


def case(nimg, H, W, Cin, Cout):
    """Inputs, collapsed weight and fp32 reference of a shape, made once and shared (never modified)."""
    key = (nimg, H, W, Cin, Cout)
    if key not in _CASES:
        x = rnd(nimg * H * W, Cin, seed=H * 7 + W)
        w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=Cin + 1), rnd(Cout, scale=0.1, seed=Cout + 2)
        _CASES[key] = (x, w, b, ops.conv_up2x_weight(w), conv_ref(x, nimg, H, W, w, b))
    return _CASES[key]


def run_new(x, nimg, H, W, wc, b, out=None):
    """The new kernel alone (no fallback) into a NaN-filled output; None where it refuses."""
    Cout = wc.shape[1]
    if out is None:
        out = torch.full((nimg * 4 * H * W, Cout), float("nan"), dtype=torch.float16, device=DEV)
    xp, ldx = x.data_ptr(), x.stride(0)
    return ops.conv_up2x_launch(xp, ldx, nimg, H, W, x.shape[1], wc, b, out, out.data_ptr(), out.stride(0), Cout)


SMALL = [(2, 3, 5, 64, 320),    # every pixel on a border, H != W, an M tail of 30 rows
         (2, 8, 8, 640, 640)]   # two N tiles per phase at BN = 320 (test_tile_knob[3]), four at the auto plan's 160
BENCH = [(2, 8, 8, 1280, 1280), (2, 16, 16, 1280, 1280), (2, 32, 32, 640, 640)]  # the benchmark's upsamplers, 2 images


@pytest.mark.parametrize("nimg,H,W,Cin,Cout", SMALL + BENCH)
def test_conv_up2x(nimg, H, W, Cin, Cout):
    x, w, b, wc, ref = case(nimg, H, W, Cin, Cout)
    out = run_new(x, nimg, H, W, wc, b)
    assert out is not None, "sdmoe_conv_up2x refused a supported shape"
    r = close(out, ref)
    print(f"conv_up2x {nimg}x{H}x{W} {Cin}->{Cout}: rel L2 {r:.3e}, plan {ops.conv_up2x_plan(nimg, H, W, Cin, Cout)}")
    assert torch.equal(ops.conv_up2x(x, nimg, H, W, wc, b), out)  # the public op: the same launch


@pytest.mark.parametrize("nimg,H,W,Cin,Cout", SMALL[1:] + BENCH)
def test_error_within_twice_the_fused_upsample_kernel(nimg, H, W, Cin, Cout):
    x, w, b, wc, ref = case(nimg, H, W, Cin, Cout)
    new = close(run_new(x, nimg, H, W, wc, b), ref)
    old = close(ops.conv3x3(x, nimg, H, W, ops.conv_weight(w), b, upsample=True), ref)
    print(f"conv_up2x {nimg}x{H}x{W} {Cin}->{Cout}: rel L2 new {new:.3e}, old {old:.3e}, ratio {new / old:.2f}")
    assert new <= 2 * old


def test_output_column_slice_of_a_wider_buffer():
    """The U-Net writes into the left columns of the next block's concat buffer: ldy honoured, neighbours untouched."""
    nimg, H, W, Cin, Cout = SMALL[1]
    x, w, b, wc, ref = case(nimg, H, W, Cin, Cout)
    for lo in (0, 320):
        buf = torch.full((nimg * 4 * H * W, Cout + 640), float("nan"), dtype=torch.float16, device=DEV)
        buf[:, :lo] = 7.0
        buf[:, lo + Cout:] = 7.0
        assert run_new(x, nimg, H, W, wc, b, out=buf[:, lo:lo + Cout]) is not None
        close(buf[:, lo:lo + Cout], ref)
        assert (buf[:, :lo] == 7.0).all() and (buf[:, lo + Cout:] == 7.0).all()


def test_input_column_slice_of_a_wider_buffer():
    nimg, H, W, Cin, Cout = SMALL[0]
    x, w, b, wc, ref = case(nimg, H, W, Cin, Cout)
    buf = rnd(nimg * H * W, Cin + 128, seed=9)
    buf[:, 64:64 + Cin] = x
    close(run_new(buf[:, 64:64 + Cin], nimg, H, W, wc, b), ref)


@pytest.mark.parametrize("ks", [2, 3])
def test_forced_splits(ks):
    """Split-K (needed at one prompt per call): fp32 slabs + splitk_reduce_up2x_kernel, which shares the row map."""
    nimg, H, W, Cin, Cout = SMALL[1]
    x, w, b, wc, ref = case(nimg, H, W, Cin, Cout)
    with tune.tuned(ksplit=ks):
        assert ops.conv_up2x_plan(nimg, H, W, Cin, Cout)["ksplit"] == ks
        out = run_new(x, nimg, H, W, wc, b)
    close(out, ref)
    # and into a column slice, as the U-Net's one-prompt calls do
    buf = torch.full((nimg * 4 * H * W, Cout + 64), float("nan"), dtype=torch.float16, device=DEV)
    buf[:, Cout:] = 7.0
    with tune.tuned(ksplit=ks):
        run_new(x, nimg, H, W, wc, b, out=buf[:, :Cout])
    assert torch.equal(buf[:, :Cout], out) and (buf[:, Cout:] == 7.0).all()


ACCEPTED_TILES = {1: (128, 160), 2: (64, 160), 3: (256, 320), 4: (256, 160), 6: (128, 320)}


@pytest.mark.parametrize("tile", range(1, 9))
def test_tile_knob(tile):
    """Every value of the tile knob: the new mode is built on the tiles of values 1-4 and 6; 5, 7 and 8 name tiles it
    is not built on, which the entry point refuses (-3) and ops.conv_up2x answers through the fallback."""
    nimg, H, W, Cin, Cout = SMALL[1]
    x, w, b, wc, ref = case(nimg, H, W, Cin, Cout)
    with tune.tuned(tile=tile):
        pl = ops.conv_up2x_plan(nimg, H, W, Cin, Cout)
        out = run_new(x, nimg, H, W, wc, b)
        if tile in ACCEPTED_TILES:
            assert pl["tile"] == ACCEPTED_TILES[tile] and out is not None
        else:
            assert pl is None and out is None
            out = torch.full_like(ref, float("nan"), dtype=torch.float16)
            ops.conv_up2x(x, nimg, H, W, wc, b, out=out, fallback=ops.conv_weight(w))
    close(out, ref)


def test_refused_cout_falls_back():
    """Cout = 200: N = 800 takes 160-column tiles, which would straddle two phases -> -3; the op falls back to the
    fused-upsample conv with a correct result, and without a fallback filter it is an error."""
    nimg, H, W, Cin, Cout = 2, 4, 6, 64, 200
    x, w, b, wc, ref = case(nimg, H, W, Cin, Cout)
    assert ops.conv_up2x_plan(nimg, H, W, Cin, Cout) is None
    assert run_new(x, nimg, H, W, wc, b) is None
    out = torch.full_like(ref, float("nan"), dtype=torch.float16)
    ops.conv_up2x(x, nimg, H, W, wc, b, out=out, fallback=ops.conv_weight(w))
    close(out, ref)
    with pytest.raises(_lib.SdmoeError):
        ops.conv_up2x(x, nimg, H, W, wc, b)


def test_unet_with_collapse_off_and_on(monkeypatch):
    """A small U-Net evaluation with UPCONV_COLLAPSE off (the fused-upsample conv) passes tests/test_gpu_unet.py's
    bound for the default path, max|eps - ref| <= 3e-2 * max(1, max|ref|) against the fp32 oracle, and builds no
    collapsed weight; the default path passes it too and does build them."""
    from oracle.unet_ref import UNetRef
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import prompt_embedding
    from sdmoe.weights import make_state_dict

    cfg = UNetConfig.tiny(16)
    sd = make_state_dict(cfg, 0)
    ref_net = UNetRef({k: v.half().float() for k, v in sd.items()}, cfg)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 16, 16, generator=g)
    d = cfg.cross_attention_dim
    ctx = torch.stack([prompt_embedding("", d), prompt_embedding("a photo of a cat", d)])
    r = ref_net(x, 501.0, ctx)
    for on in (False, True):
        monkeypatch.setattr(unet_mod, "UPCONV_COLLAPSE", on)
        unet = unet_mod.UNet2DConditionModel.from_state_dict(sd, cfg, DEV)
        for m in unet.modules():
            if isinstance(m, unet_mod.GEGLU):
                m.gelu, m.patterns = unet_mod._gelu, None
        eps = unet(x.to(DEV), 501.0, ctx.to(DEV)).float().cpu()
        err = (eps - r).abs().max().item() / max(1.0, r.abs().max().item())
        print(f"UPCONV_COLLAPSE {on}: max rel err {err:.3e}")
        assert err <= 3e-2
        made = [blk.upsamplers[0]._up2x_w is not None for blk in unet.up_blocks if hasattr(blk, "upsamplers")]
        assert len(made) == 3 and all(m == on for m in made)
