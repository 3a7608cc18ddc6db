"""Per-kernel numerics of libsdmoe_hip.so on the MI355X against plain PyTorch fp32 references of the same op.

Tolerances (fp16 storage, fp32 accumulation): max |out - ref| <= TOL * max(1, max |ref|) with TOL = 1e-2 for
GEMM/conv/attention outputs (fp16 output rounding is 2^-11 relative; K up to 11520 adds accumulation-order
differences), 2e-3 for the normalisation statistics; and everywhere relative L2 <= 2e-3 (close()).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sdmoe import ops, tune  # noqa: E402

DEV = "cuda"
TOL = 1e-2
REL_L2 = 2e-3


def close(out, ref, tol=TOL, rel=REL_L2):
    """max-abs bound (scaled) AND a relative-L2 bound: the max-abs bar alone is ~20x the fp16 output rounding and
    would pass a localised indexing error (one tile, head or halo row wrong by < 1e-2 of the output's peak); the
    rel-L2 bar of 2e-3 (~8x the fp16 rounding's 2.4e-4 RMS) fails any such error that touches > ~1 % of the output."""
    out, ref = out.float(), ref.float()
    err = (out - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert math.isfinite(err) and err <= tol * scale, f"max err {err:.4g} vs scale {scale:.4g}"
    if rel is not None:
        den = ref.norm().item()
        r = (out - ref).norm().item() / den if den > 0 else (out - ref).norm().item()
        assert r <= rel, f"rel L2 {r:.4g} > {rel}"


def rnd(*shape, scale=1.0, dtype=torch.float16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, dtype)


@pytest.mark.parametrize("M,N,K", [(256, 320, 320), (130, 640, 768), (4096, 2560, 320), (64, 1280, 5120),
                                   (1, 1280, 320), (1000, 960, 320), (77, 1280, 768), (8192, 320, 320)])
def test_linear_bias_residual(M, N, K):
    x = rnd(M, K, seed=1)
    w = rnd(N, K, scale=K ** -0.5, seed=2)
    b = rnd(N, scale=0.1, seed=3)
    r = rnd(M, N, seed=4)
    out = ops.linear(x, w, b, residual=r)
    ref = x.float() @ w.float().t() + b.float() + r.float()
    close(out, ref)


@pytest.mark.parametrize("act,fn", [(ops.ACT_SILU, F.silu), (ops.ACT_GELU, F.gelu), (ops.ACT_RELU, F.relu)])
def test_linear_act(act, fn):
    x, w, b = rnd(512, 640, seed=5), rnd(1280, 640, scale=640 ** -0.5, seed=6), rnd(1280, scale=0.1, seed=7)
    close(ops.linear(x, w, b, act=act), fn(x.float() @ w.float().t() + b.float()))


def test_linear_strided_views():
    """Row-strided input/output views (zero-copy concat slices, fused QKV columns)."""
    big = rnd(300, 960, seed=8)
    x = big[:, 320:640]
    w = rnd(640, 320, scale=320 ** -0.5, seed=9)
    dst = torch.zeros(300, 1000, dtype=torch.float16, device=DEV)
    ops.linear(x, w, out=dst[:, 200:840])
    close(dst[:, 200:840], x.float() @ w.float().t())
    assert dst[:, :200].abs().max().item() == 0 and dst[:, 840:].abs().max().item() == 0


def test_linear_groupnorm_apply_and_coladd():
    nimg, HW, C, N = 3, 64, 320, 640
    x = rnd(nimg * HW, C, seed=10)
    gamma, beta = rnd(C, scale=0.1, seed=11) + 1, rnd(C, scale=0.1, seed=12)
    sc, sh = ops.groupnorm_stats(x, nimg, HW, gamma, beta, 1e-6, 32)
    w, b = rnd(N, C, scale=C ** -0.5, seed=13), rnd(N, scale=0.1, seed=14)
    col = rnd(nimg, N, seed=15)
    out = ops.linear(x, w, b, gn=(sc, sh, True), rows_per_batch=HW, coladd=col, coladd_bstride=N)
    xn = F.group_norm(x.float().view(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-6)
    xn = F.silu(xn.permute(0, 2, 1).reshape(nimg * HW, C))
    ref = xn @ w.float().t() + b.float() + col.float().repeat_interleave(HW, 0)
    close(out, ref)


def test_linear_wanda_bitmask():
    M, N, K = 256, 320, 1280
    x, w, b = rnd(M, K, seed=16), rnd(N, K, scale=K ** -0.5, seed=17), rnd(N, scale=0.1, seed=18)
    g = torch.Generator().manual_seed(19)
    mask = (torch.rand(N, K, generator=g) < 0.03).to(torch.uint8)
    import numpy as np
    bits = torch.from_numpy(np.packbits(mask.numpy(), axis=-1, bitorder="little")).to(DEV)
    out = ops.linear(x, w, b, wmask_bits=bits)
    ref = x.float() @ (w.float() * (1 - mask.to(DEV).float())).t() + b.float()
    close(out, ref)


def conv_ref(x, nimg, H, W, w, b, stride=1, upsample=False):
    xc = x.float().view(nimg, H, W, -1).permute(0, 3, 1, 2)
    if upsample:
        xc = F.interpolate(xc, scale_factor=2.0, mode="nearest")
    wc = w.float().permute(0, 3, 1, 2)
    y = F.conv2d(xc, wc, b.float(), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


@pytest.mark.parametrize("Cin,Cout,H,stride,up", [(64, 320, 16, 1, False), (320, 320, 16, 1, False),
                                                  (320, 320, 16, 2, False), (640, 640, 8, 1, True),
                                                  (960, 320, 8, 1, False), (320, 8, 16, 1, False),
                                                  (1280, 1280, 8, 1, False)])
def test_conv3x3(Cin, Cout, H, stride, up):
    nimg = 2
    x = rnd(nimg * H * H, Cin, seed=20)
    w = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=21)
    b = rnd(Cout, scale=0.1, seed=22)
    out = ops.conv3x3(x, nimg, H, H, ops.conv_weight(w), b, stride=stride, upsample=up)
    close(out, conv_ref(x, nimg, H, H, w, b, stride, up))


def test_conv3x3_gn_silu_temb_residual():
    nimg, H, Cin, Cout = 2, 16, 320, 640
    x = rnd(nimg * H * H, Cin, seed=23)
    gamma, beta = rnd(Cin, scale=0.1, seed=24) + 1, rnd(Cin, scale=0.1, seed=25)
    sc, sh = ops.groupnorm_stats(x, nimg, H * H, gamma, beta, 1e-5, 32)
    w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=26), rnd(Cout, scale=0.1, seed=27)
    temb = rnd(1, Cout, seed=28)
    res = rnd(nimg * H * H, Cout, seed=29)
    out = ops.conv3x3(x, nimg, H, H, ops.conv_weight(w), b, gn=(sc, sh, True), coladd=temb, coladd_bstride=0, residual=res)
    xn = F.group_norm(x.float().view(nimg, H * H, Cin).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5)
    xn = F.silu(xn).permute(0, 2, 1).reshape(-1, Cin)
    ref = conv_ref(xn, nimg, H, H, w, b) + temb.float() + res.float()
    close(out, ref)


def test_conv3x3_strided_concat_input():
    nimg, H, C1, C2, Cout = 2, 8, 640, 320, 320
    buf = rnd(nimg * H * H, C1 + C2, seed=30)
    w, b = rnd(Cout, 3, 3, C1 + C2, scale=(9 * (C1 + C2)) ** -0.5, seed=31), rnd(Cout, scale=0.1, seed=32)
    close(ops.conv3x3(buf, nimg, H, H, ops.conv_weight(w), b), conv_ref(buf, nimg, H, H, w, b))
    w2 = rnd(Cout, 3, 3, C2, scale=(9 * C2) ** -0.5, seed=33)
    close(ops.conv3x3(buf[:, C1:], nimg, H, H, ops.conv_weight(w2), b), conv_ref(buf[:, C1:].contiguous(), nimg, H, H, w2, b))


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8])
def test_forced_tiles(tile):
    """Every tile configuration of the GEMM kernel (sdmoe_tune knob 1), in all three modes, with ragged M."""
    with tune.tuned(tile=tile):
        x = rnd(1000, 640, seed=40)
        w = rnd(1280, 640, scale=640 ** -0.5, seed=41)
        b = rnd(1280, scale=0.1, seed=42)
        close(ops.linear(x, w, b, act=ops.ACT_GELU), F.gelu(x.float() @ w.float().t() + b.float()))
        for Cin, Cout, H, st, up in [(320, 640, 12, 1, False), (640, 320, 8, 1, True), (320, 320, 12, 2, False)]:
            xi = rnd(2 * H * H, Cin, seed=43)
            wi = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=44)
            bi = rnd(Cout, scale=0.1, seed=45)
            close(ops.conv3x3(xi, 2, H, H, ops.conv_weight(wi), bi, stride=st, upsample=up), conv_ref(xi, 2, H, H, wi, bi, st, up))


@pytest.mark.parametrize("nimg,HW,C,N,mean", [(16, 4096, 320, 320, 0.0), (16, 1024, 640, 640, 0.0), (3, 256, 1280, 1280, 2.0),
                                               (2, 1024, 640, 640, 4.0)])
def test_gn_fold_proj_in(nimg, HW, C, N, mean):
    """Transformer2DModel.norm -> proj_in with the GroupNorm folded into per-image weights (sdmoe_gn_fold +
    sdmoe_linear_per_image) against GroupNorm + Linear in fp32, at the bench's 64x64 / 32x32 shapes (16 images) and
    with a non-zero activation mean (the fold moves -mean*scale into the per-image bias)."""
    x = rnd(nimg * HW, C, seed=50) + mean
    gamma, beta = rnd(C, scale=0.1, seed=51) + 1, rnd(C, scale=0.1, seed=52)
    w, b = rnd(N, C, scale=C ** -0.5, seed=53), rnd(N, scale=0.1, seed=54)
    sc, sh = ops.groupnorm_stats(x, nimg, HW, gamma, beta, 1e-6, 32)
    wf, cb = ops.gn_fold(w, b, sc, sh)
    out = ops.linear_per_image(x, wf, cb, HW)
    xn = F.group_norm(x.float().view(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-6)
    ref = xn.permute(0, 2, 1).reshape(nimg * HW, C) @ w.float().t() + b.float()
    close(out, ref)
    # the folded weights and bias themselves
    close(wf.float(), w.float()[None] * sc[:, None, :], rel=1e-3)
    # (the bias is taken from the ROUNDED weights, b + Wf . (shift / scale), w * shift where |scale| < 2^-14; fp64)
    terms = torch.where((sc.abs() >= 2.0 ** -14)[:, None, :], wf.double() * (sh.double() / sc.double())[:, None, :],
                        w.double()[None] * sh.double()[:, None, :])
    close(cb.double(), b.double()[None] + terms.sum(-1), tol=1e-4, rel=1e-5)
    # with a residual, and the unfused path it replaces agrees to fp16 rounding
    r = rnd(nimg * HW, N, seed=55)
    close(ops.linear_per_image(x, wf, cb, HW, residual=r), ref + r.float())
    unf = ops.linear(ops.groupnorm(x, nimg, HW, gamma, beta, 1e-6, 32), w, b)
    close(out, unf.float())


def test_gn_fold_rejects_straddling_tiles():
    x = rnd(2 * 100, 320, seed=56)
    wf, cb = torch.zeros(2, 320, 320, device=DEV, dtype=torch.float16), torch.zeros(2, 320, device=DEV)
    from sdmoe import _lib
    with pytest.raises(_lib.SdmoeError):
        ops.linear_per_image(x, wf, cb, 100)


@pytest.mark.parametrize("C,HW,eps", [(320, 4096, 1e-5), (960, 256, 1e-6), (2560, 64, 1e-5), (1920, 1024, 1e-5),
                                      (1280, 64, 1e-5), (1280, 256, 1e-5), (640, 1024, 1e-6), (320, 1024, 1e-5),
                                      (640, 2048, 1e-5), (128, 16, 1e-6)])
def test_groupnorm_stats(C, HW, eps):
    """HW <= 1024 takes the single-launch gn_small_kernel, larger HW the partial + finalize pair."""
    nimg = 2
    x = rnd(nimg * HW, C, seed=34) * 2 + 3  # non-zero mean exercises the shifted sums
    gamma, beta = rnd(C, scale=0.1, seed=35) + 1, rnd(C, scale=0.1, seed=36)
    sc, sh = ops.groupnorm_stats(x, nimg, HW, gamma, beta, eps, 32)
    xn = x.float().view(nimg, HW, C) * sc[:, None, :] + sh[:, None, :]
    ref = F.group_norm(x.float().view(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), eps)
    close(xn, ref.permute(0, 2, 1), tol=2e-3)


@pytest.mark.parametrize("C,HW,silu", [(1280, 64, True), (640, 1024, False), (2560, 256, True), (320, 4096, True),
                                       (960, 2048, False)])
def test_groupnorm_fused_apply(C, HW, silu):
    """sdmoe_groupnorm: statistics + apply(+SiLU) in one ABI call, small (HW <= 1024) and large statistics paths."""
    nimg = 3
    buf = rnd(nimg * HW, C + 64, seed=46) * 2 + 1
    x = buf[:, 64:]
    gamma, beta = rnd(C, scale=0.1, seed=47) + 1, rnd(C, scale=0.1, seed=48)
    y = ops.groupnorm(x, nimg, HW, gamma, beta, 1e-5, 32, silu)
    ref = F.group_norm(x.float().reshape(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5)
    ref = ref.permute(0, 2, 1).reshape(nimg * HW, C)
    if silu:
        ref = F.silu(ref)
    close(y, ref, tol=5e-3)
    sc, sh = ops.groupnorm_stats(x, nimg, HW, gamma, beta, 1e-5, 32)
    ap = ops.groupnorm_apply(x, nimg, HW, sc, sh, silu)
    assert (y.float() - ap.float()).abs().max().item() <= 2e-3 * max(1.0, ap.float().abs().max().item())


def test_groupnorm_stats_channel_slice():
    """A channel slice of a wider buffer (the zero-copy skip concatenation), small and large paths."""
    for HW in (256, 4096):
        nimg, C = 2, 640
        buf = rnd(nimg * HW, C + 320, seed=40) * 2 - 1
        x = buf[:, 320:]
        gamma, beta = rnd(C, scale=0.1, seed=41) + 1, rnd(C, scale=0.1, seed=42)
        sc, sh = ops.groupnorm_stats(x, nimg, HW, gamma, beta, 1e-5, 32)
        xn = x.float().reshape(nimg, HW, C) * sc[:, None, :] + sh[:, None, :]
        ref = F.group_norm(x.float().reshape(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5)
        close(xn, ref.permute(0, 2, 1), tol=2e-3)


@pytest.mark.parametrize("C", [320, 640, 1280])
def test_layernorm(C):
    x = rnd(777, C, seed=37) * 3 + 1
    g, b = rnd(C, scale=0.1, seed=38) + 1, rnd(C, scale=0.1, seed=39)
    close(ops.layernorm(x, g, b, 1e-5), F.layer_norm(x.float(), (C,), g.float(), b.float(), 1e-5), tol=5e-3)


@pytest.mark.parametrize("d,Nq,Nk", [(40, 256, 256), (40, 4096, 77), (80, 1024, 1024), (80, 200, 77),
                                     (160, 256, 256), (160, 64, 77), (64, 300, 300)])
def test_attention(d, Nq, Nk):
    nimg, heads = 2, 8
    C = heads * d
    qkv = rnd(nimg * Nq, 3 * C, seed=40)
    kv = rnd(nimg * Nk, 2 * C, seed=41)
    if Nk == Nq:
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    else:
        q, k, v = qkv[:, :C], kv[:, :C], kv[:, C:]
    out = ops.attention(q, k, v, nimg, Nq, Nk, heads)
    qf = q.float().reshape(nimg, Nq, heads, d).transpose(1, 2)
    kf = k.float().reshape(nimg, Nk, heads, d).transpose(1, 2)
    vf = v.float().reshape(nimg, Nk, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(nimg * Nq, C)
    close(out, ref)


@pytest.mark.parametrize("variant", [1, 2, 4, 8, 9])
@pytest.mark.parametrize("d,Nq,Nk", [(40, 256, 256), (40, 300, 77), (80, 200, 200), (64, 300, 300),
                                     (32, 130, 130), (40, 64, 50), (40, 1000, 4096), (40, 520, 128)])
def test_attention_forced_variant(variant, d, Nq, Nk):
    """Every attention kernel variant (sdmoe_tune knob 4: 1 = 32x32x16 kernel, 2 / 4 = 16x16x32 kernel with 32 / 64
    queries per wave, 8 = 16x16x32 kernel in 8-wave workgroups, 9 = 32x32x16 kernel in 8-wave workgroups), ragged Nq
    and Nk, single-tile and exactly-whole-tile key counts."""
    nimg, heads = 2, 4
    C = heads * d
    q = rnd(nimg * Nq, C, seed=60)
    kv = rnd(nimg * Nk, 2 * C, seed=61)
    k, v = kv[:, :C], kv[:, C:]
    with tune.tuned(attn=variant):
        out = ops.attention(q, k, v, nimg, Nq, Nk, heads)
    qf = q.float().reshape(nimg, Nq, heads, d).transpose(1, 2)
    kf = k.float().reshape(nimg, Nk, heads, d).transpose(1, 2)
    vf = v.float().reshape(nimg, Nk, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(nimg * Nq, C)
    close(out, ref)


@pytest.mark.parametrize("d,variant", [(80, 0), (40, 0), (40, 8), (40, 9), (40, 1)])
def test_attention_peaked_softmax(d, variant):
    """A spiked key forces the online-softmax rescale branch at a later tile."""
    nimg, heads, N = 1, 8, 512
    C = heads * d
    q = rnd(nimg * N, C, seed=42)
    k = rnd(nimg * N, C, seed=43)
    k[300] = q[5] * 4  # query 5 now peaks at key 300 (tile 4)
    v = rnd(nimg * N, C, seed=44)
    with tune.tuned(attn=variant):
        out = ops.attention(q, k, v, nimg, N, N, heads)
    qf = q.float().view(1, N, heads, d).transpose(1, 2)
    kf = k.float().view(1, N, heads, d).transpose(1, 2)
    vf = v.float().view(1, N, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(N, C)
    close(out, ref)


def test_timestep_embedding():
    import sys, os  # noqa: E401
    from oracle.unet_ref import timestep_embedding
    for t in (1.0, 481.0, 981.0):
        out = ops.timestep_embedding(t, 320, DEV)
        close(out, timestep_embedding(t, 320).to(DEV), tol=2e-3)


def test_cfg_ddim_step_and_prepare():
    B, H = 2, 16
    lat = rnd(B, 4, H, H, dtype=torch.float32, seed=45)
    eps = rnd(2 * B * H * H, 8, seed=46)
    x_in = torch.zeros(2 * B * H * H, 64, dtype=torch.float16, device=DEV)
    ops.prepare_input(lat, x_in, 2)
    ref_in = lat.permute(0, 2, 3, 1).reshape(B * H * H, 4)
    close(x_in[:B * H * H, :4], ref_in, tol=1e-3)
    close(x_in[B * H * H:, :4], ref_in, tol=1e-3)
    assert x_in[:, 4:].abs().max().item() == 0
    a_t, a_p, g = 0.3, 0.5, 7.5
    e = eps.float()[:, :4].reshape(2, B, H, H, 4).permute(0, 1, 4, 2, 3)
    ee = e[0] + g * (e[1] - e[0])
    x0 = (lat - math.sqrt(1 - a_t) * ee) / math.sqrt(a_t)
    ref = math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * ee
    ops.cfg_ddim_step(eps, lat, True, g, a_t, a_p, next_in=x_in)
    close(lat, ref, tol=1e-4)
    next_ref = lat.permute(0, 2, 3, 1).reshape(B * H * H, 4).half()
    assert torch.equal(x_in[:B * H * H, :4], next_ref) and torch.equal(x_in[B * H * H:, :4], next_ref)
    assert x_in[:, 4:].abs().max().item() == 0


# ---- the bench workload's exact shapes (SD-1.4 512^2, U-Net batch 16: 64x64 latents = 65,536 rows) ----------

@pytest.mark.parametrize("d,N", [(40, 4096), (64, 4096)])
def test_attention_full_size(d, N):
    """Self-attention at the metric's N = 4096 tokens (d = 40: SD-1.4 64x64 level; d = 64: SDXL-base), 8 heads,
    2 images (the kernel's grid is per (image, head), so more images only repeat these blocks)."""
    nimg, heads = 2, 8
    C = heads * d
    qkv = rnd(nimg * N, 3 * C, seed=50 + d)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    out = ops.attention(q, k, v, nimg, N, N, heads)
    qf = q.float().reshape(nimg, N, heads, d).transpose(1, 2)
    kf = k.float().reshape(nimg, N, heads, d).transpose(1, 2)
    vf = v.float().reshape(nimg, N, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(nimg * N, C)
    close(out, ref)


# tiles (sdmoe_tune knob 1): 0 auto, 1 = 128x160, 2 = 64x160, 3 = 256x320 (2x4 waves), 4 = 256x160 (4x2), 5 = 256x320
# (4x2), 7 = 128x160 (4x2, 8 waves), 8 = 64x320 (2x4, 8 waves); stages (knob 0): 0 auto, 2, 3 -- every ring the
# M = 65,536 problems can take
FULL_TILES = [(t, s) for t in (0, 1, 2, 3, 4, 5, 7, 8) for s in (0, 2, 3)]


@pytest.mark.parametrize("tile,stages", FULL_TILES)
def test_linear_full_size_tiles(tile, stages):
    """The 25 per-evaluation [65536, 320] x [320, 320] projections (+bias +residual) on every tile / stage ring."""
    M, N, K = 65536, 320, 320
    x, w = rnd(M, K, seed=60), rnd(N, K, scale=K ** -0.5, seed=61)
    b, r = rnd(N, scale=0.1, seed=62), rnd(M, N, seed=63)

    with tune.tuned(tile=tile, stages=stages):
        close(ops.linear(x, w, b, residual=r), x.float() @ w.float().t() + b.float() + r.float())


@pytest.mark.parametrize("tile,stages", FULL_TILES)
def test_conv3x3_full_size_tiles(tile, stages):
    """The 64x64 320->320 ResNet conv at U-Net batch 16 (M = 65,536, K = 2,880) with the time-embedding column
    add and residual epilogue, on every tile / stage ring."""
    nimg, H, C = 16, 64, 320
    x = rnd(nimg * H * H, C, seed=64)
    w, b = rnd(C, 3, 3, C, scale=(9 * C) ** -0.5, seed=65), rnd(C, scale=0.1, seed=66)
    temb, res = rnd(1, C, seed=67), rnd(nimg * H * H, C, seed=68)

    with tune.tuned(tile=tile, stages=stages):
        out = ops.conv3x3(x, nimg, H, H, ops.conv_weight(w), b, coladd=temb, coladd_bstride=0, residual=res)
        close(out, conv_ref(x, nimg, H, H, w, b) + temb.float() + res.float())


@pytest.mark.parametrize("H,Cin,Cout,nimg,up", [(64, 320, 320, 16, False), (64, 960, 320, 2, False),
                                                (64, 64, 320, 2, False), (32, 640, 640, 16, False),
                                                (32, 1280, 640, 4, False), (32, 320, 640, 2, False),
                                                (16, 1280, 1280, 16, False), (16, 2560, 1280, 2, False),
                                                (16, 640, 1280, 3, False), (32, 640, 640, 16, True),
                                                (32, 640, 640, 2, True), (16, 1280, 1280, 16, True),
                                                (16, 1280, 1280, 2, True), (8, 1280, 1280, 3, True)])
def test_conv3x3_halo_tiles(H, Cin, Cout, nimg, up):
    """Halo-tiled stride-1 convs (MODE_CONVH64/32/16 and the 2x-upsample MODE_CONVHUP64/32/16, every sdmoe_tune knob 16
    setting): the input halo of each 32-channel slice staged once for the 9 taps, incl. image borders, K split over
    slices (small grids: nimg 2-4) and the time-embedding column add + residual epilogue; vs torch fp32 and vs the
    shifted-tile path (knob 16 = 0) within the same tolerance (the K order differs: 32- vs 64-channel slices)."""
    OH = 2 * H if up else H
    x = rnd(nimg * H * H, Cin, seed=H + Cin)
    w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=H + Cout), rnd(Cout, scale=0.1, seed=3)
    temb, res = rnd(nimg, Cout, seed=4), rnd(nimg * OH * OH, Cout, seed=5)
    ref = conv_ref(x, nimg, H, H, w, b, 1, up)
    if not up:
        ref = ref + temb.float().repeat_interleave(H * H, 0) + res.float()
    wc = ops.conv_weight(w)
    outs = []
    kw = {} if up else dict(coladd=temb, coladd_bstride=Cout, residual=res)
    # 1 default (64-wide at <= 32 tiles: 128-row tiles); 2: the 128-row halo tiles the default leaves off; 3: 32-wide
    # outputs on 256-row tiles; 0: shifted
    for halo in (1, 2, 3, 0):
        with tune.tuned(halo=halo):
            outs.append(ops.conv3x3(x, nimg, H, H, wc, b, upsample=up, **kw))
    for o in outs:
        close(o, ref)
    for o in outs[:3]:
        close(o, outs[3].float())


@pytest.mark.parametrize("Cout,narrow", [(8, 1), (8, 0), (16, 1), (32, 1), (24, 1)])
def test_conv3x3_narrow_outputs(Cout, narrow):
    """conv_out's shape (320 -> 8 padded channels at 64x64) on the 128x32 tile (sdmoe_tune knob 21 = 1, default) and on
    128x64 (0): vs torch fp32, bias and an M tail (3 images of 10x10)."""
    for nimg, H, Cin in [(2, 64, 320), (3, 10, 128)]:
        x = rnd(nimg * H * H, Cin, seed=Cout + H)
        w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=Cout), rnd(Cout, scale=0.1, seed=Cout + 1)
        with tune.tuned(narrow=narrow):
            out = ops.conv3x3(x, nimg, H, H, ops.conv_weight(w), b)
        close(out, conv_ref(x, nimg, H, H, w, b))


@pytest.mark.parametrize("Cin,Cout,Cin2,nimg,res", [(320, 320, 0, 16, True), (960, 320, 0, 2, False), (640, 320, 0, 3, False),
                                                   (320, 320, 640, 2, False), (320, 320, 960, 16, False)])
def test_conv3x3_groupnorm_in_kernel_bit_identical(Cin, Cout, Cin2, nimg, res):
    """sdmoe_conv3x3_gn (GroupNorm + SiLU applied to each staged halo slice inside the conv: 64-wide tiles) vs
    sdmoe_groupnorm_apply + sdmoe_conv3x3(_sc): bit-identical output (same normalisation arithmetic, same conv K
    order), incl. the folded shortcut, the residual / time-embedding epilogue, a concat-buffer input (row stride >
    Cin) and K split over slices (nimg 2-3); vs torch fp32 within the kernel tolerance."""
    H = 64
    buf = rnd(nimg * H * H, Cin + 64, seed=Cin + Cin2) * 2 + 0.5
    x = buf[:, 64:]
    gamma, beta = rnd(Cin, scale=0.1, seed=1) + 1, rnd(Cin, scale=0.1, seed=2)
    sc, sh = ops.groupnorm_stats(x, nimg, H * H, gamma, beta, 1e-5, 32)
    w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=3), rnd(Cout, scale=0.1, seed=4)
    temb = rnd(1, Cout, seed=5)
    r = rnd(nimg * H * H, Cout, seed=6) if res else None
    x2 = rnd(nimg * H * H, Cin2, seed=7) if Cin2 else None
    if Cin2:
        w2 = rnd(Cout, Cin2, scale=Cin2 ** -0.5, seed=8)
        wc = ops.conv_weight_with_shortcut(ops.conv_weight(w), w2)
        kw = dict(shortcut=x2)
    else:
        wc = ops.conv_weight(w)
        kw = dict(coladd=temb, coladd_bstride=0, residual=r)
    assert ops.conv_gn_fusable(H, H, Cin, Cout)
    fused = ops.conv3x3(x, nimg, H, H, wc, b, gn=(sc, sh, True), **kw)
    xn = ops.groupnorm_apply(x, nimg, H * H, sc, sh, True)
    plain = ops.conv3x3(xn, nimg, H, H, wc, b, **kw)
    assert torch.equal(fused, plain)
    xr = F.silu(F.group_norm(x.float().view(nimg, H * H, Cin).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5))
    ref = conv_ref(xr.permute(0, 2, 1).reshape(-1, Cin), nimg, H, H, w, b)
    if Cin2:
        ref = ref + x2.float() @ w2.float().t()
    else:
        ref = ref + temb.float() + (r.float() if res else 0)
    close(fused, ref)


@pytest.mark.parametrize("H,C,nimg", [(32, 640, 2), (16, 1280, 2), (8, 1280, 3)])
@pytest.mark.parametrize("ks", [1, 2, 5, 20])
def test_conv3x3_halo_upsample_forced_splits(H, C, nimg, ks):
    """The 2x-upsample halo convs (MODE_CONVHUP*) at forced split-K counts (knob 9): 1 .. all slices per workgroup;
    vs torch fp32 (nearest upsample, then the 3x3 conv)."""
    x = rnd(nimg * H * H, C, seed=H + ks)
    w, b = rnd(C, 3, 3, C, scale=(9 * C) ** -0.5, seed=H + 1), rnd(C, scale=0.1, seed=H + 2)
    with tune.tuned(ksplit=ks):
        out = ops.conv3x3(x, nimg, H, H, ops.conv_weight(w), b, upsample=True)
    close(out, conv_ref(x, nimg, H, H, w, b, 1, True))


@pytest.mark.parametrize("Cin,Cin2", [(320, 640), (640, 0)])
@pytest.mark.parametrize("ks", [1, 2, 3, 7, 10])
def test_conv3x3_groupnorm_in_kernel_forced_splits(Cin, Cin2, ks):
    """The in-kernel GroupNorm halo conv at forced split-K counts (knob 9): the next slice is normalised at tap 5 only
    in slices with a successor, the first in the prologue -- with 1 .. all slices per workgroup both paths run at
    every count. Bit-identical to sdmoe_groupnorm_apply + the plain halo conv under the same split."""
    H, nimg, Cout = 64, 2, 320
    x = rnd(nimg * H * H, Cin, seed=Cin + ks) * 2 + 0.5
    gamma, beta = rnd(Cin, scale=0.1, seed=11) + 1, rnd(Cin, scale=0.1, seed=12)
    sc, sh = ops.groupnorm_stats(x, nimg, H * H, gamma, beta, 1e-5, 32)
    w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=13), rnd(Cout, scale=0.1, seed=14)
    if Cin2:
        x2 = rnd(nimg * H * H, Cin2, seed=15)
        wc = ops.conv_weight_with_shortcut(ops.conv_weight(w), rnd(Cout, Cin2, scale=Cin2 ** -0.5, seed=16))
        kw = dict(shortcut=x2)
    else:
        wc, kw = ops.conv_weight(w), dict(residual=rnd(nimg * H * H, Cout, seed=17))
    with tune.tuned(ksplit=ks):
        fused = ops.conv3x3(x, nimg, H, H, wc, b, gn=(sc, sh, True), **kw)
        unfused = ops.conv3x3(ops.groupnorm_apply(x, nimg, H * H, sc, sh, True), nimg, H, H, wc, b, **kw)
    assert torch.equal(fused, unfused)


def test_conv3x3_full_size_upsample_concat():
    """The 32x32 -> 64x64 upsample conv (640 ch) and a 64x64 skip-concat conv input (960 -> 320) at batch 16."""
    nimg = 16
    x = rnd(nimg * 32 * 32, 640, seed=69)
    w, b = rnd(640, 3, 3, 640, scale=(9 * 640) ** -0.5, seed=70), rnd(640, scale=0.1, seed=71)
    close(ops.conv3x3(x, nimg, 32, 32, ops.conv_weight(w), b, upsample=True), conv_ref(x, nimg, 32, 32, w, b, 1, True))
    buf = rnd(nimg * 64 * 64, 960, seed=72)
    w2 = rnd(320, 3, 3, 960, scale=(9 * 960) ** -0.5, seed=73)
    close(ops.conv3x3(buf, nimg, 64, 64, ops.conv_weight(w2), b[:320]), conv_ref(buf, nimg, 64, 64, w2, b[:320]))


@pytest.mark.parametrize("C,HW", [(320, 4096), (640, 4096), (960, 4096)])
def test_groupnorm_full_size(C, HW):
    """GroupNorm(32) statistics + apply(+SiLU) at the bench's 16 images x 4096 positions (the partial/finalize path)."""
    nimg = 16
    x = rnd(nimg * HW, C, seed=74) * 2 + 1
    gamma, beta = rnd(C, scale=0.1, seed=75) + 1, rnd(C, scale=0.1, seed=76)
    y = ops.groupnorm(x, nimg, HW, gamma, beta, 1e-5, 32, True)
    ref = F.group_norm(x.float().reshape(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5)
    close(y, F.silu(ref.permute(0, 2, 1).reshape(nimg * HW, C)), tol=5e-3)


@pytest.mark.parametrize("M,C,E,tile", [(65536, 320, 64, 0), (65536, 320, 64, 1), (65536, 320, 64, 7),
                                        (512, 1280, 256, 0)])
def test_geglu_fused_full_size(M, C, E, tile):
    """The 64x64 level's fused projection + ReLU GEGLU + expert scores at M = 65,536 (F = 1280, 64 experts of 20)
    against the unfused projection GEMM + route kernel: bit-identical, on the auto tile and the 128x160 4- and
    8-wave tiles; and the 16x16 level at one prompt (M = 512, F = 5120: the auto rule's 8-wave 128x160 tiles)."""
    F_ = 4 * C
    g = torch.Generator().manual_seed(77)
    x = torch.randn(M, C, generator=g).half().to(DEV)
    w = (torch.randn(2 * F_, C, generator=g) * C ** -0.5).half().to(DEV)
    b = (torch.randn(2 * F_, generator=g) * 0.3).half().to(DEV)
    routing = ops.Routing(torch.randperm(F_, generator=g) % E, E, 12, DEV)
    w_il, b_il = ops.interleave_geglu(w, b, routing.perm)
    score = torch.empty((M, E), dtype=torch.float16, device=DEV)
    with tune.tuned(tile=tile):
        P = ops.linear_geglu(x, w_il, b_il, ops.ACT_RELU, score=score, esize=routing.esize)
    score_u = torch.empty_like(score)
    out_u = ops.geglu_route(ops.linear(x, w, b), routing, ops.ACT_RELU, score_out=score_u, k=E)
    assert torch.equal(score, score_u)
    assert torch.equal(P, out_u[:, routing.perm.to(DEV)])


# ---- LayerNorm folded into the consuming GEMM (sdmoe_ln_fold + sdmoe_linear_ln / sdmoe_linear_geglu_ln) ---------

def _ln_ref(x, gamma, beta, eps=1e-5):
    return F.layer_norm(x.float(), (x.shape[1],), gamma.float(), beta.float(), eps)


@pytest.mark.parametrize("M,N,K", [(65536, 960, 320), (65536, 320, 320), (16384, 1920, 640), (16384, 640, 640),
                                   (4096, 3840, 1280), (4096, 1280, 1280), (1024, 1280, 1280), (1000, 960, 320),
                                   (77, 640, 640)])
def test_linear_ln(M, N, K):
    """LN(x) @ W^T (+ bias) with the norm folded into the GEMM vs torch fp32 LayerNorm + linear; rows carry a
    per-row offset (mean/std up to ~4) so the folded mean correction is exercised. Covers every tile the QKV / Q
    projections take at the bench's shapes (256x320, 128x160, 64x160) and M tails."""
    x = rnd(M, K, seed=81) + rnd(M, 1, scale=2.0, seed=82)
    gamma, beta = rnd(K, scale=0.2, seed=83) + 1, rnd(K, scale=0.2, seed=84)
    w = rnd(N, K, scale=K ** -0.5, seed=85)
    b = rnd(N, scale=0.1, seed=86)
    for bias in (None, b):
        fold = ops.LNFold(w, gamma, beta, 1e-5, bias)
        out = ops.linear_ln(x, fold)
        ref = _ln_ref(x, gamma, beta) @ w.float().t() + (0 if bias is None else bias.float())
        close(out, ref)


def test_ln_fold_operands():
    """sdmoe_ln_fold: Wf = fp16(W*gamma), wsum = rowsum(Wf) and bias_f = bias + W beta (fp32)."""
    N, K = 640, 1280
    w, gamma, beta, b = rnd(N, K, seed=87), rnd(K, seed=88), rnd(K, seed=89), rnd(N, seed=90)
    f = ops.LNFold(w, gamma, beta, 1e-5, b)
    assert torch.equal(f.w, (w.float() * gamma.float()).half())
    torch.testing.assert_close(f.wsum, f.w.float().sum(1), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(f.bias, b.float() + w.float() @ beta.float(), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("M,C", [(65536, 320), (16384, 640), (4096, 1280), (1000, 320)])
def test_linear_geglu_ln(M, C):
    """The routed-GEGLU projection with norm3 folded in vs LayerNorm + the unfused projection + route kernel
    (torch fp32 reference of the product; expert scores within the same tolerance)."""
    F_, E = 4 * C, C // 5
    g = torch.Generator().manual_seed(91)
    x = (torch.randn(M, C, generator=g) + torch.randn(M, 1, generator=g) * 2).half().to(DEV)
    gamma = (torch.randn(C, generator=g) * 0.2 + 1).half().to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).half().to(DEV)
    w = (torch.randn(2 * F_, C, generator=g) * C ** -0.5).half().to(DEV)
    b = (torch.randn(2 * F_, generator=g) * 0.3).half().to(DEV)
    routing = ops.Routing(torch.randperm(F_, generator=g) % E, E, 12, DEV)
    fold = ops.interleave_ln_fold(ops.LNFold(w, gamma, beta, 1e-5, b), routing.perm)
    score = torch.empty((M, E), dtype=torch.float16, device=DEV)
    P = ops.linear_geglu(x, None, None, ops.ACT_RELU, score=score, esize=routing.esize, ln=fold)
    y = _ln_ref(x, gamma, beta) @ w.float().t() + b.float()
    ref = y[:, :F_] * F.relu(y[:, F_:])
    perm = routing.perm.to(DEV)
    close(P, ref[:, perm])
    sref = F.relu(y[:, F_:])[:, perm].reshape(M, E, F_ // E).sum(-1)
    close(score, sref)


def test_transformer_block_ln_folded_vs_explicit():
    """A whole SD-1.4 BasicTransformerBlock (64x64 level, 16 images, relufied MoE-routed FFN) with the three
    LayerNorms folded into their GEMMs vs the explicit sdmoe_layernorm path. top-k = all experts, so no near-tie
    selection flip can separate the two; the routed top-k path is covered against the oracle by the bench-workload
    pipeline test (tests/test_gpu_unet.py), which runs with the fold on."""
    from sdmoe import unet as U
    from sdmoe.config import UNetConfig
    from sdmoe.weights import make_state_dict
    from moefication.helper import moefy_synthetic
    from sdmoe.pipeline import StableDiffusionPipeline
    cfg = UNetConfig.sd14(64)
    pipe = StableDiffusionPipeline.synthetic(cfg, seed=0, device=DEV, num_inference_steps=1)
    moefy_synthetic(pipe, 1.0, 20, seed=0)
    blk = pipe.unet.down_blocks[0].attentions[0].transformer_blocks[0]
    nimg, N, C = 16, 4096, 320
    hs = rnd(nimg * N, C, seed=92) + rnd(nimg * N, 1, scale=1.0, seed=93)
    ctx = rnd(nimg * 77, 768, seed=94)
    outs = []
    try:
        for fused, ffn in ((True, True), (True, False), (False, False)):
            U.FUSED_LN, U.FUSED_LN_FFN = fused, ffn
            outs.append(blk.run(hs.clone(), nimg, N, ctx).float())
    finally:
        U.FUSED_LN, U.FUSED_LN_FFN = True, False
    for o in outs[:2]:
        rel = ((o - outs[2]).norm() / outs[2].norm()).item()
        assert rel < 2e-3, rel


@pytest.mark.parametrize("H,C", [(32, 640), (32, 1280), (16, 1280), (16, 2560), (8, 1280), (8, 2560), (32, 960),
                                 (16, 1920)])
def test_groupnorm_small_bench_shapes(H, C):
    """gn_small_kernel (single-launch statistics) at the bench's small latents, 16 images, + apply(+SiLU)."""
    nimg, HW = 16, H * H
    x = rnd(nimg * HW, C, seed=95) * 2 + 1
    gamma, beta = rnd(C, scale=0.1, seed=96) + 1, rnd(C, scale=0.1, seed=97)
    y = ops.groupnorm(x, nimg, HW, gamma, beta, 1e-5, 32, True)
    ref = F.group_norm(x.float().reshape(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5)
    close(y, F.silu(ref.permute(0, 2, 1).reshape(nimg * HW, C)), tol=5e-3)


@pytest.mark.parametrize("HW,C,nimg,silu", [(1024, 640, 16, True), (1024, 320, 16, False), (1024, 1920, 16, True),
                                            (256, 1280, 16, True), (256, 2560, 16, True), (256, 640, 5, False),
                                            (64, 1280, 16, True), (64, 2560, 16, True), (64, 1280, 3, False),
                                            (16, 128, 2, True), (1024, 960, 2, True),
                                            # chunk widths with nq = WC/8 > 16 (rows 16.. of the
                                            # per-chunk reduction were skipped)
                                            (64, 576, 3, True), (64, 1152, 2, True), (16, 1600, 2, False)])
def test_groupnorm_single_launch_bit_identical(HW, C, nimg, silu):
    """The single-launch kernels (statistics + apply, HW <= 256: gn_fused_reg_kernel, knob 7 = 1, and
    gn_fused_kernel, knob 7 = 2) vs the two-launch path (gn_small_kernel + gn_apply_kernel, knob 7 = 0): the same
    sums in the same order, the same fp64 finalize and the same fp32 scale/shift, so the outputs are bit-identical;
    strided input/output views."""
    buf = rnd(nimg * HW, C + 64, seed=HW + C) * 2 + 1
    x = buf[:, 64:]
    gamma, beta = rnd(C, scale=0.1, seed=C + 1) + 1, rnd(C, scale=0.1, seed=C + 2)
    outs = []
    for mode in (1, 2, 0):
        with tune.tuned(gn_fused=mode):
            dst = torch.full((nimg * HW, C + 16), 7.0, dtype=torch.float16, device=DEV)
            ops.groupnorm(x, nimg, HW, gamma, beta, 1e-5, 32, silu, out=dst[:, 8:8 + C])
            outs.append(dst)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])
    assert (outs[0][:, :8] == 7).all() and (outs[0][:, 8 + C:] == 7).all()
    ref = F.group_norm(x.float().reshape(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5)
    ref = ref.permute(0, 2, 1).reshape(nimg * HW, C)
    close(outs[0][:, 8:8 + C], F.silu(ref) if silu else ref, tol=5e-3)


@pytest.mark.parametrize("HW,C,nimg,silu", [(1024, 640, 16, True), (1024, 1920, 16, True), (1024, 2560, 3, False),
                                            (4096, 320, 16, True), (300, 960, 5, True), (2048, 640, 1, False),
                                            (1024, 1280, 2, True)])
def test_groupnorm_large_latents(HW, C, nimg, silu):
    """sdmoe_groupnorm above 256 positions (statistics kernels + gn_apply_kernel) vs torch fp32, into a strided output
    view whose neighbouring columns must stay untouched; row tails (HW % 32 != 0) and C > 2048."""
    buf = rnd(nimg * HW, C + 64, seed=HW + C + 5) * 2 + 1
    x = buf[:, 64:]
    gamma, beta = rnd(C, scale=0.1, seed=C + 3) + 1, rnd(C, scale=0.1, seed=C + 4)
    dst = torch.full((nimg * HW, C + 16), 7.0, dtype=torch.float16, device=DEV)
    ops.groupnorm(x, nimg, HW, gamma, beta, 1e-5, 32, silu, out=dst[:, 8:8 + C])
    assert (dst[:, :8] == 7).all() and (dst[:, 8 + C:] == 7).all()
    ref = F.group_norm(x.float().reshape(nimg, HW, C).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5)
    ref = ref.permute(0, 2, 1).reshape(nimg * HW, C)
    close(dst[:, 8:8 + C], F.silu(ref) if silu else ref, tol=5e-3)


@pytest.mark.parametrize("H,C,Cin2,nimg", [(64, 320, 960, 2), (64, 320, 640, 3), (32, 640, 1920, 4), (32, 640, 320, 3),
                                           (16, 1280, 2560, 16), (16, 1280, 640, 5), (8, 1280, 2560, 16),
                                           (8, 1280, 1920, 3)])
def test_conv3x3_folded_shortcut(H, C, Cin2, nimg):
    """sdmoe_conv3x3_sc: conv2(hn) + conv_shortcut(x) (+ bias, per-image column add) as one implicit GEMM vs torch
    fp32 conv2d + 1x1 projection, at the U-Net's shortcut shapes (incl. the split-K 16x16 / 8x8 levels, M tails
    and a channel-slice shortcut input)."""
    hn = rnd(nimg * H * H, C, seed=101)
    buf = rnd(nimg * H * H, Cin2 + 64, seed=102)
    x = buf[:, 64:]  # row stride > Cin2, like the concatenation buffers
    w = rnd(C, C, 3, 3, scale=(9 * C) ** -0.5, seed=103)
    wsc = rnd(C, Cin2, scale=Cin2 ** -0.5, seed=104)
    b = rnd(C, scale=0.1, seed=105)
    cadd = rnd(nimg, C, scale=0.1, seed=106)
    wcat = ops.conv_weight_with_shortcut(ops.conv_weight_from_torch(w), wsc)
    out = ops.conv3x3(hn, nimg, H, H, wcat, b, shortcut=x, coladd=cadd, coladd_bstride=C)
    xi = hn.float().reshape(nimg, H, H, C).permute(0, 3, 1, 2)
    ref = F.conv2d(xi, w.float(), b.float(), padding=1).permute(0, 2, 3, 1).reshape(-1, C)
    ref = ref + x.float() @ wsc.float().t() + cadd.float().repeat_interleave(H * H, 0)
    close(out, ref)



@pytest.mark.parametrize("H,C,Cin2,nimg", [(64, 320, 640, 2), (32, 640, 960, 2), (16, 1280, 2560, 2)])
@pytest.mark.parametrize("ks", [1, 2, 3, 4, 7, 10, 20])
def test_conv3x3_halo_forced_splits(H, C, Cin2, nimg, ks):
    """Halo convs with the folded shortcut at forced split-K counts (sdmoe_tune knob 9): 1..20 splits leave each
    workgroup from one to all of its 32-channel main slices and from one to all of the shortcut's steps, so every wait
    regime of the halo loop -- compile-time counts in slices with a successor, in taps 0-6 of the last slice and in the
    shortcut steps but the last two, run-time counts elsewhere -- runs at every slice count; vs torch fp32 (any
    missed LDS-DMA wait reads a stale or half-landed tile: garbage, far outside the tolerance)."""
    hn = rnd(nimg * H * H, C, seed=111 + ks)
    x = rnd(nimg * H * H, Cin2, seed=112)
    w = rnd(C, C, 3, 3, scale=(9 * C) ** -0.5, seed=113)
    wsc = rnd(C, Cin2, scale=Cin2 ** -0.5, seed=114)
    b = rnd(C, scale=0.1, seed=115)
    wcat = ops.conv_weight_with_shortcut(ops.conv_weight_from_torch(w), wsc)
    with tune.tuned(ksplit=ks):
        out = ops.conv3x3(hn, nimg, H, H, wcat, b, shortcut=x)
    xi = hn.float().reshape(nimg, H, H, C).permute(0, 3, 1, 2)
    ref = F.conv2d(xi, w.float(), b.float(), padding=1).permute(0, 2, 3, 1).reshape(-1, C)
    close(out, ref + x.float() @ wsc.float().t())


@pytest.mark.parametrize("kind", ["linear", "linear_res", "linear_ln", "conv_temb", "conv_halo_sc", "keep", "per_image"])
def test_direct_epilogue_bit_identical(kind):
    """fp16 epilogue stored straight from the MFMA fragments (sdmoe_tune knob 23 = 2: two v_permlane16_swap per
    fragment pair, 16-B row pieces) vs the LDS-staged copy-out (knob 23 = 0): bit-identical outputs, M / N tails,
    strided output views; the default (1) takes the direct path only without a residual."""
    g = 16
    outs = []

    def run():
        if kind in ("linear", "linear_res"):
            M, N, K = 1000, 968, 320
            x, w, b = rnd(M, K, seed=g), rnd(N, K, scale=K ** -0.5, seed=g + 1), rnd(N, scale=0.1, seed=g + 2)
            r = rnd(M, N, seed=g + 3) if kind == "linear_res" else None
            dst = torch.full((M, N + 24), 3.0, dtype=torch.float16, device=DEV)
            ops.linear(x, w, b, residual=r, out=dst[:, 8:8 + N])
            return dst
        if kind == "linear_ln":
            M, N, K = 777, 640, 320
            x = rnd(M, K, seed=g) * 2 + 1
            w, b = rnd(N, K, scale=K ** -0.5, seed=g + 1), rnd(N, scale=0.1, seed=g + 2)
            gamma, beta = rnd(K, scale=0.1, seed=g + 3) + 1, rnd(K, scale=0.1, seed=g + 4)
            fold = ops.LNFold(w, gamma, beta, 1e-5, bias=b)
            return ops.linear_ln(x, fold)
        if kind == "conv_temb":
            nimg, H, C = 3, 32, 640
            x = rnd(nimg * H * H, C, seed=g)
            w, b = rnd(C, 3, 3, C, scale=(9 * C) ** -0.5, seed=g + 1), rnd(C, scale=0.1, seed=g + 2)
            temb = rnd(nimg, C, seed=g + 3)
            return ops.conv3x3(x, nimg, H, H, ops.conv_weight(w), b, coladd=temb, coladd_bstride=C)
        if kind == "conv_halo_sc":
            nimg, H, C, C2 = 2, 64, 320, 640
            x, x2 = rnd(nimg * H * H, C, seed=g), rnd(nimg * H * H, C2, seed=g + 5)
            w, w2 = rnd(C, 3, 3, C, scale=(9 * C) ** -0.5, seed=g + 1), rnd(C, C2, scale=C2 ** -0.5, seed=g + 6)
            wc = ops.conv_weight_with_shortcut(ops.conv_weight(w), w2)
            return ops.conv3x3(x, nimg, H, H, wc, rnd(C, scale=0.1, seed=g + 2), shortcut=x2)
        if kind == "keep":
            M, F, N, E = 4096, 1280, 320, 64
            routing = ops.Routing(torch.arange(F) % E, E, E // 5, DEV)
            keep = ops.moe_topk_keep(rnd(M, E, seed=g), routing, M)
            return ops.linear_keep(rnd(M, F, seed=g + 1), keep, rnd(N, F, scale=F ** -0.5, seed=g + 2),
                                   rnd(N, scale=0.1, seed=g + 3))
        nimg, HW, N, K = 4, 256, 320, 320  # per_image (GN-folded proj_in)
        x = rnd(nimg * HW, K, seed=g)
        wf = rnd(nimg, N, K, scale=K ** -0.5, seed=g + 1)
        colf = rnd(nimg, N, seed=g + 3).float()
        return ops.linear_per_image(x, wf, colf, HW)

    for mode in (0, 2, 1):
        with tune.tuned(epi_direct=mode):
            outs.append(run())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
