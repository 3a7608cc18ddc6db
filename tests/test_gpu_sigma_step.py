"""The sigma-scheduler step kernels of csrc/sigma_step.hip (sdmoe_prepare_input_scaled, sdmoe_cfg_x0_step) on the MI355X
against the float64 restatements of tests/sigma_step_ref.py, alone, free-running through whole Euler and DPM-Solver++ 2M
schedules (epsilon and v-prediction), and through StableDiffusionPipeline; plus the UNetConfig.sd2 preset.

Every bound comes from sigma_step_ref (constants and their justification there; tests/test_sigma_step_host.py shows on
the CPU that an fp32 restatement stays inside them and that subtly wrong ones do not). The device is compared with
itself only where two paths must agree bit for bit: next_in given against None, a NULL prev_x0 against a NaN-filled
one, the two CFG copies of next_in. Output buffers carry a sentinel wherever the kernel must not write. Each test prints
the largest fraction of its bound the device reached (pytest -s); nothing is sized from those figures. On the MI355X
they were: cfg_x0_step 0.269 of the lat bound and 0.263 of the stored-x0 bound (0.263 and 0.305 at the grid-stride
size); free-running 0.064 of the propagated bound at most (Euler "leading", epsilon, 6 steps; 0.002 for DPM++ epsilon
at 50 steps, whose bound grows fastest); through the pipeline 0.063 for the latents and 0.999 for the U-Net inputs
(nearly all of it the half fp16 ulp of the input's own rounding).
"""
import math

import numpy as np
import pytest
import torch

import sigma_step_ref as S
import step_loop_ref as R

pytestmark = pytest.mark.gpu

from sdmoe import _lib, ops  # noqa: E402
from sdmoe.config import UNetConfig  # noqa: E402
from sdmoe.pipeline import StableDiffusionPipeline, dpmpp_2m_schedule, euler_schedule, prompt_embedding  # noqa: E402

DEV = "cuda"
G = R.GUIDANCE
SENT = 123.0
NAN = float("nan")
F = np.float32


def schedule(kind, steps, pt, spacing=None):
    return dpmpp_2m_schedule(steps, pt) if kind == "dpmpp_2m" else euler_schedule(steps, spacing, pt)


def sentinel(rows, cols):
    return torch.full((rows, cols), SENT, dtype=torch.float16, device=DEV)


def untouched(t):
    return bool((t == SENT).all().item())


def same_bits(a, b):
    return R.bits_equal(R.as_bits(a), R.as_bits(b))


def half_ulp16(v):
    """Half an fp16 ulp at |v| (float64 array): 2^-25 in the subnormal range."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 11)


def rows_to_planes(rows, B, HW):
    """fp16 rows [B * HW, >= 4] -> float64 [B, 4, HW]."""
    return R.f64(rows)[:, :4].reshape(B, HW, 4).transpose(0, 2, 1)


# ---- prepare_input_scaled ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ldo", [4, 8, 64])
@pytest.mark.parametrize("ncopy", [1, 2])
def test_prepare_input_scaled(ncopy, ldo):
    B, H, W = 2, 5, 7
    lat = R.prepare_latents(B, H, W, 1)
    rows = ncopy * B * H * W

    def run(lat_scale, in_scale):
        buf = torch.full((rows + 3, ldo), NAN, dtype=torch.float16, device=DEV)
        d = lat.to(DEV)
        ops.prepare_input_scaled(d, buf[:rows], ncopy, lat_scale, in_scale)
        got = buf.cpu()
        pad = torch.full((rows + 3, ldo), NAN, dtype=torch.float16)
        assert same_bits(got[:rows, 4:], pad[:rows, 4:]) and same_bits(got[rows:], pad[rows:]), "padding written"
        return d.cpu(), got[:rows, :4]

    # scales (1, 1): sdmoe_prepare_input bit for bit, lat unchanged
    d, out = run(1.0, 1.0)
    plain = sentinel(rows, ldo)
    ops.prepare_input(lat.to(DEV), plain, ncopy)
    assert same_bits(out, plain[:, :4].cpu()) and same_bits(out, R.prepare_ref(lat, ncopy))
    assert same_bits(d, lat)
    assert torch.isinf(out).any()
    # SDXL's 50-step "leading" scales: two separately rounded fp32 products, so equality is the bar
    s, k = 13.158469, 1 / math.sqrt(13.120416 ** 2 + 1)
    d, out = run(s, k)
    scaled, ref = S.prepare_scaled_ref(lat, ncopy, s, k)
    assert R.bits_equal(d.numpy(), scaled), "lat is not fp32(lat * lat_scale)"
    assert R.bits_equal(out.numpy(), ref), "out is not fp16(fp32(fp32(lat * lat_scale) * in_scale))"


# ---- one call of cfg_x0_step ---------------------------------------------------------------------------------------

def check_next_in(x_in, lat, in_scale, B, HW, do_cfg):
    """x_in [2 * B * HW + 2, ld] after a step with next_in: both CFG copies are bit-equal and hold fp16 of the device's
    own lat * in_scale (within half an fp16 ulp and the fp32 rounding of the product); the rest keeps the sentinel."""
    n = B * HW
    x = x_in.cpu()
    want = R.planes(lat) * R.f32(in_scale)
    got = rows_to_planes(x[:n], B, HW)
    assert (np.abs(got - want) <= half_ulp16(want) + R.U * np.abs(want)).all(), "next_in is not fp16(lat * in_scale)"
    if do_cfg:
        assert same_bits(x[n:2 * n, :4], x[:n, :4]), "the two CFG copies of next_in differ"
    else:
        assert untouched(x[n:2 * n, :4]), "second image copy written without CFG"
    assert untouched(x[:, 4:]) and untouched(x[2 * n:]), "wrote outside channels 0..3 of the image rows"


def one_call(lat0, prev0, dbuf_view, B, HW, do_cfg, coef, flags, ldn=64):
    """Run the kernel once from CPU lat0 / prev0 (prev0 None: NULL pointer): (lat, prev, x_in) afterwards, on the
    device."""
    lat = lat0.to(DEV)
    prev = None if prev0 is None else prev0.to(DEV)
    x_in = sentinel(2 * B * HW + 2, ldn)
    ops.cfg_x0_step(dbuf_view, lat, do_cfg, G, prev, coef, flags, next_in=x_in)
    return lat, prev, x_in


@pytest.mark.parametrize("form", R.EPS_FORMS)
@pytest.mark.parametrize("H,W", [(5, 10), (16, 16)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("do_cfg", [True, False])
def test_cfg_x0_step(do_cfg, B, H, W, form):
    HW = H * W
    lat0 = R.latents(B, H, W, 3)
    prev_rand = R.latents(B, H, W, 23)
    prev_nan = torch.full_like(lat0, NAN)
    buf, c0, w = R.eps_buffer((2 if do_cfg else 1) * B * HW, form, 7)
    eu, ec = R.eps_planes(buf[:, c0:c0 + w], B, HW, do_cfg)
    dbuf = buf.to(DEV)
    eps = dbuf[:, c0:c0 + w]
    worst = sworst = 0.0
    for name, coef in S.coef_cases():
        for flags in S.FLAG_PAIRS:
            use_prev, store_prev = flags
            prev0 = prev_rand if use_prev else prev_nan  # never read without use_prev: NaN must not reach lat
            r = S.x0_step_ref(R.planes(lat0), R.planes(prev0), eu, ec, do_cfg, G, coef, flags)
            lat, prev, x_in = one_call(lat0, prev0, eps, B, HW, do_cfg, coef, flags)
            pre = (R.planes(lat0).astype(F), R.planes(prev0).astype(F))
            post = (R.planes(lat).astype(F), R.planes(prev).astype(F))
            fails, frac, sfrac = S.x0_call_failures(r, flags, pre, post)
            assert not fails, (name, flags, fails)
            worst, sworst = max(worst, frac), max(sworst, sfrac)
            check_next_in(x_in, lat, coef[5], B, HW, do_cfg)
            lat2 = lat0.to(DEV)
            prev2 = prev0.to(DEV)
            ops.cfg_x0_step(eps, lat2, do_cfg, G, prev2, coef, flags, next_in=None)
            assert same_bits(lat2, lat) and same_bits(prev2, prev), "the result depends on next_in"
            if flags == (0, 0):
                lat3, _, x3 = one_call(lat0, None, eps, B, HW, do_cfg, coef, flags)
                assert same_bits(lat3, lat) and same_bits(x3, x_in), "a NULL prev_x0 changes the result"
    assert same_bits(dbuf, buf), "eps was written"
    print(f"cfg_x0_step cfg={do_cfg} B={B} HW={HW} {form}: {worst:.3f} of the lat bound, {sworst:.3f} of the stored-x0 "
          f"bound")


@pytest.mark.parametrize("flags", [(0, 1), (1, 0), (1, 1)])
def test_cfg_x0_step_rejects_null_prev(flags):
    B, H = 1, 5
    lat0, eps = R.schedule_inputs(1, B, H, H, True, 5)
    lat = lat0.to(DEV)
    x_in = sentinel(2 * B * H * H, 8)
    with pytest.raises(_lib.SdmoeError, match="sdmoe_cfg_x0_step"):
        ops.cfg_x0_step(eps[0].to(DEV), lat, True, G, None, S.HAND_COEF, flags, next_in=x_in)
    assert same_bits(lat, lat0) and untouched(x_in)


def test_cfg_x0_step_rejects_ragged_strides():
    B, H = 1, 5
    lat0 = R.latents(B, H, H, 5).to(DEV)
    eps6 = torch.zeros((2 * B * H * H, 6), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="sdmoe_cfg_x0_step"):
        ops.cfg_x0_step(eps6, lat0, True, G, None, S.HAND_COEF, (0, 0))
    eps8 = torch.zeros((2 * B * H * H, 8), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="sdmoe_cfg_x0_step"):
        ops.cfg_x0_step(eps8, lat0, True, G, None, S.HAND_COEF, (0, 0), next_in=sentinel(2 * B * H * H, 6))


def test_grid_stride_cfg_x0_step():
    """B * HW = 1,058,000 > 4096 blocks * 256 threads: the grid-stride loop takes a second trip. Second order with a
    store."""
    B, H, W = 2, 529, 1000
    HW = H * W
    assert B * HW > 4096 * 256
    coef, flags = dpmpp_2m_schedule(50, "v_prediction").plan[25][1], (1, 1)
    lat0, prev0 = R.latents(B, H, W, 3), R.latents(B, H, W, 23)
    buf = R.eps_buffer(2 * B * HW, "dense8", 7)[0]
    eu, ec = R.eps_planes(buf, B, HW, True)
    r = S.x0_step_ref(R.planes(lat0), R.planes(prev0), eu, ec, True, G, coef, flags)
    lat, prev, x_in = one_call(lat0, prev0, buf.to(DEV), B, HW, True, coef, flags, ldn=8)
    pre = (R.planes(lat0).astype(F), R.planes(prev0).astype(F))
    post = (R.planes(lat).astype(F), R.planes(prev).astype(F))
    fails, frac, sfrac = S.x0_call_failures(r, flags, pre, post)
    assert not fails, fails
    check_next_in(x_in, lat, coef[5], B, HW, True)
    print(f"cfg_x0_step grid-stride: {frac:.3f} of the lat bound, {sfrac:.3f} of the stored-x0 bound")


# ---- free-running schedules ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [6, 50])
@pytest.mark.parametrize("pt", S.PREDICTION_TYPES)
@pytest.mark.parametrize("kind,spacing", S.SCHEDULE_KINDS)
def test_schedule_free_running(kind, spacing, pt, steps):
    """prepare_input_scaled, then every step on fresh random fp16 model outputs, CFG at 7.5, from a NaN-filled prev_x0:
    the final latents against EulerRef / DPMSolverPPRef (float64, diffusers' operation order)."""
    B, H = 2, 5
    HW = H * H
    sched = schedule(kind, steps, pt, spacing)
    lat0, eps = R.schedule_inputs(steps, B, H, H, True, 11)
    lat = lat0.to(DEV)
    prev = torch.full_like(lat, NAN)
    x_in = sentinel(2 * B * HW + 2, 64)
    ops.prepare_input_scaled(lat, x_in[:2 * B * HW], 2, sched.init_noise_sigma, sched.first_in_scale)
    for e, (t, coef, flags) in zip([e.to(DEV) for e in eps], sched.plan):
        ops.cfg_x0_step(e, lat, True, G, prev, coef, flags, next_in=x_in)
    got = R.planes(lat)
    planes = [R.eps_planes(e, B, HW, True) for e in eps]
    s = S.sigma_schedule_ref(R.planes(lat0), planes, sched.plan, True, G, sched.init_noise_sigma, sched.first_in_scale)
    ref = S.scheduler_ref_run(S.make_ref(kind, steps, pt, spacing), R.planes(lat0), planes, True, G)
    assert np.isfinite(ref).all() and np.isfinite(s.E_lat).all() and np.isfinite(got).all()
    frac = float((np.abs(got - ref) / s.E_lat).max())
    assert (np.abs(got - ref) <= s.E_lat).all(), frac
    assert untouched(x_in[:, 4:]) and untouched(x_in[2 * B * HW:])
    print(f"free-running {kind} {spacing} {pt} {steps}: {frac:.3f} of the propagated bound")


# ---- through the pipeline ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_unet():
    from sdmoe.unet import UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    cfg = UNetConfig.tiny(16)
    return cfg, UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 0), cfg, DEV)


@pytest.mark.parametrize("kind,spacing,pt", [("euler", "leading", "epsilon"), ("euler", "linspace", "v_prediction"),
                                             ("dpmpp_2m", None, "v_prediction")])
def test_pipeline_sigma_schedulers(tiny_unet, kind, spacing, pt):
    cfg, unet = tiny_unet
    B, steps, H = 2, 6, cfg.sample_size
    HW = H * H
    pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=steps, scheduler=kind, timestep_spacing=spacing,
                                   prediction_type=pt)
    sched = schedule(kind, steps, pt, spacing)
    seen_t, seen_x, seen_steps = [], [], []
    store = torch.zeros((steps, 2 * B * HW, 4), dtype=torch.float16, device=DEV)
    inner = unet.forward_nhwc

    def shim(x_in, t, ctx, **kw):
        seen_t.append(t)
        seen_x.append(x_in[:, :4].clone())
        return inner(x_in, t, ctx, **kw)

    def hook(step_index, eps, nimg, hw):
        assert (nimg, hw) == (2 * B, HW)
        seen_steps.append(step_index)
        ops.noise_capture(eps, store[step_index])

    handle = pipe.register_unet_output_hook(hook)
    unet.forward_nhwc = shim
    try:
        lat0 = R.latents(B, H, H, 31)
        out = pipe(["a red bicycle", "two owls"], latents=lat0, output_type="latent")
    finally:
        del unet.forward_nhwc
        handle.remove()
    assert seen_steps == list(range(steps))
    assert seen_t == [float(t) for t in sched.timesteps]
    got = R.planes(torch.stack([im.cpu() for im in out.images]))
    planes = [R.eps_planes(store[i].cpu(), B, HW, True) for i in range(steps)]
    g = pipe.guidance_scale
    s = S.sigma_schedule_ref(R.planes(lat0), planes, sched.plan, True, g, sched.init_noise_sigma, sched.first_in_scale)
    xs = []
    ref = S.scheduler_ref_run(S.make_ref(kind, steps, pt, spacing), R.planes(lat0), planes, True, g,
                              on_call=lambda i, x_in, x: xs.append(x_in))
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    frac = float((np.abs(got - ref) / s.E_lat).max())
    assert (np.abs(got - ref) <= s.E_lat).all(), frac
    xfrac = 0.0
    for i in range(steps):
        rows = seen_x[i].cpu()
        assert same_bits(rows[B * HW:], rows[:B * HW]), i
        tol = half_ulp16(xs[i]) + s.inputs[i][1]
        err = np.abs(rows_to_planes(rows[:B * HW], B, HW) - xs[i])
        assert (err <= tol).all(), (i, float((err / tol).max()))
        xfrac = max(xfrac, float((err / tol).max()))
    print(f"pipeline {kind} {spacing} {pt}: latents {frac:.3f} of the propagated bound, U-Net inputs {xfrac:.3f} of "
          f"theirs")


def test_pipeline_argument_errors(tiny_unet):
    cfg, unet = tiny_unet
    with pytest.raises(ValueError, match="euler"):
        StableDiffusionPipeline(unet, DEV, scheduler="heun")
    with pytest.raises(ValueError, match="v_prediction"):
        StableDiffusionPipeline(unet, DEV, scheduler="euler", prediction_type="sample")
    for name in ("ddim", "pndm"):
        with pytest.raises(ValueError, match="epsilon-only"):
            StableDiffusionPipeline(unet, DEV, scheduler=name, prediction_type="v_prediction")
    assert StableDiffusionPipeline(unet, DEV, scheduler="euler").timestep_spacing == "linspace"


# ---- the SD-2.x preset ---------------------------------------------------------------------------------------------

def test_unet_forward_sd2():
    """One forward of the SD-2.x U-Net (64-wide heads, linear projections, 1024-wide context) against the oracle on the
    same fp16-rounded state dict, under test_gpu_sdxl.test_unet_forward_tiny_xl's bar. No new kernel: it pins the
    preset."""
    from oracle.unet_ref import UNetRef
    from sdmoe.unet import UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    from test_gpu_unet import max_rel, moefy_tiny
    cfg = UNetConfig.sd2(16)
    assert (cfg.head_dim, cfg.cross_attention_dim, cfg.use_linear_projection) == (64, 1024, True)
    assert cfg.block_out_channels == UNetConfig.sd14().block_out_channels and UNetConfig.sd2().sample_size == 96
    assert [cfg.heads_for(c) for c in cfg.block_out_channels] == [5, 10, 20, 20]
    sd = make_state_dict(cfg, 0)
    for k in sd:
        sd[k] = sd[k].half().float()
    unet, ref = UNet2DConditionModel.from_state_dict(sd, cfg, DEV), UNetRef(sd, cfg)
    moefy_tiny(StableDiffusionPipeline(unet, DEV), topk=None)
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(0))
    ctx = torch.stack([prompt_embedding("", 1024), prompt_embedding("a photo of a cat", 1024)])
    assert ctx.shape == (2, 77, 1024)
    eps = unet(x.to(DEV), 501.0, ctx.to(DEV))
    assert max_rel(eps, ref(x, 501.0, ctx)) <= 3e-2
