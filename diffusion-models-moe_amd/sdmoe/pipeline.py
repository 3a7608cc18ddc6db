"""StableDiffusionPipeline stand-in: synthetic text conditioning + a scheduler (DDIM, PNDM, Euler or DPM-Solver++ 2M;
epsilon or v-prediction for the last two) + classifier-free guidance, with the denoising loop entirely on the GPU
(U-Net on the sdmoe kernels, CFG + scheduler update + next U-Net input in one HIP kernel).

Call shape kept from diffusers / the reference's callers: `pipe(prompt_or_list, safety_checker=...)` returns
an object with `.images` (base_receiver.py:73, remove_wanda_neurons_fast.py:127-130, eval_coco.py:266-272).
Without `text_encoder` / `vae` attached (the metric's workload) prompts map to seeded synthetic
[77, 768] embeddings and `.images` holds the final latents ([4, H, W] fp32 per prompt); with them attached
(sdmoe.clip, sdmoe.vae) prompts are encoded by the HIP CLIP encoder and `output_type` "pt" / "np" decodes to RGB.
Loop invariants are hoisted per call: the cross-attention K/V of the context (unet.Attention.cross_kv) and the
projected time embeddings of every step of the schedule (UNet2DConditionModel.time_embed_table).
"""
from __future__ import annotations

import os
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .config import UNetConfig
from .unet import CTX_LEN, IN_PAD, OUT_PAD, UNet2DConditionModel
from .weights import make_state_dict

# all steps' time embeddings in one batched pass per call (0: per step, the A/B reference)
PRECOMPUTE_TEMB = os.environ.get("SDMOE_TEMB_TABLE", "1") != "0"


def ddim_schedule(num_inference_steps=50, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                  steps_offset=1, set_alpha_to_one=False):
    """DDIMScheduler as SD-1.x configures it (scaled_linear betas, 'leading' spacing, steps_offset=1):
    returns (timesteps, alpha_cumprod[t], alpha_cumprod[prev t]) as host lists (scheduler constants)."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    final = 1.0 if set_alpha_to_one else float(ac[0])
    ratio = num_train_timesteps // num_inference_steps
    ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].astype(np.int64) + steps_offset
    a_t = [float(ac[t]) for t in ts]
    a_prev = [float(ac[t - ratio]) if t - ratio >= 0 else final for t in ts]
    return [int(t) for t in ts], a_t, a_prev


def pndm_schedule(num_inference_steps=50, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                  steps_offset=1, set_alpha_to_one=False):
    """PNDMScheduler(skip_prk_steps=True) as SD-1.x configures it — the reference pipelines' default scheduler
    (51 U-Net calls for 50 steps, hence the reference's T = 51). Returns, per U-Net call, (timestep, coef[7],
    flags[3]) for sdmoe_cfg_multistep_step: the PLMS combination of step_plms (diffusers
    schedulers/scheduling_pndm.py) over a 4-slot eps history ring and _get_prev_sample's a, b."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0).double().numpy()
    final = 1.0 if set_alpha_to_one else float(ac[0])
    ratio = num_train_timesteps // num_inference_steps
    ts = (np.arange(0, num_inference_steps) * ratio).round() + steps_offset
    plms = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].astype(np.int64)
    plan, ets, counter = [], [], 0
    for t_call in plms:
        timestep, prev_t = int(t_call), int(t_call) - ratio
        c_hist = [0.0, 0.0, 0.0, 0.0]
        store, use_cur, save_cur = -1, 0, 0
        if counter != 1:
            ets = ets[-3:]
            store = next(s for s in range(4) if s not in ets)
            new_ets = ets + [store]
        else:
            prev_t, timestep = timestep, timestep + ratio
            new_ets = ets
        n = len(new_ets)
        if n == 1 and counter == 0:
            c_new, save_cur = 1.0, 1
        elif n == 1 and counter == 1:
            c_new, use_cur = 0.5, 1
            c_hist[new_ets[-1]] = 0.5
        elif n == 2:
            c_new = 1.5
            c_hist[new_ets[-2]] = -0.5
        elif n == 3:
            c_new = 23.0 / 12
            c_hist[new_ets[-2]], c_hist[new_ets[-3]] = -16.0 / 12, 5.0 / 12
        else:
            c_new = 55.0 / 24
            c_hist[new_ets[-2]], c_hist[new_ets[-3]], c_hist[new_ets[-4]] = -59.0 / 24, 37.0 / 24, -9.0 / 24
        at = float(ac[timestep])
        ap = float(ac[prev_t]) if prev_t >= 0 else final
        a = (ap / at) ** 0.5
        denom = at * (1 - ap) ** 0.5 + (at * (1 - at) * ap) ** 0.5
        plan.append((int(t_call), [c_new] + c_hist + [a, (ap - at) / denom], [store, use_cur, save_cur]))
        ets = new_ets
        counter += 1
    return plan


@dataclass
class SigmaSchedule:
    """A sigma-parameterised schedule for sdmoe_cfg_x0_step: `timesteps` as the U-Net is given them, `sigmas` fp32
    [steps + 1] ending in 0, the first input's two scales for sdmoe_prepare_input_scaled, and per step
    plan[i] = (t, coef[6] = [cx, cm, a, b0, b1, in_scale], flags[2] = [use_prev, store_prev])."""
    timesteps: np.ndarray
    sigmas: np.ndarray
    init_noise_sigma: float
    first_in_scale: float
    plan: list


PREDICTION_TYPES = ("epsilon", "v_prediction")


def _sigmas_at(timesteps, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
    """Both sigma schedulers: the fp32 table ((1 - ac) / ac) ** 0.5 of the scaled_linear betas, interpolated at
    `timesteps`, 0.0 appended (final_sigmas_type "zero"), fp32."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    table = (((1 - ac) / ac) ** 0.5).numpy()
    s = np.interp(np.asarray(timesteps, dtype=np.float64), np.arange(num_train_timesteps), table)
    return np.concatenate([s, [0.0]]).astype(np.float32)


def _check_prediction_type(prediction_type):
    if prediction_type not in PREDICTION_TYPES:
        raise ValueError(f"prediction_type must be 'epsilon' or 'v_prediction', got {prediction_type!r}")


def euler_schedule(num_inference_steps=50, timestep_spacing="leading", prediction_type="epsilon", steps_offset=1,
                   num_train_timesteps=1000):
    """EulerDiscreteScheduler (s_churn = 0, no Karras sigmas) as stabilityai/stable-diffusion-xl-base-1.0 ("leading",
    steps_offset 1, epsilon) and stabilityai/stable-diffusion-2 ("linspace", v_prediction) configure it, restated from
    diffusers' scheduling_euler_discrete.py: pred_original_sample, derivative = (x - x0) / sigma and
    x + derivative * (sigma' - sigma) collapse to x' = (sigma' / sigma) x + (1 - sigma' / sigma) x0. The "linspace"
    timesteps are non-integer floats and reach the U-Net as they are. Coefficients are Python floats (float64) of the
    fp32 sigma table; the C ABI rounds them to fp32 once."""
    _check_prediction_type(prediction_type)
    n = num_inference_steps
    if timestep_spacing == "linspace":
        ts = np.linspace(0, num_train_timesteps - 1, n, dtype=np.float32)[::-1].copy()
    elif timestep_spacing == "leading":
        ts = (np.arange(0, n) * (num_train_timesteps // n)).round()[::-1].astype(np.float32) + steps_offset
    else:
        raise ValueError(f"timestep_spacing must be 'leading' or 'linspace', got {timestep_spacing!r}")
    sigmas = _sigmas_at(ts, num_train_timesteps)
    smax = float(sigmas.max())
    init = smax if timestep_spacing == "linspace" else (smax ** 2 + 1) ** 0.5
    plan = []
    for i in range(n):
        s, sn = float(sigmas[i]), float(sigmas[i + 1])
        if prediction_type == "epsilon":
            cx, cm = 1.0, -s
        else:
            cx, cm = 1.0 / (s * s + 1), -s / (s * s + 1) ** 0.5
        a = sn / s
        plan.append((float(ts[i]), [cx, cm, a, 1.0 - a, 0.0, 1.0 / (sn * sn + 1) ** 0.5], [0, 0]))
    return SigmaSchedule(ts, sigmas, init, 1.0 / (float(sigmas[0]) ** 2 + 1) ** 0.5, plan)


def dpmpp_2m_schedule(num_inference_steps=50, prediction_type="epsilon", num_train_timesteps=1000):
    """DPMSolverMultistepScheduler as stabilityai/stable-diffusion-2-1's config gives it (dpmsolver++, solver_order 2,
    midpoint, lower_order_final, "linspace" spacing, final sigma 0, no Karras sigmas, no thresholding), restated from
    diffusers' scheduling_dpmsolver_multistep.py. With alpha = 1 / sqrt(sigma^2 + 1), varsigma = sigma * alpha,
    lambda = ln alpha - ln varsigma, h = lambda_t - lambda_s and E = -alpha_t * expm1(-h), the first-order update is
    x' = (varsigma_t / varsigma_s) x + E x0 and the second-order one adds 0.5 E (x0 - prev_x0) / r0,
    r0 = (lambda_s - lambda_{s-1}) / h. The first and the last step are first order; the last step has sigma' = 0
    (lambda_t = +inf), where diffusers' arithmetic gives x0: (a, b0, b1) = (0, 1, 0), set directly and ahead of every
    other case (a single step is the last step). No input scaling: init_noise_sigma and every in_scale are 1."""
    import math
    _check_prediction_type(prediction_type)
    n = num_inference_steps
    ts = np.linspace(0, num_train_timesteps - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
    sigmas = _sigmas_at(ts, num_train_timesteps)
    alpha = [1.0 / (float(s) ** 2 + 1) ** 0.5 for s in sigmas]
    vs = [float(s) * a for s, a in zip(sigmas, alpha)]
    lam = [math.log(a) - math.log(v) for a, v in zip(alpha[:-1], vs[:-1])]  # lambda of sigma = 0 is never evaluated
    plan = []
    for i in range(n):
        if prediction_type == "epsilon":
            cx, cm = 1.0 / alpha[i], -vs[i] / alpha[i]
        else:
            cx, cm = alpha[i], -vs[i]
        if i == n - 1:
            a, b0, b1, use_prev = 0.0, 1.0, 0.0, 0
        else:
            h = lam[i + 1] - lam[i]
            E = -alpha[i + 1] * math.expm1(-h)
            a = vs[i + 1] / vs[i]
            if i == 0:
                b0, b1, use_prev = E, 0.0, 0
            else:
                r0 = (lam[i] - lam[i - 1]) / h
                b0, b1, use_prev = E * (1 + 0.5 / r0), -0.5 * E / r0, 1
        plan.append((int(ts[i]), [cx, cm, a, b0, b1, 1.0], [use_prev, int(i < n - 1)]))
    return SigmaSchedule(ts, sigmas, 1.0, 1.0, plan)


def prompt_embedding(prompt: str, dim: int = 768) -> torch.Tensor:
    """Seeded synthetic text conditioning [77, dim] fp32 (CPU) standing in for the CLIP text encoder."""
    rng = np.random.default_rng(zlib.crc32(prompt.encode("utf-8")))
    return torch.from_numpy((rng.standard_normal((CTX_LEN, dim)) * 0.5).astype(np.float32))


def pooled_embedding(prompt: str, dim: int = 1280) -> torch.Tensor:
    """Seeded synthetic pooled text embedding [dim] (SDXL text_embeds; CLIP-G pooled output stand-in)."""
    rng = np.random.default_rng(zlib.crc32(("pooled:" + prompt).encode("utf-8")))
    return torch.from_numpy((rng.standard_normal(dim) * 0.5).astype(np.float32))


def sdxl_time_ids(height: int, width: int) -> list:
    """SDXL micro-conditioning (original_size, crops_coords_top_left, target_size) for an uncropped image."""
    return [float(height), float(width), 0.0, 0.0, float(height), float(width)]


def initial_latents(seed: int, index: int, cfg: UNetConfig) -> torch.Tensor:
    """Per-prompt latents from a CPU generator seeded by (seed, global prompt index): identical for any
    world size / sharding."""
    # masked to 63 bits: torch.initial_seed() of an unseeded process is a random 64-bit value
    g = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(index)) & 0x7FFF_FFFF_FFFF_FFFF)
    return torch.randn((1, cfg.in_channels, cfg.sample_size, cfg.sample_size), generator=g)


@dataclass
class PipelineOutput:
    images: list


class _HookHandle:
    """Returned by StableDiffusionPipeline.register_unet_output_hook / register_prompt_hook: remove() takes the hook
    off again (once)."""

    def __init__(self, hooks, fn):
        self._hooks, self._fn = hooks, fn

    def remove(self):
        if self._fn is not None and self._fn in self._hooks:
            self._hooks.remove(self._fn)
        self._fn = None


SCHEDULERS = ("ddim", "pndm", "euler", "dpmpp_2m")


class StableDiffusionPipeline:
    def __init__(self, unet: UNet2DConditionModel, device="cuda", num_inference_steps=50, guidance_scale=7.5,
                 scheduler="ddim", vae=None, text_encoder=None, tokenizer=None, text_encoder_2=None,
                 tokenizer_2=None, timestep_spacing=None, prediction_type="epsilon"):
        if scheduler not in SCHEDULERS:
            raise ValueError(f"scheduler must be one of {', '.join(map(repr, SCHEDULERS))}, got {scheduler!r}")
        _check_prediction_type(prediction_type)
        if prediction_type != "epsilon" and scheduler in ("ddim", "pndm"):
            raise ValueError(f"scheduler {scheduler!r} is epsilon-only; prediction_type {prediction_type!r} needs "
                             "'euler' or 'dpmpp_2m'")
        self.scheduler = scheduler  # "pndm": the reference's default (51 U-Net calls per 50 steps)
        self.unet = unet
        self.config = unet.config
        self.prediction_type = prediction_type
        # Euler only: "leading" on an SDXL config, "linspace" otherwise, as the checkpoints' scheduler configs
        if scheduler == "euler":
            timestep_spacing = timestep_spacing or ("leading" if self.is_sdxl else "linspace")
            if timestep_spacing not in ("leading", "linspace"):
                raise ValueError(f"timestep_spacing must be 'leading' or 'linspace', got {timestep_spacing!r}")
        elif timestep_spacing is not None and (scheduler, timestep_spacing) not in (
                ("ddim", "leading"), ("pndm", "leading"), ("dpmpp_2m", "linspace")):
            raise ValueError(f"scheduler {scheduler!r} does not support timestep_spacing {timestep_spacing!r}")
        self.timestep_spacing = timestep_spacing
        self.device = torch.device(device)
        self.num_inference_steps = num_inference_steps
        self.guidance_scale = guidance_scale
        self.prompt_offset = 0  # global index of the first prompt (data-parallel shards set this per rank)
        self.vae = vae  # sdmoe.vae.AutoencoderKLDecoder or None (output_type "pt"/"np" then decodes the latents)
        self.output_type = "latent"  # default of __call__'s output_type (the receivers call pipe(prompt) bare)
        # sdmoe.clip.CLIPTextModel(s) or None (None: seeded synthetic [77, dim] conditioning, prompt_embedding)
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.text_encoder_2 = text_encoder_2
        self.tokenizer_2 = tokenizer_2
        self._unet_output_hooks = []  # register_unet_output_hook
        self._prompt_hooks = []  # register_prompt_hook

    def register_unet_output_hook(self, fn):
        """Call fn(step_index, eps, nimg, HW) after every U-Net evaluation of the denoising loop, before the scheduler
        step consumes it -- the seam of `model.unet.register_forward_hook` in the reference's BaseUNetReceiver /
        RemoveNeuronsNoiseHPO (the loop calls unet.forward_nhwc, so a module forward hook never fires). eps is the
        loop's live fp16 [nimg * HW, OUT_PAD] buffer: channels 0..3 are the prediction, rows are [uncond x B ; cond x
        B] images of HW positions, and the next step overwrites it -- valid during the call only (copy what you keep:
        ops.noise_capture). step_index counts U-Net calls (0..49 for DDIM, Euler and DPM++ 2M, 0..50 for PNDM at 50 steps). The return
        value is ignored. Returns a handle whose .remove() unregisters fn."""
        self._unet_output_hooks.append(fn)
        return _HookHandle(self._unet_output_hooks, fn)

    def register_prompt_hook(self, fn):
        """Call fn(prompts, ctx, B) in every __call__ after encode_prompt and before the denoising loop: prompts the
        call's B prompt strings, ctx the full fp16 [2B * 77, dim] conditioning buffer ([uncond x B ; cond x B] rows,
        also when the call runs without guidance and the loop reads only the conditional half). The seam of the
        reference's per-prompt concept checkers (benchmarks/unified_editing.py:109-119): a hook may configure a
        receiver for the call from the rows (neuron_receivers.WandaRemovePerPrompt with a router). The return value
        is ignored. Returns a handle whose .remove() unregisters fn."""
        self._prompt_hooks.append(fn)
        return _HookHandle(self._prompt_hooks, fn)

    def _after_unet(self, step_index, eps, HW):
        for fn in tuple(self._unet_output_hooks):
            fn(step_index, eps, eps.shape[0] // HW, HW)

    @classmethod
    def synthetic(cls, cfg: UNetConfig | None = None, seed: int = 0, device="cuda", **kw):
        cfg = cfg or UNetConfig.sd14()
        unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, seed), cfg, device)
        return cls(unet, device, **kw)

    @property
    def is_sdxl(self):
        return self.config.addition_embed_type == "text_time"

    def _ids(self, tok, texts):
        return tok(texts, padding="max_length", max_length=CTX_LEN, truncation=True, return_tensors="pt").input_ids

    def encode_prompt(self, prompts, return_pooled=False):
        """[uncond x B ; cond x B] context rows [2B*77, dim] fp16 on device (uncond first, as diffusers).
        SDXL base sets force_zeros_for_empty_prompt: the unconditional embeddings are zeros.
        With text encoders: SD-1.x runs text_encoder on [""] * B + prompts (last_hidden_state); SDXL writes the
        two encoders' penultimate hidden states straight into the two column halves of the context and takes
        text_encoder_2's projected pooled output (diffusers StableDiffusionXLPipeline.encode_prompt)."""
        dim = self.config.cross_attention_dim
        B = len(prompts)
        if self.text_encoder is not None:
            ctx = torch.empty((2 * B * CTX_LEN, dim), dtype=torch.float16, device=self.device)
            pooled = None
            if not self.is_sdxl:
                self.text_encoder.encode(self._ids(self.tokenizer, [""] * B + list(prompts)), out=ctx)
            else:
                d1 = self.text_encoder.config.hidden_size
                ctx[:B * CTX_LEN].zero_()
                cond = ctx[B * CTX_LEN:]
                self.text_encoder.encode(self._ids(self.tokenizer, prompts), hidden_layer=-2, out=cond[:, :d1])
                r = self.text_encoder_2.encode(self._ids(self.tokenizer_2 or self.tokenizer, prompts),
                                               hidden_layer=-2, out=cond[:, d1:], pooled=True)
                pooled = torch.zeros((2 * B, r["text_embeds"].shape[1]), dtype=torch.float16, device=self.device)
                pooled[B:] = r["text_embeds"]
            return (ctx, pooled) if return_pooled else ctx
        unc = torch.zeros(CTX_LEN, dim) if self.is_sdxl else prompt_embedding("", dim)
        embs = [unc] * len(prompts) + [prompt_embedding(p, dim) for p in prompts]
        ctx = torch.cat(embs, 0).to(self.device, torch.float16).contiguous()
        return (ctx, None) if return_pooled else ctx

    def added_cond(self, prompts, pooled=None):
        """SDXL added_cond_kwargs rows [uncond x B ; cond x B]: pooled text_embeds [2B, pooled] and time_ids
        [2B, 6] (1024^2 uncropped at sample_size 128)."""
        cfg = self.config
        d = cfg.pooled_dim
        if pooled is None:
            pooled = torch.stack([torch.zeros(d)] * len(prompts) + [pooled_embedding(p, d) for p in prompts])
        px = 8 * cfg.sample_size
        tids = torch.tensor([sdxl_time_ids(px, px)] * (2 * len(prompts)), dtype=torch.float32)
        return {"text_embeds": pooled, "time_ids": tids}

    def __call__(self, prompt, num_inference_steps=None, guidance_scale=None, latents=None, seed=None,
                 prompt_offset=None, safety_checker=None, output_type=None, **unused):
        prompts = [prompt] if isinstance(prompt, str) else list(prompt)
        B = len(prompts)
        cfg = self.config
        steps = num_inference_steps or self.num_inference_steps
        g = self.guidance_scale if guidance_scale is None else guidance_scale
        do_cfg = g > 1.0
        if seed is None:
            seed = torch.initial_seed()  # receivers call torch.manual_seed(self.seed) first (base_receiver.py:70)
        if prompt_offset is None:
            prompt_offset = self.prompt_offset
        if latents is None:
            latents = torch.cat([initial_latents(seed, prompt_offset + i, cfg) for i in range(B)])
        lat = latents.to(self.device, torch.float32).contiguous()
        ncopy = 2 if do_cfg else 1
        ctx, pooled = self.encode_prompt(prompts, return_pooled=True)
        for fn in tuple(self._prompt_hooks):
            fn(prompts, ctx, B)
        add_hidden = None
        if self.is_sdxl:
            ac = self.added_cond(prompts, pooled)
            add_hidden = self.unet.add_embed_hidden(ac["text_embeds"], ac["time_ids"])  # once per call
            if not do_cfg:
                add_hidden = add_hidden[B:]
        if not do_cfg:
            ctx = ctx[B * CTX_LEN:]
        HW = cfg.sample_size * cfg.sample_size
        x_in = torch.zeros((ncopy * B * HW, IN_PAD), dtype=torch.float16, device=self.device)
        eps = torch.empty((ncopy * B * HW, OUT_PAD), dtype=torch.float16, device=self.device)
        bufs = dict(lat=lat, x_in=x_in, eps=eps, ctx=ctx, add_hidden=add_hidden)
        if self.scheduler in ("euler", "dpmpp_2m"):
            sched = bufs["sigma_schedule"] = self.sigma_schedule(steps)
            ops.prepare_input_scaled(lat, x_in, ncopy, sched.init_noise_sigma, sched.first_in_scale)
        else:
            ops.prepare_input(lat, x_in, ncopy)
        self._denoise(bufs, steps, g, do_cfg)
        out = PipelineOutput(images=self._finish(lat, output_type or self.output_type))
        return out

    def sigma_schedule(self, steps):
        """The SigmaSchedule of scheduler "euler" / "dpmpp_2m" for `steps` steps."""
        if self.scheduler == "euler":
            return euler_schedule(steps, self.timestep_spacing, self.prediction_type)
        if self.scheduler == "dpmpp_2m":
            return dpmpp_2m_schedule(steps, self.prediction_type)
        raise ValueError(f"scheduler {self.scheduler!r} has no sigma schedule")

    def _denoise(self, bufs, steps, g, do_cfg):
        """The denoising loop over bufs (lat, x_in, eps, ctx, add_hidden)."""
        lat, x_in, eps, ctx, add_hidden = (bufs[k] for k in ("lat", "x_in", "eps", "ctx", "add_hidden"))
        hooks = self._unet_output_hooks  # register_unet_output_hook: empty = the bare loop
        HW = self.config.sample_size * self.config.sample_size

        def temb_row(table, i):
            return None if table is None else table[i:i + 1]

        time_table = self.unet.time_embed_table if PRECOMPUTE_TEMB else (lambda ts: None)
        if self.scheduler == "pndm":
            hist = bufs.setdefault("hist", torch.zeros((4,) + tuple(lat.shape), dtype=torch.float32, device=self.device))
            cur = bufs.setdefault("cur", torch.zeros_like(lat))
            plan = pndm_schedule(steps)
            if "table" not in bufs:
                bufs["table"] = time_table([t for t, _, _ in plan])  # loop-invariant: all steps at once
            table = bufs["table"]
            for i, (t, coef, flags) in enumerate(plan):
                def body(i=i, t=t, coef=coef, flags=flags):
                    self.unet.forward_nhwc(x_in, float(t), ctx, out=eps, add_hidden=add_hidden, temb=temb_row(table, i))
                    if hooks:
                        self._after_unet(i, eps, HW)
                    ops.cfg_multistep_step(eps, lat, do_cfg, g, hist, cur, coef, flags, next_in=x_in)
                body()
        elif self.scheduler in ("euler", "dpmpp_2m"):
            # x_in already holds the scaled first input (__call__: prepare_input_scaled with this schedule's scales)
            plan = (bufs.get("sigma_schedule") or self.sigma_schedule(steps)).plan
            prev_x0 = None
            if any(f[0] or f[1] for _, _, f in plan):  # DPM++ only; allocated on first use
                if "prev_x0" not in bufs:
                    bufs["prev_x0"] = torch.zeros_like(lat)
                prev_x0 = bufs["prev_x0"]
            if "table" not in bufs:
                bufs["table"] = time_table([t for t, _, _ in plan])  # loop-invariant: all steps at once
            table = bufs["table"]
            for i, (t, coef, flags) in enumerate(plan):
                def body(i=i, t=t, coef=coef, flags=flags):
                    self.unet.forward_nhwc(x_in, float(t), ctx, out=eps, add_hidden=add_hidden, temb=temb_row(table, i))
                    if hooks:
                        self._after_unet(i, eps, HW)
                    ops.cfg_x0_step(eps, lat, do_cfg, g, prev_x0, coef, flags, next_in=x_in)
                body()
        else:
            ts, a_t, a_prev = ddim_schedule(steps)
            if "table" not in bufs:
                bufs["table"] = time_table(list(ts))  # loop-invariant: all steps at once
            table = bufs["table"]
            for s, t in enumerate(ts):
                def body(s=s, t=t):
                    self.unet.forward_nhwc(x_in, float(t), ctx, out=eps, add_hidden=add_hidden, temb=temb_row(table, s))
                    if hooks:
                        self._after_unet(s, eps, HW)
                    ops.cfg_ddim_step(eps, lat, do_cfg, g, a_t[s], a_prev[s], next_in=x_in)
                body()

    def _finish(self, lat, output_type):
        """output_type "latent": the denoised latents; "pt" / "np": vae.decode(latents / scaling_factor) then
        (x / 2 + 0.5).clamp(0, 1) as diffusers' VaeImageProcessor does (images [3, H, W] / [H, W, 3])."""
        B = lat.shape[0]
        if output_type == "latent":
            return [lat[i] for i in range(B)]
        if self.vae is None:
            raise ValueError(f"output_type {output_type!r} needs a VAE decoder (pipe.vae = AutoencoderKLDecoder(...))")
        from .vae import postprocess
        img = postprocess(self.vae.decode(lat))
        if output_type == "np":
            return [img[i].permute(1, 2, 0).cpu().numpy() for i in range(B)]
        return [img[i] for i in range(B)]

    def to(self, device):
        """Weights are placed at construction; kept for the reference's `model.to(args.gpu)` call shape."""
        return self
