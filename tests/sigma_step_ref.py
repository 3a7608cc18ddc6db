"""Float64 restatements (numpy / torch on the CPU, no HIP library) of the sigma-scheduler step kernels of
csrc/sigma_step.hip and of the two schedulers they serve, the checker of tests/test_sigma_step_host.py (which proves on
the host that an fp32 restatement in the kernel's operation order stays inside every bound and that subtly wrong ones do
not) and of tests/test_gpu_sigma_step.py. Inputs, layouts and the CFG bound come from tests/step_loop_ref.py.

  prepare_scaled_ref   sdmoe_prepare_input_scaled: fp32(lat * lat_scale), then fp16(fp32(that * in_scale)). Two separately
                       rounded fp32 products cannot contract into one FMA, so the result is exact.
  x0_step_ref          one call of sdmoe_cfg_x0_step (m -> x0 -> x' -> store -> lat). With
                         X0 = |cx| |x| + |cm| |m|max,  |m|max = |eu| + g (|ec| + |eu|)  (step_loop_ref.cfg_eps),
                       the stored x0 is within (3 + STORE_C) u X0 (two products and a sum, plus the CFG combine on m) and
                       lat within SIGMA_C u (|a| |x| + |b0| X0 + |b1| |p|): three roundings in x0, five in x', plus the
                       CFG combine on the model-output term, each on a partial no larger than the bracket.
  sigma_schedule_ref   a whole schedule through x0_step_ref in float64 with the propagated bound
                         E_x0 = |cx| E_lat + (3 + STORE_C) u X0        (m is exact in float64: fp16 inputs)
                         E'   = |a + b0 cx| E_lat + |b1| E_prev + local    (a x + b0 cx x is linear in the one x)
                       prev_x0 and its bound start as NaN: a step that does not set use_prev never reads them. The first
                       input's scaling starts E_lat at 2 u |x| (the product and the fp32 rounding of init_noise_sigma).
  EulerRef, DPMSolverPPRef
                       the schedulers in float64, written in diffusers' operation order (scheduling_euler_discrete.py:
                       pred_original_sample, derivative, dt; scheduling_dpmsolver_multistep.py: _sigma_to_alpha_sigma_t,
                       convert_model_output, the first-order update and the midpoint second-order update with D0, D1, r0
                       and exp(-h) - 1), NOT from the collapsed (a, b0, b1): the collapse of pipeline.euler_schedule /
                       dpmpp_2m_schedule is what they check. diffusers is not installed here, so these restate its
                       formulas; they are not pinned against diffusers itself.

Scalars that cross the C ABI as float (guidance, coef[6], the two scales) are rounded to fp32 first.

SIGMA_C = 8 + STORE_C = 12.42. What an fp32 numpy restatement (kernel operation order, no FMA contraction) reaches of
the bounds, measured by tests/test_sigma_step_host.py on the GPU tests' inputs (N(0,1) latents, prev_x0 and model
outputs, guidance 7.5):
  one call   0.269 of the lat bound (= 3.35 u times the bracket) and 0.263 of the stored-x0 bound over the 21
             coefficient sets, four flag pairs, three eps layouts, B, HW and CFG on / off; 0.252 and 0.382 at the
             grid-stride size
  schedules  free-running, 6 and 50 calls against EulerRef / DPMSolverPPRef: 0.059 of the propagated bound at most
             (Euler "linspace", epsilon, 6 steps)
The restatement stays well inside the constant, so it is kept as reasoned (step_loop_ref's twice-the-measured rule is not
needed).
"""
import numpy as np
import torch

from step_loop_ref import STORE_C, U, bits_equal, cfg_eps, f32, f64

SIGMA_C = 8 + STORE_C
X0_C = 3 + STORE_C
PREDICTION_TYPES = ("epsilon", "v_prediction")
HAND_COEF = [0.625, -1.75, 0.8125, 0.4375, -0.21875, 0.3125]  # all six entries non-trivial
FLAG_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]


# ---- sdmoe_prepare_input_scaled -------------------------------------------------------------------------------------

def prepare_scaled_ref(lat, ncopy, lat_scale, in_scale):
    """lat [B, 4, H, W] fp32 (CPU) -> (scaled lat fp32 numpy, rows [ncopy * B * H * W, 4] fp16 numpy). Exact."""
    x = lat.detach().cpu().numpy().astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = (x * np.float32(lat_scale)).astype(np.float32)
        out = (scaled * np.float32(in_scale)).astype(np.float32).astype(np.float16)
    rows = out.transpose(0, 2, 3, 1).reshape(-1, 4)
    return scaled, np.tile(rows, (ncopy, 1))


# ---- one call of sdmoe_cfg_x0_step ----------------------------------------------------------------------------------

class X0Result:
    __slots__ = ("lat", "x0", "prev", "bound", "x0_bound", "X0", "mmax")


def x0_step_ref(lat, prev, eu, ec, do_cfg, g, coef, flags, round_coef=True):
    """lat, prev [B, 4, HW] (prev may be None when both flags are 0); coef = [cx, cm, a, b0, b1, in_scale]; flags =
    [use_prev, store_prev]. Returns the value (.lat), the x0 (.x0), prev_x0 after the call (.prev) and the per-element
    bounds (.bound of lat, .x0_bound of the stored x0). prev is not read when use_prev is 0."""
    x = f64(lat)
    cx, cm, a, b0, b1, _ = [f32(v) if round_coef else float(v) for v in coef]
    use_prev, store_prev = (int(v) for v in flags)
    m, mmax = cfg_eps(eu, ec, do_cfg, g)
    r = X0Result()
    r.mmax = mmax
    r.X0 = abs(cx) * np.abs(x) + abs(cm) * mmax
    r.x0 = cx * x + cm * m
    val = a * x + b0 * r.x0
    mag = abs(a) * np.abs(x) + abs(b0) * r.X0
    if use_prev:
        p = f64(prev)
        val = val + b1 * p
        mag = mag + abs(b1) * np.abs(p)
    r.lat = val
    r.bound = SIGMA_C * U * mag
    r.x0_bound = X0_C * U * r.X0
    r.prev = r.x0.copy() if store_prev else (None if prev is None else f64(prev).copy())
    return r


def x0_call_failures(r, flags, pre, post):
    """Everything one call must satisfy. r: x0_step_ref of the pre-call state; pre / post: (lat, prev_x0) fp32 arrays
    before and after. Returns (failures, |lat - ref| / bound at its largest, the same for the stored x0)."""
    use_prev, store_prev = (int(v) for v in flags)
    (lat0, prev0), (lat, prev) = pre, post
    fails = []
    if not np.isfinite(lat).all():
        fails.append("lat is not finite")
    err = np.abs(f64(lat) - r.lat)
    if not (err <= r.bound).all():
        fails.append(f"lat off by {np.nanmax(err / r.bound):.3g} of its bound")
    sfrac = 0.0
    if store_prev:
        serr = np.abs(f64(prev) - r.x0)
        if not (serr <= r.x0_bound).all():
            fails.append(f"stored x0 off by {np.nanmax(serr / np.maximum(r.x0_bound, 1e-300)):.3g} of its bound")
        nz = r.x0_bound > 0
        sfrac = float(np.nanmax(serr[nz] / r.x0_bound[nz])) if nz.any() else 0.0
    elif prev0 is not None and not bits_equal(prev, prev0):
        fails.append("prev_x0 changed without store_prev")
    nz = r.bound > 0
    frac = float(np.nanmax(err[nz] / r.bound[nz])) if nz.any() else 0.0
    return fails, frac, sfrac


def coef_cases():
    """(name, coef[6]) of the single-call tests: Euler epsilon and v at steps 0, 25 and 49 (sigma' = 0) of both
    spacings, DPM++ epsilon and v at steps 0, 1, 48 and 49, and one hand-made set."""
    from sdmoe.pipeline import dpmpp_2m_schedule, euler_schedule
    out = []
    for pt in PREDICTION_TYPES:
        for sp in ("leading", "linspace"):
            plan = euler_schedule(50, sp, pt).plan
            out += [(f"euler-{sp}-{pt}-{i}", plan[i][1]) for i in (0, 25, 49)]
        plan = dpmpp_2m_schedule(50, pt).plan
        out += [(f"dpmpp-{pt}-{i}", plan[i][1]) for i in (0, 1, 48, 49)]
    return out + [("hand", HAND_COEF)]


# ---- whole schedules ------------------------------------------------------------------------------------------------

class SigmaScheduleResult:
    __slots__ = ("lat", "prev", "E_lat", "E_prev", "inputs")


def sigma_schedule_ref(lat0, eps_calls, plan, do_cfg, g, lat_scale=1.0, first_in_scale=1.0, round_coef=True,
                       on_call=None):
    """Every call of `plan` ([(t, coef, flags)] of a pipeline.SigmaSchedule) through x0_step_ref in float64 from
    lat0 * lat_scale and a NaN-filled prev_x0, with the propagated bound. eps_calls[i] = (eu, ec) float64 [B, 4, HW].
    .inputs[i] is (the U-Net input of call i in float64 before its fp16 rounding, its bound)."""
    s = f32(lat_scale) if round_coef else float(lat_scale)
    lat = f64(lat0) * s
    E_lat = 2 * U * np.abs(lat) if s != 1.0 else np.zeros_like(lat)
    prev = np.full(lat.shape, np.nan)
    E_prev = np.full(lat.shape, np.nan)
    scale = f32(first_in_scale) if round_coef else float(first_in_scale)
    inputs = []
    for i, (t, coef, flags) in enumerate(plan):
        inputs.append((lat * scale, abs(scale) * (E_lat + 2 * U * np.abs(lat))))
        eu, ec = eps_calls[i]
        r = x0_step_ref(lat, prev, eu, ec, do_cfg, g, coef, flags, round_coef)
        cx, cm, a, b0, b1, scale = [f32(v) if round_coef else float(v) for v in coef]
        E_x0 = abs(cx) * E_lat + r.x0_bound
        E_new = abs(a + b0 * cx) * E_lat + r.bound
        if flags[0]:
            E_new = E_new + abs(b1) * E_prev
        if flags[1]:
            prev, E_prev = r.prev, E_x0
        lat, E_lat = r.lat, E_new
        if on_call is not None:
            on_call(i, t, lat)
    out = SigmaScheduleResult()
    out.lat, out.prev, out.E_lat, out.E_prev, out.inputs = lat, prev, E_lat, E_prev, inputs
    return out


def sigma_table(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
    """((1 - alphas_cumprod) / alphas_cumprod) ** 0.5 of the scaled_linear betas, in fp32 as diffusers computes it."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    return (((1 - ac) / ac) ** 0.5).numpy()


def interp_sigmas(timesteps):
    table = sigma_table()
    s = np.interp(np.asarray(timesteps, dtype=np.float64), np.arange(len(table)), table)
    return np.concatenate([s, [0.0]]).astype(np.float32)


class EulerRef:
    """diffusers EulerDiscreteScheduler (s_churn = 0, interpolation "linear", final sigma 0) in float64."""

    def __init__(self, steps, timestep_spacing="leading", prediction_type="epsilon", steps_offset=1):
        assert prediction_type in PREDICTION_TYPES
        if timestep_spacing == "linspace":
            self.timesteps = np.linspace(0, 999, steps, dtype=np.float32)[::-1].copy()
        else:
            assert timestep_spacing == "leading"
            self.timesteps = (np.arange(0, steps) * (1000 // steps)).round()[::-1].copy().astype(np.float32)
            self.timesteps += steps_offset
        self.sigmas = interp_sigmas(self.timesteps).astype(np.float64)
        smax = self.sigmas.max()
        self.init_noise_sigma = smax if timestep_spacing == "linspace" else (smax ** 2 + 1) ** 0.5
        self.prediction_type = prediction_type

    def scale_model_input(self, sample, i):
        return sample / ((self.sigmas[i] ** 2 + 1) ** 0.5)

    def step(self, model_output, i, sample):
        sigma = self.sigmas[i]
        sigma_hat = sigma  # gamma = 0
        if self.prediction_type == "epsilon":
            pred_original_sample = sample - sigma_hat * model_output
        else:
            pred_original_sample = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        derivative = (sample - pred_original_sample) / sigma_hat
        dt = self.sigmas[i + 1] - sigma_hat
        return sample + derivative * dt


class DPMSolverPPRef:
    """diffusers DPMSolverMultistepScheduler (algorithm_type "dpmsolver++", solver_order 2, solver_type "midpoint",
    lower_order_final, timestep_spacing "linspace", final_sigmas_type "zero") in float64."""

    def __init__(self, steps, prediction_type="epsilon"):
        assert prediction_type in PREDICTION_TYPES
        self.timesteps = np.linspace(0, 999, steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        self.sigmas = interp_sigmas(self.timesteps).astype(np.float64)
        self.init_noise_sigma = 1.0
        self.prediction_type = prediction_type
        self.model_outputs = [None, None]
        self.lower_order_nums = 0

    def scale_model_input(self, sample, i):
        return sample

    @staticmethod
    def _sigma_to_alpha_sigma_t(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def convert_model_output(self, model_output, i, sample):
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[i])
        if self.prediction_type == "epsilon":
            return (sample - sigma_t * model_output) / alpha_t
        return alpha_t * sample - sigma_t * model_output

    def first_order_update(self, x0, i, sample):
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[i + 1])
        alpha_s, sigma_s = self._sigma_to_alpha_sigma_t(self.sigmas[i])
        with np.errstate(divide="ignore"):
            lambda_t = np.log(alpha_t) - np.log(sigma_t)  # +inf at the final sigma 0: exp(-h) - 1 = -1, x_t = x0
        lambda_s = np.log(alpha_s) - np.log(sigma_s)
        h = lambda_t - lambda_s
        return (sigma_t / sigma_s) * sample - (alpha_t * (np.exp(-h) - 1.0)) * x0

    def second_order_update(self, i, sample):
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[i + 1])
        alpha_s0, sigma_s0 = self._sigma_to_alpha_sigma_t(self.sigmas[i])
        alpha_s1, sigma_s1 = self._sigma_to_alpha_sigma_t(self.sigmas[i - 1])
        lambda_t = np.log(alpha_t) - np.log(sigma_t)
        lambda_s0 = np.log(alpha_s0) - np.log(sigma_s0)
        lambda_s1 = np.log(alpha_s1) - np.log(sigma_s1)
        m0, m1 = self.model_outputs[-1], self.model_outputs[-2]
        h, h_0 = lambda_t - lambda_s0, lambda_s0 - lambda_s1
        r0 = h_0 / h
        D0, D1 = m0, (1.0 / r0) * (m0 - m1)
        return ((sigma_t / sigma_s0) * sample - (alpha_t * (np.exp(-h) - 1.0)) * D0
                - 0.5 * (alpha_t * (np.exp(-h) - 1.0)) * D1)

    def step(self, model_output, i, sample):
        lower_order_final = i == len(self.timesteps) - 1  # final_sigmas_type "zero"
        x0 = self.convert_model_output(model_output, i, sample)
        self.model_outputs = [self.model_outputs[1], x0]
        if self.lower_order_nums < 1 or lower_order_final:
            out = self.first_order_update(x0, i, sample)
        else:
            out = self.second_order_update(i, sample)
        if self.lower_order_nums < 2:
            self.lower_order_nums += 1
        return out


def make_ref(kind, steps, prediction_type, spacing=None):
    return DPMSolverPPRef(steps, prediction_type) if kind == "dpmpp_2m" else EulerRef(steps, spacing, prediction_type)


def scheduler_ref_run(sch, lat0, eps_calls, do_cfg, g, on_call=None):
    """latents * init_noise_sigma, then every step of an EulerRef / DPMSolverPPRef on the float64 CFG combine of
    eps_calls[i] = (eu, ec): the final latents. on_call(i, scaled model input, latents after the step)."""
    x = f64(lat0) * sch.init_noise_sigma
    for i in range(len(sch.timesteps)):
        m, _ = cfg_eps(eps_calls[i][0], eps_calls[i][1], do_cfg, g)
        x_in = sch.scale_model_input(x, i)
        x = sch.step(m, i, x)
        if on_call is not None:
            on_call(i, x_in, x)
    return x


SCHEDULE_KINDS = [("euler", "leading"), ("euler", "linspace"), ("dpmpp_2m", None)]
