"""Float64 restatements (numpy / torch on the CPU, no HIP library) of the denoising-loop step kernels of
csrc/misc.hip, each with a per-element error bound, the checker of tests/test_step_loop_host.py (which proves on the
host that an fp32 restatement in the kernel's operation order stays inside every bound and that subtly wrong ones do
not) and of tests/test_gpu_step_loop.py.

  prepare_ref      sdmoe_prepare_input: lat.permute(0, 2, 3, 1).half(), ncopy times. Exact.
  ddim_ref         sdmoe_cfg_ddim_step. Bound DDIM_C * u * T with u = 2^-24,
                     T = sp/sa * (|x| + sb * |e|max) + sq * |e|max,
                     |e|max = |eu| + g * (|ec| + |eu|)   (|eu| without CFG):
                   eight fp32 roundings, each on a partial no larger than T.
  multistep_ref    one call of sdmoe_cfg_multistep_step (e -> mo -> store -> src / save_cur -> lat). Bound
                     MULTI_C * u * (|a| * |src| + |b| * sum |c| * |term|);
                   the stored slot holds the fp32 CFG eps within STORE_C * u * |e|max.
  multistep_schedule_ref
                   a whole schedule in float64 with the propagated bound
                     E' = |a| * E_src + |b| * (|c_new| * STORE_C * u * |e|max + sum |c_j| * E_hist[j]) + local;
                   the bounds of hist and cur travel with them. A slot whose coefficient is zero is never read: hist and
                   cur (and their bounds) start as NaN and the result must stay finite.
  temb_ref         sdmoe_timestep_embedding(_rows). Bound 2^-12 + TEMB_C * u * |a| with a = t * exp(expo): half an fp16
                   ulp below 1, plus the fp32 logf, division, expf, product and sinf / cosf on an argument of size a.
                   dim = 2 with freq_shift = 1 divides 0 by 0 (as diffusers' get_timestep_embedding does): value NaN.

Scalars that cross the C ABI as float (a_t, a_prev, guidance, coef[7], t, freq_shift) are rounded to fp32 first.

Constants and what an fp32 numpy restatement (kernel operation order, no FMA contraction) reaches of them on the GPU
tests' inputs, measured by tests/test_step_loop_host.py (N(0,1) latents and eps, guidance 7.5):

  DDIM_C  = 8     reaches 3.07 (0.384 of the bound) over the six (a_t, a_prev) points, the three eps layouts, B, HW and
                  CFG on / off; 0.385 over all 50 schedule points; 0.294 at the grid-stride size
  MULTI_C = 8     per call (teacher-forced) 0.278 of the bound over pndm_schedule(5) and (50), 0.459 at the grid-stride
                  size; free-running, 6 and 51 calls against PNDMRef in float64: 0.112 of the propagated bound
                  (which is <= 2.7e-3 absolute on |x| <= 90)
  STORE_C = 4.42  the stored CFG eps. With the constant 2 (fused multiply-add: two roundings; or three with an exact
                  ec - eu) the restatement reaches 0.68 at B * HW = 50 but 2.208 at the grid-stride size: in 3 of its
                  4,232,000 elements |eu| is below 2^-13 |ec|, the fp32 difference of the two fp16 values is itself
                  rounded, and the three roundings line up (the unfused order can reach 3). The reference alone broke
                  the constant 2, so it is twice the host-measured value: 2 * 2.21.
  TEMB_C  = 16    the fp16 output needs the constant 3.31 at most (0.9997 of the bound, nearly all of it the fp16
                  rounding) over every timestep of both 50-step schedules, 1024 and 0, dims 320 / 256 / 2, flip on /
                  off and freq_shift 0 / 1
"""
import numpy as np
import torch

U = 2.0 ** -24
DDIM_C = 8
MULTI_C = 8
STORE_C = 4.42
TEMB_C = 16
HALF_ULP = 2.0 ** -12  # half an fp16 ulp below 1

GUIDANCE = 7.5
DDIM_POINTS = (0, 1, 25, 48, 49)  # indices into ddim_schedule(50); (0.3, 0.5) is added by ddim_alpha_cases()
EPS_FORMS = ("dense8", "dense4", "cols8of24")


def f32(v):
    return float(np.float32(v))


def f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def bits_equal(a, b):
    """Bit identity of two arrays of one dtype and shape (NaN-proof, distinguishes -0 from +0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    w = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((a.view(w) == b.view(w)).all())


# ---- inputs shared by the host and the GPU tests (CPU tensors) ----------------------------------------------------

def latents(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, H, W, generator=g, dtype=torch.float32)


def eps_buffer(rows, form, seed):
    """fp16 U-Net output stand-in in one of the three layouts: returns (buffer, first column, view width). The view
    handed to the kernel is buffer[:, c0:c0 + width]; "cols8of24" is NaN outside its four columns."""
    g = torch.Generator().manual_seed(seed)
    if form == "dense8":
        return torch.randn(rows, 8, generator=g).half(), 0, 8
    if form == "dense4":
        return torch.randn(rows, 4, generator=g).half(), 0, 4
    if form == "cols8of24":
        buf = torch.full((rows, 24), float("nan"), dtype=torch.float16)
        buf[:, 8:12] = torch.randn(rows, 4, generator=g).half()
        return buf, 8, 4
    raise ValueError(form)


def ddim_alpha_cases():
    from sdmoe.pipeline import ddim_schedule
    _, a_t, a_prev = ddim_schedule(50)
    return [(a_t[i], a_prev[i]) for i in DDIM_POINTS] + [(0.3, 0.5)]


def temb_timesteps():
    """Every timestep the two 50-step schedules issue, plus the SDXL time ids 1024 and 0."""
    from sdmoe.pipeline import ddim_schedule, pndm_schedule
    ts = set(ddim_schedule(50)[0]) | {t for t, _, _ in pndm_schedule(50)} | {1024, 0}
    return sorted(float(t) for t in ts)


def unit_cases():
    """Hand-made (coef, flags) of one multistep call: no store; every store slot with a nonzero coefficient on that
    same slot (the update must use the old value); use_cur and save_cur together (src is read before cur is saved)."""
    coef = [0.75, -0.5, 0.25, 0.375, -0.125, 1.01, 0.3]
    return [(coef, [s, 0, 0]) for s in (-1, 0, 1, 2, 3)] + [(coef, [2, 1, 1]), (coef, [-1, 1, 0]), (coef, [1, 0, 1])]


def prepare_latents(B, H, W, seed):
    """N(0,1) latents with, at the head and the tail of every image, values whose fp16 image is subnormal, zero by a
    rounding tie, the largest finite value, or infinite."""
    lat = latents(B, H, W, seed)
    special = torch.tensor([1e-6, -3e-7, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -25) * 1.5, 6.0e-5, 65504.0, 65519.0, 65520.0,
                            -65520.0, 1e5, -3e38, 0.0, -0.0], dtype=torch.float32)
    flat = lat.view(B, -1)
    k = min(special.numel(), flat.shape[1] // 2)
    flat[:, :k] = special[:k]
    flat[:, -k:] = special[:k].flip(0)
    return lat


ADD_PAIRS = [(float("inf"), 1.0), (float("-inf"), float("-inf")), (-0.0, -0.0), (-0.0, 0.0), (2.0 ** -24, 2.0 ** -24),
             (2048.0, 1.0), (2050.0, 1.0), (65504.0, 16.0),  # the first eight fill the n = 8 case
             (float("-inf"), 3.0), (float("inf"), float("inf")), (0.0, -0.0), (3 * 2.0 ** -24, -(2.0 ** -24)),
             (2.0 ** -14, -(2.0 ** -24)), (-2048.0, -1.0), (1024.0, 0.5), (1025.0, 0.5), (65504.0, 15.0),
             (-65504.0, -16.0)]
ADD_TIES = [(2048.0, 1.0), (2050.0, 1.0), (65504.0, 16.0), (-2048.0, -1.0), (1024.0, 0.5), (1025.0, 0.5),
            (-65504.0, -16.0)]


def add_inputs(n, seed):
    """fp16 a, b [n]: N(0,1) with ADD_PAIRS (infinities, signed zeros, subnormals, sums on a rounding tie) at the head
    and, where they fit, at the tail."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()
    pa = torch.tensor([p[0] for p in ADD_PAIRS], dtype=torch.float16)
    pb = torch.tensor([p[1] for p in ADD_PAIRS], dtype=torch.float16)
    k = min(n, pa.numel())
    a[:k], b[:k] = pa[:k], pb[:k]
    if n >= 2 * pa.numel():
        a[-pa.numel():], b[-pa.numel():] = pa, pb
    return a, b


def add_ref(a, b):
    return (a.cpu().float() + b.cpu().float()).half()


def as_bits(t):
    """fp16 / fp32 torch tensor -> numpy unsigned integers of its bit patterns."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()


# ---- layouts ------------------------------------------------------------------------------------------------------

def prepare_ref(lat, ncopy):
    """[B, 4, H, W] fp32 -> [ncopy * B * H * W, 4] fp16 (exact)."""
    x = lat.detach().cpu().permute(0, 2, 3, 1).half().reshape(-1, 4)
    return x.repeat(ncopy, 1)


def eps_planes(rows, B, HW, do_cfg):
    """fp16 rows [ncopy * B * HW, >= 4] (uncond images first) -> (eu, ec) float64 [B, 4, HW]; ec is None without CFG."""
    r = f64(rows)[:, :4]
    eu = r[:B * HW].reshape(B, HW, 4).transpose(0, 2, 1)
    ec = r[B * HW:2 * B * HW].reshape(B, HW, 4).transpose(0, 2, 1) if do_cfg else None
    return eu, ec


def planes(lat):
    """[..., B, 4, H, W] -> float64 [..., B, 4, HW]."""
    a = f64(lat)
    return a.reshape(a.shape[:-2] + (-1,))


def cfg_eps(eu, ec, do_cfg, g):
    """(e, |e|max) in float64."""
    eu = f64(eu)
    if not do_cfg:
        return eu.copy(), np.abs(eu)
    g, ec = f32(g), f64(ec)
    return eu + g * (ec - eu), np.abs(eu) + abs(g) * (np.abs(ec) + np.abs(eu))


# ---- DDIM ---------------------------------------------------------------------------------------------------------

def ddim_ref(lat, eu, ec, do_cfg, g, a_t, a_prev):
    x = f64(lat)
    e, emax = cfg_eps(eu, ec, do_cfg, g)
    a_t, a_prev = f32(a_t), f32(a_prev)
    sa, sb, sp, sq = np.sqrt(a_t), np.sqrt(1.0 - a_t), np.sqrt(a_prev), np.sqrt(1.0 - a_prev)
    val = sp * ((x - sb * e) / sa) + sq * e
    T = sp / sa * (np.abs(x) + sb * emax) + sq * emax
    return val, DDIM_C * U * T


# ---- PLMS multistep -----------------------------------------------------------------------------------------------

class MultistepResult:
    __slots__ = ("lat", "hist", "cur", "bound", "e", "e_bound", "emax")


def multistep_ref(lat, hist, cur, eu, ec, do_cfg, g, coef, flags, round_coef=True):
    """One call. lat, cur [B, 4, HW]; hist [4, B, 4, HW]; coef = [c_new, c0..c3, a, b]; flags = [store, use_cur,
    save_cur]. A history slot whose coefficient is zero is not read."""
    lat, hist, cur = f64(lat), f64(hist), f64(cur)
    c = [f32(v) if round_coef else float(v) for v in coef]
    store, use_cur, save_cur = (int(v) for v in flags)
    assert -1 <= store <= 3
    e, emax = cfg_eps(eu, ec, do_cfg, g)
    mo, mag = c[0] * e, abs(c[0]) * emax
    for j in range(4):
        if c[1 + j] != 0.0:
            mo = mo + c[1 + j] * hist[j]
            mag = mag + abs(c[1 + j]) * np.abs(hist[j])
    r = MultistepResult()
    r.hist = hist.copy()
    if store >= 0:
        r.hist[store] = e
    src = cur if use_cur else lat
    r.cur = lat.copy() if save_cur else cur.copy()
    r.lat = c[5] * src - c[6] * mo
    r.bound = MULTI_C * U * (abs(c[5]) * np.abs(src) + abs(c[6]) * mag)
    r.e, r.emax, r.e_bound = e, emax, STORE_C * U * emax
    return r


def multistep_call_failures(r, flags, pre, post):
    """Everything one call must satisfy. r: multistep_ref of the pre-call state; pre / post: (lat, hist, cur) fp32
    arrays before and after. Returns (list of failures, |lat - ref| / bound at its largest, the same for the stored
    slot)."""
    store, _, save_cur = (int(v) for v in flags)
    (lat0, hist0, cur0), (lat, hist, cur) = pre, post
    fails = []
    if np.isnan(lat).any():
        fails.append("NaN in lat")
    err = np.abs(f64(lat) - r.lat)
    if not (err <= r.bound).all():
        fails.append(f"lat off by {np.nanmax(err / r.bound):.3g} of its bound")
    sfrac = 0.0
    for j in range(4):
        if j == store:
            serr = np.abs(f64(hist[j]) - r.e)
            if not (serr <= r.e_bound).all():
                over = np.nanmax(serr / np.maximum(r.e_bound, 1e-300))
                fails.append(f"stored slot {j} off by {over:.3g} of its bound")
            nz = r.e_bound > 0
            sfrac = float((serr[nz] / r.e_bound[nz]).max()) if nz.any() else 0.0
        elif not bits_equal(hist[j], hist0[j]):
            fails.append(f"history slot {j} changed (store = {store})")
    if not bits_equal(cur, lat0 if save_cur else cur0):
        fails.append("cur is not the pre-call lat" if save_cur else "cur changed without save_cur")
    nz = r.bound > 0
    frac = float(np.nanmax(err[nz] / r.bound[nz])) if nz.any() else 0.0
    return fails, frac, sfrac


class ScheduleResult:
    __slots__ = ("lat", "hist", "cur", "E_lat", "E_hist", "E_cur")


def multistep_schedule_ref(lat0, eps_calls, plan, do_cfg, g, round_coef=True, on_call=None):
    """Every call of `plan` (pipeline.pndm_schedule) in float64 from NaN-filled hist and cur, with the propagated
    bound. eps_calls[i] = (eu, ec) float64 [B, 4, HW] of call i. on_call(i, t, e, lat) sees each call's result."""
    lat = f64(lat0).copy()
    hist = np.full((4,) + lat.shape, np.nan)
    cur = np.full(lat.shape, np.nan)
    E_lat = np.zeros_like(lat)
    E_hist = np.full_like(hist, np.nan)
    E_cur = np.full_like(lat, np.nan)
    for i, (t, coef, flags) in enumerate(plan):
        eu, ec = eps_calls[i]
        r = multistep_ref(lat, hist, cur, eu, ec, do_cfg, g, coef, flags, round_coef)
        c = [f32(v) for v in coef]
        store, use_cur, save_cur = flags
        E_mo = abs(c[0]) * STORE_C * U * r.emax
        for j in range(4):
            if c[1 + j] != 0.0:
                E_mo = E_mo + abs(c[1 + j]) * E_hist[j]
        E_src = E_cur if use_cur else E_lat
        E_new = abs(c[5]) * E_src + abs(c[6]) * E_mo + r.bound
        if save_cur:
            E_cur = E_lat
        if store >= 0:
            E_hist[store] = STORE_C * U * r.emax
        lat, hist, cur, E_lat = r.lat, r.hist, r.cur, E_new
        if on_call is not None:
            on_call(i, t, r.e, lat)
    s = ScheduleResult()
    s.lat, s.hist, s.cur, s.E_lat, s.E_hist, s.E_cur = lat, hist, cur, E_lat, E_hist, E_cur
    return s


def schedule_inputs(ncalls, B, H, W, do_cfg, seed):
    """(lat0 fp32 [B, 4, H, W], [fresh fp16 eps rows [ncopy * B * HW, 8] per call]) as CPU tensors."""
    rows = (2 if do_cfg else 1) * B * H * W
    return latents(B, H, W, seed), [eps_buffer(rows, "dense8", seed + 1 + i)[0] for i in range(ncalls)]


def teacher_forced(impl, plan, eps_rows, B, HW, do_cfg, g):
    """Drive an implementation through every call of `plan`, checking each call against multistep_ref of the state the
    implementation itself held before it. impl.state() -> (lat [B, 4, HW], hist [4, B, 4, HW], cur [B, 4, HW]) as fp32
    numpy copies; impl.call(i, eps rows, coef, flags) makes call i. Returns ([(call, failure)], largest fraction of the
    lat bound reached, largest fraction of the stored-slot bound)."""
    fails, frac, sfrac = [], 0.0, 0.0
    for i, (t, coef, flags) in enumerate(plan):
        pre = impl.state()
        eu, ec = eps_planes(eps_rows[i], B, HW, do_cfg)
        r = multistep_ref(pre[0], pre[1], pre[2], eu, ec, do_cfg, g, coef, flags)
        impl.call(i, eps_rows[i], coef, flags)
        f, fr, sf = multistep_call_failures(r, flags, pre, impl.state())
        fails += [(i, m) for m in f]
        frac, sfrac = max(frac, fr), max(sfrac, sf)
    return fails, frac, sfrac


def pndm_ref_run(lat0, eps_calls, steps, do_cfg, g):
    """The oracle's PNDMScheduler restatement (oracle.unet_ref.PNDMRef) over all calls in float64: the final latents."""
    from oracle.unet_ref import PNDMRef
    sch = PNDMRef(steps)
    x = f64(lat0).copy()
    for i, t in enumerate(sch.timesteps):
        e, _ = cfg_eps(eps_calls[i][0], eps_calls[i][1], do_cfg, g)
        x = sch.step(e, int(t), x)
    return x


# ---- timestep embedding ---------------------------------------------------------------------------------------------

def temb_ref(t, dim, flip, freq_shift):
    """diffusers get_timestep_embedding(t, dim, flip_sin_to_cos, downscale_freq_shift, max_period=10000) of one t in
    float64: (value [dim], bound [dim])."""
    half = dim // 2
    t, fs = f32(t), f32(freq_shift)
    i = np.arange(half, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        expo = -np.log(10000.0) * i / (half - fs)
    a = t * np.exp(expo)
    s, c = np.sin(a), np.cos(a)
    val = np.concatenate([c, s] if flip else [s, c])
    b = HALF_ULP + TEMB_C * U * np.abs(a)
    return val, np.concatenate([b, b])


def temb_failures(out, t, dim, flip, freq_shift):
    """out: fp16 [dim] against temb_ref: (failures, err / bound at its largest, the constant in TEMB_C's place that this
    output needs, (err - 2^-12) / (u * |a|) at its largest). Where the reference is NaN (0 / 0) the output must be
    NaN."""
    val, bound = temb_ref(t, dim, flip, freq_shift)
    o = f64(out).reshape(-1)
    nan = np.isnan(val)
    fails = []
    if not (np.isnan(o) == nan).all():
        fails.append(f"t={t} dim={dim} flip={flip} shift={freq_shift}: NaN pattern differs")
    err = np.abs(o - val)[~nan]
    frac = float((err / bound[~nan]).max()) if err.size else 0.0
    if not (err <= bound[~nan]).all():
        fails.append(f"t={t} dim={dim} flip={flip} shift={freq_shift}: {frac:.3g} of the bound")
    ua = (bound[~nan] - HALF_ULP) / TEMB_C
    need = float(((err - HALF_ULP)[ua > 0] / ua[ua > 0]).max()) if (ua > 0).any() else 0.0
    return fails, frac, max(need, 0.0)
