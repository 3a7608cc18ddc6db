"""CPU tests of pipeline.euler_schedule / dpmpp_2m_schedule and of tests/sigma_step_ref.py, the float64 checker of the
sigma-scheduler step kernels (csrc/sigma_step.hip).

  * the schedules: spot values, monotone timesteps, final sigma 0, Euler's a + b0 = 1, the DPM++ last step (0, 1, 0);
  * the collapse: free-running x0_step_ref under the schedules' unrounded (cx, cm, a, b0, b1) equals EulerRef /
    DPMSolverPPRef (diffusers' operation order, float64) to 1e-12 relative, so one per-element form serves both
    schedulers and both prediction types;
  * an fp32 numpy restatement of the kernel, in its operation order, stays inside every bound of the reference (the
    fractions reached are printed; run with -s), and each subtly wrong restatement (the mutants) leaves them.
"""
import math

import numpy as np
import pytest

import sigma_step_ref as S
import step_loop_ref as R
from sdmoe.pipeline import dpmpp_2m_schedule, euler_schedule

F = np.float32
G = R.GUIDANCE
NAN = float("nan")


def schedule(kind, steps, pt, spacing=None):
    return dpmpp_2m_schedule(steps, pt) if kind == "dpmpp_2m" else euler_schedule(steps, spacing, pt)


# ---- fp32 restatement in the kernel's operation order (mutant = one of the deliberate errors) -----------------------

def x0_step32(lat, prev, eu, ec, do_cfg, g, coef, flags, mutant=None):
    """(lat, prev_x0, next_in before its fp16 rounding) after one call, all fp32."""
    cx, cm, a, b0, b1, in_scale = [F(v) for v in coef]
    use_prev, store_prev = flags
    if mutant == "swap_b":
        b0, b1 = b1, b0
    eu = eu.astype(F)
    m = eu + F(g) * (ec.astype(F) - eu) if do_cfg else eu
    x = lat
    prev = None if prev is None else prev.copy()
    x0 = cx * x + cm * m
    if mutant == "store_first" and store_prev:
        prev = x0.copy()
    xp = a * x + b0 * x0
    if use_prev:
        xp = xp + b1 * prev
    if store_prev:
        prev = x0.copy()
    nxt = xp * in_scale
    if mutant == "scale_lat":
        xp = nxt
    assert xp.dtype == F and x0.dtype == F and nxt.dtype == F
    return xp, prev, nxt


def single_inputs(B, H, W, form, do_cfg, seed=3):
    rows = (2 if do_cfg else 1) * B * H * W
    buf, c0, w = R.eps_buffer(rows, form, seed + 4)
    eu, ec = R.eps_planes(buf[:, c0:c0 + w], B, H * W, do_cfg)
    lat = R.planes(R.latents(B, H, W, seed)).astype(F)
    prev = R.planes(R.latents(B, H, W, seed + 20)).astype(F)
    return lat, prev, eu, ec


def single_families():
    for B in (1, 3):
        for H, W in ((5, 10), (16, 16)):
            for form in R.EPS_FORMS:
                for do_cfg in (True, False):
                    yield (B, H * W, form, do_cfg), single_inputs(B, H, W, form, do_cfg), do_cfg


def run_single(inputs, do_cfg, coef, flags, mutant=None):
    lat, prev, eu, ec = inputs
    r = S.x0_step_ref(lat, prev, eu, ec, do_cfg, G, coef, flags)
    out, prev2, _ = x0_step32(lat, prev, eu, ec, do_cfg, G, coef, flags, mutant)
    return S.x0_call_failures(r, flags, (lat, prev), (out, prev2))


def free_run32(sched, lat0, eps_rows, B, HW, do_cfg, lat_scale=None, mutant=None):
    """The fp32 restatement through a whole schedule, as the pipeline drives the kernel."""
    scale = sched.init_noise_sigma if lat_scale is None else lat_scale
    lat = (R.planes(lat0).astype(F) * F(scale)).astype(F)
    prev = np.full(lat.shape, NAN, dtype=F)
    for (t, coef, flags), rows in zip(sched.plan, eps_rows):
        eu, ec = R.eps_planes(rows, B, HW, do_cfg)
        with np.errstate(invalid="ignore", over="ignore"):
            lat, prev, _ = x0_step32(lat, prev, eu, ec, do_cfg, G, coef, flags, mutant)
    return lat


def free_run_fraction(kind, spacing, pt, steps, do_cfg=True, plan_mutant=None, lat_scale=None, seed=11):
    """(|fp32 run - scheduler ref| / propagated bound at its largest, the final fp32 latents)."""
    B, H, W = 2, 5, 5
    sched = schedule(kind, steps, pt, spacing)
    lat0, eps = R.schedule_inputs(steps, B, H, W, do_cfg, seed)
    planes = [R.eps_planes(e, B, H * W, do_cfg) for e in eps]
    s = S.sigma_schedule_ref(R.planes(lat0), planes, sched.plan, do_cfg, G, sched.init_noise_sigma, sched.first_in_scale)
    ref = S.scheduler_ref_run(S.make_ref(kind, steps, pt, spacing), R.planes(lat0), planes, do_cfg, G)
    assert np.isfinite(ref).all() and np.isfinite(s.E_lat).all() and (s.E_lat > 0).all()
    run = sched
    if plan_mutant is not None:
        run = type(sched)(sched.timesteps, sched.sigmas, sched.init_noise_sigma, sched.first_in_scale,
                          plan_mutant(sched))
    got = free_run32(run, lat0, eps, B, H * W, do_cfg, lat_scale)
    with np.errstate(invalid="ignore"):
        frac = np.abs(got.astype(np.float64) - ref) / s.E_lat
    return (float("inf") if not np.isfinite(got).all() else float(frac.max())), got


# ---- the schedules --------------------------------------------------------------------------------------------------

def spot(want, got):
    """The recorded values are printed to 7 or 8 significant digits: agreement to half a unit of the 7th. (fp32
    equality with the formula itself is test_schedule_properties'.)"""
    return all(abs(float(g) - w) <= 5e-7 * abs(w) for w, g in zip(want, got))


def test_spot_values():
    e = euler_schedule(50, "linspace")
    assert np.array_equal(e.timesteps[:3], np.array([999, 978.61224, 958.2245], dtype=F)) and e.timesteps[-1] == 0
    assert e.timesteps.dtype == F and not float(e.timesteps[1]).is_integer()
    assert spot((14.614647, 12.936777, 0.02916753), (e.sigmas[0], e.sigmas[1], e.sigmas[49]))
    assert spot((14.614647,), (e.init_noise_sigma,))
    e = euler_schedule(50, "leading")
    assert e.timesteps[:3].tolist() == [981, 961, 941] and e.timesteps[-1] == 1
    assert spot((13.120416, 11.67605, 0.04131448), (e.sigmas[0], e.sigmas[1], e.sigmas[49]))
    assert spot((13.158469,), (e.init_noise_sigma,))
    assert e.first_in_scale == 1 / math.sqrt(float(e.sigmas[0]) ** 2 + 1)
    d = dpmpp_2m_schedule(50)
    assert d.timesteps[:3].tolist() == [999, 979, 959] and d.timesteps[-1] == 20 and d.timesteps.dtype == np.int64
    assert spot((14.614647, 12.966325, 0.13799095), (d.sigmas[0], d.sigmas[1], d.sigmas[49]))
    assert d.init_noise_sigma == 1 and d.first_in_scale == 1 and all(c[5] == 1 for _, c, _ in d.plan)
    want = [(0.9884, 0.0987, 0), (0.9593, 0.2296, -0.0649), (0.8992, 0.3314, -0.0973), (0.8016, 0.4550, -0.1450),
            (0.6478, 0.6684, -0.2451), (0, 1, 0)]
    for pt in S.PREDICTION_TYPES:
        got = [c[2:5] for _, c, _ in dpmpp_2m_schedule(6, pt).plan]
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-4, got
    assert [f for _, _, f in dpmpp_2m_schedule(6).plan] == [[0, 1], [1, 1], [1, 1], [1, 1], [1, 1], [0, 0]]


@pytest.mark.parametrize("steps", [1, 2, 3, 6, 50])
@pytest.mark.parametrize("pt", S.PREDICTION_TYPES)
def test_schedule_properties(steps, pt):
    for kind, spacing in S.SCHEDULE_KINDS:
        sc = schedule(kind, steps, pt, spacing)
        ref = S.make_ref(kind, steps, pt, spacing)
        assert len(sc.plan) == steps == len(sc.timesteps) and sc.sigmas.shape == (steps + 1,)
        assert np.array_equal(sc.timesteps, ref.timesteps) and sc.timesteps.dtype == ref.timesteps.dtype
        assert [t for t, _, _ in sc.plan] == sc.timesteps.tolist()
        assert sc.sigmas.dtype == F and np.array_equal(sc.sigmas, S.interp_sigmas(sc.timesteps))  # fp32 equality
        assert (np.diff(sc.timesteps) < 0).all() and (np.diff(sc.sigmas) < 0).all()
        assert sc.sigmas[-1] == 0
        assert sc.init_noise_sigma == ref.init_noise_sigma
        assert all(np.isfinite(c).all() for _, c, _ in sc.plan)
        if kind == "euler":
            assert all(c[2] + c[3] == 1 and c[4] == 0 and f == [0, 0] for _, c, f in sc.plan)
            assert sc.plan[-1][1][2] == 0 and sc.plan[-1][1][5] == 1
            for i, (_, c, _) in enumerate(sc.plan):
                assert c[5] == 1 / math.sqrt(float(sc.sigmas[i + 1]) ** 2 + 1)
        else:
            assert sc.plan[-1][1][2:5] == [0, 1, 0] and sc.plan[-1][2] == [0, 0]  # also at steps == 1
            assert [f[0] for _, _, f in sc.plan] == [int(0 < i < steps - 1) for i in range(steps)]
            assert [f[1] for _, _, f in sc.plan] == [int(i < steps - 1) for i in range(steps)]


def test_leading_init_noise_sigma_has_plus_one():
    e = euler_schedule(50, "leading")
    assert e.init_noise_sigma == math.sqrt(float(e.sigmas.max()) ** 2 + 1) > float(e.sigmas.max())


def test_schedule_argument_errors():
    with pytest.raises(ValueError):
        euler_schedule(50, "trailing")
    with pytest.raises(ValueError):
        euler_schedule(50, "leading", "sample")
    with pytest.raises(ValueError):
        dpmpp_2m_schedule(50, "sample")


# ---- the collapse ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [6, 50])
@pytest.mark.parametrize("pt", S.PREDICTION_TYPES)
@pytest.mark.parametrize("kind,spacing", S.SCHEDULE_KINDS)
def test_collapse_identity(kind, spacing, pt, steps):
    """x0_step_ref under the schedule's unrounded coefficients equals the scheduler restatement at every call, and the
    scaled inputs equal its scale_model_input, to 1e-12 relative, from a NaN-filled prev_x0."""
    B, H, W = 2, 5, 5
    sched = schedule(kind, steps, pt, spacing)
    lat0, eps = R.schedule_inputs(steps, B, H, W, True, 11)
    planes = [R.eps_planes(e, B, H * W, True) for e in eps]
    mine, theirs, ins = [], [], []
    s = S.sigma_schedule_ref(R.planes(lat0), planes, sched.plan, True, G, sched.init_noise_sigma, sched.first_in_scale,
                             round_coef=False, on_call=lambda i, t, lat: mine.append(lat))
    ref = S.make_ref(kind, steps, pt, spacing)
    S.scheduler_ref_run(ref, R.planes(lat0), planes, True, G,
                        on_call=lambda i, x_in, x: (ins.append(x_in), theirs.append(x)))
    worst = 0.0
    for i in range(steps):
        assert np.isfinite(mine[i]).all(), i
        rel = np.abs(mine[i] - theirs[i]).max() / np.abs(theirs[i]).max()
        rel_in = np.abs(s.inputs[i][0] - ins[i]).max() / np.abs(ins[i]).max()
        assert rel <= 1e-12 and rel_in <= 1e-12, (i, rel, rel_in)
        worst = max(worst, rel, rel_in)
    # the rounded-coefficient run (what the kernel is given) stays within a fraction of the propagated bound of it
    r = S.sigma_schedule_ref(R.planes(lat0), planes, sched.plan, True, G, sched.init_noise_sigma, sched.first_in_scale)
    assert (np.abs(r.lat - theirs[-1]) <= 0.25 * r.E_lat).all()
    print(f"collapse {kind} {spacing} {pt} {steps}: largest gap {worst:.2g}")


# ---- the fp32 restatement stays inside the bounds -------------------------------------------------------------------

def test_single_call_restatement_within_bounds():
    worst = sworst = 0.0
    for key, inputs, do_cfg in single_families():
        for name, coef in S.coef_cases():
            for flags in S.FLAG_PAIRS:
                fails, frac, sfrac = run_single(inputs, do_cfg, coef, flags)
                assert not fails, (key, name, flags, fails)
                worst, sworst = max(worst, frac), max(sworst, sfrac)
    print(f"x0 step: fp32 restatement reaches {worst:.3f} of the lat bound = {worst * S.SIGMA_C:.2f} * u * bracket, "
          f"{sworst:.3f} of the stored-x0 bound")


def test_unread_prev_is_unread():
    """use_prev = 0 on a NaN-filled prev_x0: the reference and the restatement stay finite, the buffer stays as it is
    without store_prev."""
    inputs = single_inputs(2, 5, 10, "dense8", True)
    lat, _, eu, ec = inputs
    nan = np.full(lat.shape, NAN, dtype=F)
    for name, coef in S.coef_cases():
        fails, _, _ = run_single((lat, nan, eu, ec), True, coef, (0, 0))
        assert not fails, (name, fails)
        r = S.x0_step_ref(lat, None, eu, ec, True, G, coef, (0, 0))
        assert np.isfinite(r.lat).all() and r.prev is None


def test_grid_stride_family_restatement():
    """The full-size inputs of the GPU grid-stride case (B = 2, HW = 529,000), second order with a store."""
    B, H, W = 2, 529, 1000
    coef = dpmpp_2m_schedule(50, "v_prediction").plan[25][1]
    fails, frac, sfrac = run_single(single_inputs(B, H, W, "dense8", True), True, coef, (1, 1))
    assert not fails, fails
    print(f"x0 step grid-stride: {frac:.3f} of the lat bound, {sfrac:.3f} of the stored-x0 bound")


@pytest.mark.parametrize("steps", [6, 50])
@pytest.mark.parametrize("pt", S.PREDICTION_TYPES)
@pytest.mark.parametrize("kind,spacing", S.SCHEDULE_KINDS)
def test_free_running_restatement(kind, spacing, pt, steps):
    frac, _ = free_run_fraction(kind, spacing, pt, steps)
    assert frac <= 1.0, frac
    print(f"free-running {kind} {spacing} {pt} {steps}: {frac:.3f} of the propagated bound")


# ---- mutants: each must leave its bound -----------------------------------------------------------------------------

def test_mutant_swapped_b0_b1():
    hit = total = 0
    for key, inputs, do_cfg in single_families():
        for name, coef in S.coef_cases():
            if coef[3] == coef[4]:
                continue
            fails, _, _ = run_single(inputs, do_cfg, coef, (1, 1), "swap_b")
            total += 1
            hit += bool(fails)
    assert total > 0 and hit == total, (hit, total)


def test_mutant_store_before_read():
    """prev_x0 overwritten before the update reads it: caught wherever both flags are set and b1 is not zero, and only
    there."""
    for key, inputs, do_cfg in single_families():
        for name, coef in S.coef_cases():
            for flags in S.FLAG_PAIRS:
                fails, _, _ = run_single(inputs, do_cfg, coef, flags, "store_first")
                assert bool(fails) == (flags == (1, 1) and coef[4] != 0), (key, name, flags, fails)
    B, H, W, steps = 2, 5, 5, 6
    sched = dpmpp_2m_schedule(steps, "epsilon")
    lat0, eps = R.schedule_inputs(steps, B, H, W, True, 11)
    planes = [R.eps_planes(e, B, H * W, True) for e in eps]
    s = S.sigma_schedule_ref(R.planes(lat0), planes, sched.plan, True, G)
    got = free_run32(sched, lat0, eps, B, H * W, True, mutant="store_first")
    assert (np.abs(got - s.lat) / s.E_lat).max() > 1.0


def test_mutant_in_scale_on_lat():
    hit = total = 0
    for key, inputs, do_cfg in single_families():
        for name, coef in S.coef_cases():
            if coef[5] == 1:
                continue
            fails, _, _ = run_single(inputs, do_cfg, coef, (0, 0), "scale_lat")
            total += 1
            hit += bool(fails)
    assert total >= 8 * 24 and hit == total, (hit, total)
    for spacing in ("leading", "linspace"):
        B, H, W, steps = 2, 5, 5, 6
        sched = euler_schedule(steps, spacing, "epsilon")
        lat0, eps = R.schedule_inputs(steps, B, H, W, True, 11)
        planes = [R.eps_planes(e, B, H * W, True) for e in eps]
        s = S.sigma_schedule_ref(R.planes(lat0), planes, sched.plan, True, G, sched.init_noise_sigma,
                                 sched.first_in_scale)
        got = free_run32(sched, lat0, eps, B, H * W, True, mutant="scale_lat")
        assert (np.abs(got - s.lat) / s.E_lat).max() > 1.0


@pytest.mark.parametrize("steps", [6, 50])
@pytest.mark.parametrize("kind,spacing", S.SCHEDULE_KINDS)
def test_mutant_epsilon_coefficients_for_v(kind, spacing, steps):
    eps_plan = schedule(kind, steps, "epsilon", spacing).plan
    frac, _ = free_run_fraction(kind, spacing, "v_prediction", steps, plan_mutant=lambda s: eps_plan)
    assert frac > 1.0
    v, e = schedule(kind, 50, "v_prediction", spacing).plan, schedule(kind, 50, "epsilon", spacing).plan
    inputs = single_inputs(2, 5, 10, "dense8", True)
    lat, prev, eu, ec = inputs
    for i in (0, 25, 48):
        r = S.x0_step_ref(lat, prev, eu, ec, True, G, v[i][1], v[i][2])
        out, prev2, _ = x0_step32(lat, prev, eu, ec, True, G, e[i][1], e[i][2])
        assert S.x0_call_failures(r, v[i][2], (lat, prev), (out, prev2))[0], i


def unspecial_last_step(sched):
    """dpmpp_2m_schedule's plan with the last step computed as every other: lambda of sigma' = 0 evaluated (+inf), so
    h = inf and r0 = 0 in the second-order coefficients."""
    plan = [list(p) for p in sched.plan]
    n = len(plan)
    if n < 2:
        return sched.plan
    sig = [float(v) for v in sched.sigmas]
    alpha = [1 / math.sqrt(v * v + 1) for v in sig]
    vs = [v * a for v, a in zip(sig, alpha)]
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = [float(np.log(a) - np.log(np.float64(v))) for a, v in zip(alpha, vs)]
        i = n - 1
        h = lam[i + 1] - lam[i]
        E = -alpha[i + 1] * math.expm1(-h)
        r0 = np.float64(lam[i] - lam[i - 1]) / h
        coef = list(plan[i][1])
        coef[2:5] = [vs[i + 1] / vs[i], float(E * (1 + 0.5 / r0)), float(-0.5 * E / r0)]
    plan[i] = [plan[i][0], coef, [1, 0]]
    return [tuple(p) for p in plan]


@pytest.mark.parametrize("steps", [2, 6, 50])
@pytest.mark.parametrize("pt", S.PREDICTION_TYPES)
def test_mutant_last_step_lambda_evaluated(pt, steps):
    sched = dpmpp_2m_schedule(steps, pt)
    bad = unspecial_last_step(sched)
    assert not np.isfinite(bad[-1][1]).all()
    frac, got = free_run_fraction("dpmpp_2m", None, pt, steps, plan_mutant=lambda s: bad)
    assert not np.isfinite(got).all() and frac > 1.0
    # and the per-call checker reports it
    inputs = single_inputs(2, 5, 10, "dense8", True)
    lat, prev, eu, ec = inputs
    r = S.x0_step_ref(lat, prev, eu, ec, True, G, sched.plan[-1][1], sched.plan[-1][2])
    with np.errstate(invalid="ignore", over="ignore"):
        out, prev2, _ = x0_step32(lat, prev, eu, ec, True, G, bad[-1][1], bad[-1][2])
    fails = S.x0_call_failures(r, sched.plan[-1][2], (lat, prev), (out, prev2))[0]
    assert "lat is not finite" in fails


@pytest.mark.parametrize("steps", [6, 50])
@pytest.mark.parametrize("pt", S.PREDICTION_TYPES)
def test_mutant_leading_init_sigma_without_plus_one(pt, steps):
    sched = euler_schedule(steps, "leading", pt)
    frac, _ = free_run_fraction("euler", "leading", pt, steps, lat_scale=float(sched.sigmas.max()))
    assert frac > 1.0
    ok, _ = free_run_fraction("euler", "leading", pt, steps, lat_scale=sched.init_noise_sigma)
    assert ok <= 1.0


def test_pipeline_arguments():
    """Constructor checks need no device: unknown names, v-prediction on the epsilon-only schedulers, the default
    spacing per model family."""
    from types import SimpleNamespace
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline as P
    unet, xl = SimpleNamespace(config=UNetConfig.tiny(16)), SimpleNamespace(config=UNetConfig.tiny_xl(16))
    with pytest.raises(ValueError, match="'euler', 'dpmpp_2m'"):
        P(unet, "cpu", scheduler="heun")
    with pytest.raises(ValueError, match="v_prediction"):
        P(unet, "cpu", scheduler="dpmpp_2m", prediction_type="sample")
    for name in ("ddim", "pndm"):
        with pytest.raises(ValueError, match="epsilon-only"):
            P(unet, "cpu", scheduler=name, prediction_type="v_prediction")
    with pytest.raises(ValueError, match="timestep_spacing"):
        P(unet, "cpu", scheduler="dpmpp_2m", timestep_spacing="leading")
    with pytest.raises(ValueError, match="timestep_spacing"):
        P(unet, "cpu", scheduler="euler", timestep_spacing="trailing")
    assert P(unet, "cpu", scheduler="euler").timestep_spacing == "linspace"
    assert P(xl, "cpu", scheduler="euler").timestep_spacing == "leading"
    assert P(xl, "cpu", scheduler="euler", timestep_spacing="linspace").timestep_spacing == "linspace"
    p = P(unet, "cpu", scheduler="dpmpp_2m", prediction_type="v_prediction")
    assert p.sigma_schedule(6).plan == dpmpp_2m_schedule(6, "v_prediction").plan
    assert P(xl, "cpu", scheduler="euler").sigma_schedule(6).plan == euler_schedule(6, "leading", "epsilon").plan
    assert P(unet, "cpu").scheduler == "ddim" and P(unet, "cpu").prediction_type == "epsilon"


def test_prepare_scaled_ref():
    """With both scales 1 it is step_loop_ref.prepare_ref and leaves lat alone; otherwise two fp32 products."""
    lat = R.prepare_latents(2, 5, 7, 1)
    scaled, rows = S.prepare_scaled_ref(lat, 2, 1.0, 1.0)
    assert R.bits_equal(scaled, lat.numpy()) and R.bits_equal(rows, R.prepare_ref(lat, 2).numpy())
    s, k = 13.158469, 1 / math.sqrt(13.120416 ** 2 + 1)
    scaled, rows = S.prepare_scaled_ref(lat, 1, s, k)
    x = lat.numpy()
    with np.errstate(over="ignore"):
        assert R.bits_equal(scaled, x * F(s))
    assert np.isinf(rows).any()
