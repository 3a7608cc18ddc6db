"""CPU tests of tests/step_loop_ref.py, the float64 checker of the denoising-loop step kernels (csrc/misc.hip).

Three things are shown here, without a GPU, on the input families tests/test_gpu_step_loop.py uses:
  * fp32 numpy restatements of each kernel, in the kernel's operation order, stay inside the reference's bounds, so
    the reference alone satisfies them (the fractions reached are printed; run with -s);
  * multistep_ref, driven by pipeline.pndm_schedule from NaN-filled hist and cur, reproduces oracle.unet_ref.PNDMRef
    in float64 to 1e-12 relative at every call: a zero coefficient means "never read", and the coef / flags encoding
    is the scheduler's;
  * each subtly wrong restatement (the mutants below) breaks its bound on the same inputs: the GPU assertions have
    teeth.
"""
import numpy as np
import pytest
import torch

import step_loop_ref as R
from sdmoe.pipeline import ddim_schedule, pndm_schedule

F = np.float32
G = R.GUIDANCE
NAN = float("nan")


# ---- fp32 restatements in the kernels' operation order (mutant = one of the deliberate errors) ---------------------

def cfg32(eu, ec, do_cfg, g, mutant=None):
    eu = eu.astype(F)
    if not do_cfg:
        return eu
    ec, g = ec.astype(F), F(g)
    if mutant == "swap":
        eu, ec = ec, eu
    if mutant == "guidance":
        return ec + g * (eu - ec)
    return eu + g * (ec - eu)


def ddim32(lat, eu, ec, do_cfg, g, a_t, a_prev, mutant=None):
    a_t, a_prev, one = F(a_t), F(a_prev), F(1)
    sa, sb, sp, sq = np.sqrt(a_t), np.sqrt(one - a_t), np.sqrt(a_prev), np.sqrt(one - a_prev)
    if mutant == "sbsq":
        sb, sq = sq, sb
    e = cfg32(eu, ec, do_cfg, g, mutant)
    x0 = (lat.astype(F) - sb * e) / sa
    out = sp * x0 + sq * e
    assert out.dtype == F
    return out


def multistep32(lat, hist, cur, eu, ec, do_cfg, g, coef, flags, mutant=None):
    c = [F(v) for v in coef]
    store, use_cur, save_cur = flags
    ch = list(c[1:5])
    if mutant == "drop924":
        ch = [F(0) if v == F(-9.0 / 24) else v for v in ch]
    if mutant == "shift" and F(-9.0 / 24) in ch:  # the oldest term read from the neighbouring slot
        j = ch.index(F(-9.0 / 24))
        ch[(j + 1) % 4] = ch[(j + 1) % 4] + ch[j]
        ch[j] = F(0)
    e = cfg32(eu, ec, do_cfg, g)
    hist = hist.copy()
    if mutant == "store_first" and store >= 0:
        hist[store] = e
    mo = c[0] * e
    for j in range(4):
        if ch[j] != 0:
            mo = mo + ch[j] * hist[j]
    if store >= 0:
        hist[store] = e
    src = cur if (use_cur and mutant != "no_use_cur") else lat
    out = c[5] * src - c[6] * mo
    if save_cur:
        cur = out.copy() if mutant == "save_updated" else lat.copy()
    assert out.dtype == F and hist.dtype == F and cur.dtype == F
    return out, hist, cur


def temb32(t, dim, flip, freq_shift, mutant=None):
    """(fp16 output, the fp32 value before the fp16 rounding, the fp32 argument a)."""
    half = dim // 2
    i = np.arange(half).astype(F)
    L = np.log2(F(10000)) if mutant == "log2" else np.log(F(10000))
    den = F(half) - (F(0) if mutant == "nofs" else F(freq_shift))
    with np.errstate(invalid="ignore", divide="ignore"):
        expo = -L * i / den
    a = F(t) * np.exp(expo)
    s, c = np.sin(a), np.cos(a)
    if mutant == "flip":
        flip = not flip
    v = np.concatenate([c, s] if flip else [s, c])
    assert v.dtype == F
    return v.astype(np.float16), v, a


class Host32:
    """The fp32 restatement behind step_loop_ref.teacher_forced's interface."""

    def __init__(self, lat0, B, HW, do_cfg, mutant=None, hist=None, cur=None):
        self.B, self.HW, self.do_cfg, self.mutant = B, HW, do_cfg, mutant
        self.lat = np.asarray(lat0, dtype=F).reshape(B, 4, HW).copy()
        self.hist = np.full((4, B, 4, HW), NAN, dtype=F) if hist is None else hist.copy()
        self.cur = np.full((B, 4, HW), NAN, dtype=F) if cur is None else cur.copy()

    def state(self):
        return self.lat.copy(), self.hist.copy(), self.cur.copy()

    def call(self, i, rows, coef, flags):
        eu, ec = R.eps_planes(rows, self.B, self.HW, self.do_cfg)
        self.lat, self.hist, self.cur = multistep32(self.lat, self.hist, self.cur, eu, ec, self.do_cfg, G, coef, flags,
                                                    self.mutant)


# ---- inputs --------------------------------------------------------------------------------------------------------

def ddim_inputs():
    """Every (B, HW, eps layout, CFG) family of the GPU test: yields (key, lat [B, 4, HW], eu, ec, do_cfg)."""
    for B in (1, 3):
        for H, W in ((5, 5), (17, 17)):
            for form in R.EPS_FORMS:
                for do_cfg in (True, False):
                    rows = (2 if do_cfg else 1) * B * H * W
                    buf, c0, w = R.eps_buffer(rows, form, 7)
                    eu, ec = R.eps_planes(buf[:, c0:c0 + w], B, H * W, do_cfg)
                    yield (B, H * W, form, do_cfg), R.planes(R.latents(B, H, W, 3)), eu, ec, do_cfg


def ddim_fraction(out, ref, bound):
    return float((np.abs(out.astype(np.float64) - ref) / bound).max())


def ddim_mutant_hits(mutant):
    """How many of the (family, schedule point) pairs with CFG the mutant breaks, and how many there are."""
    cases = R.ddim_alpha_cases()
    _, a_t_all, a_prev_all = ddim_schedule(50)
    hit = total = 0
    for key, lat, eu, ec, do_cfg in ddim_inputs():
        if not do_cfg:
            continue
        for k, (a_t, a_prev) in enumerate(cases):
            wrong_prev = a_prev
            if mutant == "aprev":
                if k >= len(R.DDIM_POINTS):
                    continue
                i = R.DDIM_POINTS[k]
                wrong_prev = a_prev_all[i + 1] if i + 1 < 50 else a_prev_all[i - 1]
            ref, bound = R.ddim_ref(lat, eu, ec, do_cfg, G, a_t, a_prev)
            out = ddim32(lat, eu, ec, do_cfg, G, a_t, wrong_prev, None if mutant == "aprev" else mutant)
            total += 1
            hit += ddim_fraction(out, ref, bound) > 1.0
    return hit, total


# ---- the references agree with the restatements --------------------------------------------------------------------

def test_prepare_and_add_references():
    """numpy's fp16 conversion and torch's agree bit for bit on the special values; the tie pairs are ties."""
    for B, (H, W), ncopy in [(1, (5, 5), 1), (3, (17, 9), 3)]:
        lat = R.prepare_latents(B, H, W, 1)
        ref = R.prepare_ref(lat, ncopy)
        assert ref.shape == (ncopy * B * H * W, 4) and ref.dtype == torch.float16
        with np.errstate(over="ignore"):
            mine = np.tile(lat.numpy().transpose(0, 2, 3, 1).astype(np.float16).reshape(-1, 4), (ncopy, 1))
        assert R.bits_equal(mine, ref.numpy())
        assert torch.isinf(ref).any() and (ref == 65504).any()
        sub = (ref.float().abs() > 0) & (ref.float().abs() < 2.0 ** -14)
        assert sub.any()
    for n in (8, 2056):
        a, b = R.add_inputs(n, 2)
        ref = R.add_ref(a, b)
        with np.errstate(over="ignore"):
            mine = (a.numpy().astype(F) + b.numpy().astype(F)).astype(np.float16)
        assert R.bits_equal(mine, ref.numpy())
        assert not torch.isnan(ref).any()
    for x, y in R.ADD_TIES:
        assert (x, y) in R.ADD_PAIRS
        s = abs(x + y)
        ulp = 2.0 ** (np.floor(np.log2(s)) - 10)
        assert (s / (ulp / 2)) % 2 == 1, (x, y)  # an odd multiple of half an ulp: exactly between two fp16 values


def test_ddim_restatement_within_bound():
    worst = 0.0
    for key, lat, eu, ec, do_cfg in ddim_inputs():
        for a_t, a_prev in R.ddim_alpha_cases():
            ref, bound = R.ddim_ref(lat, eu, ec, do_cfg, G, a_t, a_prev)
            assert np.isfinite(ref).all() and (bound > 0).all()
            frac = ddim_fraction(ddim32(lat, eu, ec, do_cfg, G, a_t, a_prev), ref, bound)
            assert frac <= 1.0, (key, a_t, frac)
            worst = max(worst, frac)
    print(f"ddim: fp32 restatement reaches {worst:.3f} of the bound = {worst * R.DDIM_C:.2f} * u * T")


def test_ddim_restatement_all_schedule_points():
    """All 50 points of the schedule (the GPU test runs six of them)."""
    _, a_t, a_prev = ddim_schedule(50)
    lat = R.planes(R.latents(2, 17, 17, 3))
    eu, ec = R.eps_planes(R.eps_buffer(2 * 2 * 289, "dense8", 7)[0], 2, 289, True)
    worst = 0.0
    for s in range(50):
        ref, bound = R.ddim_ref(lat, eu, ec, True, G, a_t[s], a_prev[s])
        worst = max(worst, ddim_fraction(ddim32(lat, eu, ec, True, G, a_t[s], a_prev[s]), ref, bound))
    assert worst <= 1.0
    print(f"ddim, 50 points: {worst:.3f} of the bound")


@pytest.mark.parametrize("steps", [5, 50])
@pytest.mark.parametrize("do_cfg", [True, False])
def test_multistep_restatement_teacher_forced(steps, do_cfg):
    B, H, W = 2, 5, 5
    plan = pndm_schedule(steps)
    lat0, eps = R.schedule_inputs(len(plan), B, H, W, do_cfg, 11)
    fails, frac, sfrac = R.teacher_forced(Host32(lat0, B, H * W, do_cfg), plan, eps, B, H * W, do_cfg, G)
    assert not fails, fails[:5]
    print(f"multistep {steps} cfg={do_cfg}: per call {frac:.3f} of the lat bound, {sfrac:.3f} of the stored-slot bound")


@pytest.mark.parametrize("steps", [5, 50])
@pytest.mark.parametrize("do_cfg", [True, False])
def test_multistep_restatement_free_running(steps, do_cfg):
    """All calls in fp32 against PNDMRef in float64, within the propagated bound."""
    B, H, W = 2, 5, 5
    plan = pndm_schedule(steps)
    lat0, eps = R.schedule_inputs(len(plan), B, H, W, do_cfg, 11)
    impl = Host32(lat0, B, H * W, do_cfg)
    for i, (t, coef, flags) in enumerate(plan):
        impl.call(i, eps[i], coef, flags)
    planes = [R.eps_planes(e, B, H * W, do_cfg) for e in eps]
    s = R.multistep_schedule_ref(R.planes(lat0), planes, plan, do_cfg, G)
    ref = R.pndm_ref_run(R.planes(lat0), planes, steps, do_cfg, G)
    assert np.isfinite(ref).all() and np.isfinite(s.E_lat).all() and (s.E_lat > 0).all()
    frac = float((np.abs(impl.lat.astype(np.float64) - ref) / s.E_lat).max())
    assert frac <= 1.0, frac
    print(f"multistep {steps} cfg={do_cfg} free-running: {frac:.3f} of the propagated bound, "
          f"bound <= {s.E_lat.max():.3g}, |x| <= {np.abs(ref).max():.3g}")


def test_grid_stride_family_restatement():
    """The full-size inputs of the GPU grid-stride cases (4.2 million elements reach further into the tails: this is
    where the stored CFG eps needs more than 2 * u * |e|max, see step_loop_ref's docstring)."""
    B, H = 5, 460
    HW = H * H
    t, coef, flags = pndm_schedule(50)[10]
    lat0, eps = R.schedule_inputs(1, B, H, H, True, 11)
    hist = R.latents(4 * B, H, H, 30).numpy().reshape(4, B, 4, HW)
    impl = Host32(lat0, B, HW, True, hist=hist)
    fails, frac, sfrac = R.teacher_forced(impl, [(t, coef, flags)], eps, B, HW, True, G)
    assert not fails, fails
    print(f"multistep grid-stride: {frac:.3f} of the lat bound; the stored slot reaches {sfrac * R.STORE_C:.3f} * u * "
          f"|e|max = {sfrac:.3f} of its bound")
    a_t, a_prev = R.ddim_alpha_cases()[0]
    eu, ec = R.eps_planes(R.eps_buffer(2 * B * HW, "dense8", 7)[0], B, HW, True)
    lat = R.planes(R.latents(B, H, H, 3))
    ref, bound = R.ddim_ref(lat, eu, ec, True, G, a_t, a_prev)
    frac = ddim_fraction(ddim32(lat, eu, ec, True, G, a_t, a_prev), ref, bound)
    assert frac <= 1.0
    print(f"ddim grid-stride: {frac:.3f} of the bound")


def test_multistep_unit_cases_restatement():
    B, HW = 2, 25
    for k, (coef, flags) in enumerate(R.unit_cases()):
        lat0, eps = R.schedule_inputs(1, B, 5, 5, True, 20 + k)
        hist = R.latents(4 * B, 5, 5, 30 + k).numpy().reshape(4, B, 4, HW)
        cur = R.latents(B, 5, 5, 40 + k).numpy().reshape(B, 4, HW)
        impl = Host32(lat0, B, HW, True, hist=hist, cur=cur)
        fails, frac, _ = R.teacher_forced(impl, [(0, coef, flags)], eps, B, HW, True, G)
        assert not fails and frac <= 1.0, (flags, fails)


@pytest.mark.parametrize("steps", [5, 50])
def test_multistep_ref_reproduces_pndm_scheduler(steps):
    """multistep_ref under pndm_schedule's coef / flags equals the scheduler restatement at every call, in float64 (so
    with unrounded coefficients) to 1e-12 relative, from NaN-filled hist and cur."""
    from oracle.unet_ref import PNDMRef
    B, H, W = 2, 5, 5
    plan = pndm_schedule(steps)
    sch = PNDMRef(steps)
    assert [p[0] for p in plan] == sch.timesteps.tolist() and len(plan) == steps + 1
    lat0, eps = R.schedule_inputs(len(plan), B, H, W, True, 11)
    planes = [R.eps_planes(e, B, H * W, True) for e in eps]
    x = [R.planes(lat0).copy()]
    seen = []

    def on_call(i, t, e, lat):
        x[0] = sch.step(e, int(t), x[0])
        assert np.isfinite(lat).all(), i
        rel = np.abs(lat - x[0]).max() / np.abs(x[0]).max()
        assert rel <= 1e-12, (i, rel)
        seen.append(rel)

    s = R.multistep_schedule_ref(R.planes(lat0), planes, plan, True, G, round_coef=False, on_call=on_call)
    assert len(seen) == len(plan) and np.isfinite(s.E_lat).all()
    # the rounded-coefficient run (what the kernel is given) stays within a few u of it
    r = R.multistep_schedule_ref(R.planes(lat0), planes, plan, True, G)
    assert np.abs(r.lat - x[0]).max() <= 0.25 * r.E_lat.max()


def test_temb_restatement_within_bound():
    worst = need = 0.0
    for dim in (320, 256, 2):
        for flip in (True, False):
            for fs in (0.0, 1.0):
                for t in R.temb_timesteps():
                    fails, frac, c = R.temb_failures(temb32(t, dim, flip, fs)[0], t, dim, flip, fs)
                    assert not fails, fails
                    worst, need = max(worst, frac), max(need, c)
    assert need <= R.TEMB_C
    print(f"temb: fp16 output reaches {worst:.4f} of the bound and needs the constant {need:.2f}")


def test_temb_ref_matches_oracle_and_nan_case():
    from oracle.unet_ref import timestep_embedding
    for t in (1.0, 481.0, 981.0, 1024.0):
        for flip in (True, False):
            for fs in (0.0, 1.0):
                val, bound = R.temb_ref(t, 320, flip, fs)
                ref = timestep_embedding(t, 320, flip, fs)[0].double().numpy()
                assert (np.abs(val - ref) <= R.U + bound - R.HALF_ULP).all()  # the oracle's is an fp32 value
    val, _ = R.temb_ref(5.0, 2, True, 1.0)
    assert np.isnan(val).all()  # 0 / 0, as diffusers computes it
    val, _ = R.temb_ref(0.0, 2, True, 0.0)
    assert val.tolist() == [1.0, 0.0]


# ---- mutants: each must break its bound ----------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", ["swap", "guidance", "sbsq", "aprev"])
def test_ddim_mutant_breaks_bound(mutant):
    hit, total = ddim_mutant_hits(mutant)
    print(f"ddim mutant {mutant}: breaks the bound at {hit} of {total} (family, point) pairs")
    assert total > 0 and hit == total


@pytest.mark.parametrize("steps", [5, 50])
@pytest.mark.parametrize("mutant", ["no_use_cur", "save_updated", "shift", "drop924"])
def test_multistep_mutant_breaks_bound(mutant, steps):
    """Teacher-forced, the mutant fails a call while every value is still finite; free-running, it leaves the propagated
    bound."""
    B, H, W = 2, 5, 5
    plan = pndm_schedule(steps)
    lat0, eps = R.schedule_inputs(len(plan), B, H, W, True, 11)
    impl = Host32(lat0, B, H * W, True, mutant=mutant)
    fails, _, _ = R.teacher_forced(impl, plan, eps, B, H * W, True, G)
    assert fails and not any("NaN" in m for _, m in fails), fails[:3]
    first = fails[0][0]
    assert first == {"no_use_cur": 1, "save_updated": 0, "shift": 4, "drop924": 4}[mutant], fails[:3]
    planes = [R.eps_planes(e, B, H * W, True) for e in eps]
    s = R.multistep_schedule_ref(R.planes(lat0), planes, plan, True, G)
    ref = R.pndm_ref_run(R.planes(lat0), planes, steps, True, G)
    assert float((np.abs(impl.lat.astype(np.float64) - ref) / s.E_lat).max()) > 1.0


def test_multistep_mutant_store_before_read():
    """The store lands before the history read: caught where `store` is a slot with a nonzero coefficient."""
    B, HW = 2, 25
    caught = []
    for k, (coef, flags) in enumerate(R.unit_cases()):
        lat0, eps = R.schedule_inputs(1, B, 5, 5, True, 20 + k)
        hist = R.latents(4 * B, 5, 5, 30 + k).numpy().reshape(4, B, 4, HW)
        cur = R.latents(B, 5, 5, 40 + k).numpy().reshape(B, 4, HW)
        impl = Host32(lat0, B, HW, True, mutant="store_first", hist=hist, cur=cur)
        fails, _, _ = R.teacher_forced(impl, [(0, coef, flags)], eps, B, HW, True, G)
        caught.append(bool(fails))
    assert caught == [flags[0] >= 0 for _, flags in R.unit_cases()]


@pytest.mark.parametrize("mutant", ["flip", "nofs", "log2"])
def test_temb_mutant_breaks_bound(mutant):
    hit = total = 0
    for dim in (320, 256):
        for flip in (True, False):
            for fs in ((1.0,) if mutant == "nofs" else (0.0, 1.0)):
                for t in R.temb_timesteps():
                    if t == 0.0:
                        continue  # a = 0 whatever the frequencies are
                    fails, _, _ = R.temb_failures(temb32(t, dim, flip, fs, mutant)[0], t, dim, flip, fs)
                    total += 1
                    hit += bool(fails)
    print(f"temb mutant {mutant}: breaks the bound at {hit} of {total} (t, dim, flip, shift) cases")
    assert hit == total
