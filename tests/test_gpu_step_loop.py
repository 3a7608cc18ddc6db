"""The denoising-loop step kernels of csrc/misc.hip on the MI355X against the float64 restatements of
tests/step_loop_ref.py: prepare_input, cfg_ddim_step, cfg_multistep_step, timestep_embedding(_rows) and add.

Every bound comes from step_loop_ref (constants and their justification there; tests/test_step_loop_host.py shows on the
CPU that an fp32 restatement stays inside them and that subtly wrong ones do not). The device is compared with itself
only where two paths must agree bit for bit: t_dev against the scalar timestep, the rows kernel against the single-row
kernel, next_in given against None, and reused hist / cur buffers against NaN-fresh ones. Output buffers carry a
sentinel wherever the kernel must not write. Each test prints the largest fraction of its bound the device reached
(pytest -s); nothing is sized from those figures. On the MI355X they were: cfg_ddim_step 0.384 (0.261 at the
grid-stride size); cfg_multistep_step 0.278 per call (0.470 at the grid-stride size), its stored slot 0.403,
free-running 0.048 of the propagated bound; timestep_embedding 0.9997 (nearly all of it the fp16 rounding; it needs
3.31 of TEMB_C = 16).
"""
import numpy as np
import pytest
import torch

import step_loop_ref as R

pytestmark = pytest.mark.gpu

from sdmoe import _lib, ops  # noqa: E402
from sdmoe.pipeline import pndm_schedule  # noqa: E402

DEV = "cuda"
G = R.GUIDANCE
SENT = 123.0
NAN = float("nan")
GRID_B, GRID_H = 5, 460  # B * HW = 1,058,000 > 4096 blocks * 256 threads: the grid-stride loop takes a second trip


def sentinel(rows, cols):
    return torch.full((rows, cols), SENT, dtype=torch.float16, device=DEV)


def untouched(t):
    return bool((t == SENT).all().item())


def same_bits(a, b):
    return R.bits_equal(R.as_bits(a), R.as_bits(b))


def check_next_in(x_in, lat, B, HW, do_cfg):
    """x_in [>= 2 * B * HW rows, >= 4 columns] after a step with next_in: the image copies hold lat.half() in NHWC, the
    second copy only with CFG; everything else keeps the sentinel."""
    want = R.prepare_ref(lat, 1)
    n = B * HW
    assert same_bits(x_in[:n, :4], want), "first image copy is not lat.half()"
    if do_cfg:
        assert same_bits(x_in[n:2 * n, :4], want), "second image copy is not lat.half()"
    else:
        assert untouched(x_in[n:2 * n, :4]), "second image copy written without CFG"
    assert untouched(x_in[:, 4:]) and untouched(x_in[2 * n:]), "wrote outside channels 0..3 of the image rows"


# ---- prepare_input -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ldo", [4, 64])
@pytest.mark.parametrize("ncopy", [1, 2, 3])
@pytest.mark.parametrize("H,W", [(5, 5), (16, 16), (17, 9)])
@pytest.mark.parametrize("B", [1, 3])
def test_prepare_input(B, H, W, ncopy, ldo):
    lat = R.prepare_latents(B, H, W, 1)
    rows = ncopy * B * H * W
    out = sentinel(rows + 3, ldo)
    ops.prepare_input(lat.to(DEV), out[:rows], ncopy)
    ref = R.prepare_ref(lat, ncopy)
    assert torch.isinf(ref).any()
    assert same_bits(out[:rows, :4], ref)
    assert untouched(out[:rows, 4:]) and untouched(out[rows:])


# ---- cfg_ddim_step -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", R.EPS_FORMS)
@pytest.mark.parametrize("H", [5, 17])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("do_cfg", [True, False])
def test_cfg_ddim_step(do_cfg, B, H, form):
    HW = H * H
    lat0 = R.latents(B, H, H, 3)
    buf, c0, w = R.eps_buffer((2 if do_cfg else 1) * B * HW, form, 7)
    eu, ec = R.eps_planes(buf[:, c0:c0 + w], B, HW, do_cfg)
    dbuf = buf.to(DEV)
    eps = dbuf[:, c0:c0 + w]
    worst = 0.0
    for a_t, a_prev in R.ddim_alpha_cases():
        ref, bound = R.ddim_ref(R.planes(lat0), eu, ec, do_cfg, G, a_t, a_prev)
        lat = lat0.to(DEV)
        x_in = sentinel(2 * B * HW + 2, 64)
        ops.cfg_ddim_step(eps, lat, do_cfg, G, a_t, a_prev, next_in=x_in)
        got = R.planes(lat)
        frac = float((np.abs(got - ref) / bound).max())
        worst = max(worst, frac)
        assert (np.abs(got - ref) <= bound).all(), (a_t, a_prev, frac)
        check_next_in(x_in, lat, B, HW, do_cfg)
        lat2 = lat0.to(DEV)
        ops.cfg_ddim_step(eps, lat2, do_cfg, G, a_t, a_prev, next_in=None)
        assert same_bits(lat2, lat), "lat depends on next_in"
    assert same_bits(dbuf, buf), "eps was written"
    print(f"cfg_ddim_step cfg={do_cfg} B={B} HW={HW} {form}: {worst:.3f} of the bound")


# ---- cfg_multistep_step --------------------------------------------------------------------------------------------

class Dev:
    """sdmoe_cfg_multistep_step behind step_loop_ref.teacher_forced's interface."""

    def __init__(self, lat0, do_cfg, hist=None, cur=None, ldn=64):
        self.B, _, self.H, self.W = lat0.shape
        self.HW, self.do_cfg = self.H * self.W, do_cfg
        self.lat = lat0.to(DEV).clone()
        shape = tuple(lat0.shape)
        self.hist = torch.full((4,) + shape, NAN, dtype=torch.float32, device=DEV) if hist is None else hist
        self.cur = torch.full(shape, NAN, dtype=torch.float32, device=DEV) if cur is None else cur
        self.x_in = sentinel(2 * self.B * self.HW + 2, ldn)

    def state(self):
        B, HW = self.B, self.HW
        return (self.lat.cpu().numpy().reshape(B, 4, HW), self.hist.cpu().numpy().reshape(4, B, 4, HW),
                self.cur.cpu().numpy().reshape(B, 4, HW))

    def call(self, i, rows, coef, flags):
        ops.cfg_multistep_step(rows.to(DEV), self.lat, self.do_cfg, G, self.hist, self.cur, coef, flags,
                               next_in=self.x_in)

    def run(self, plan, eps):
        eps = [e.to(DEV) for e in eps]
        for e, (t, coef, flags) in zip(eps, plan):
            ops.cfg_multistep_step(e, self.lat, self.do_cfg, G, self.hist, self.cur, coef, flags, next_in=self.x_in)
        return self.lat


@pytest.mark.parametrize("do_cfg", [True, False])
@pytest.mark.parametrize("steps", [5, 50])
def test_multistep_teacher_forced(steps, do_cfg):
    B, H = 2, 5
    plan = pndm_schedule(steps)
    lat0, eps = R.schedule_inputs(len(plan), B, H, H, do_cfg, 11)
    dev = Dev(lat0, do_cfg)
    fails, frac, sfrac = R.teacher_forced(dev, plan, eps, B, H * H, do_cfg, G)
    assert not fails, fails[:5]
    check_next_in(dev.x_in, dev.lat, B, H * H, do_cfg)
    print(f"cfg_multistep_step {steps} cfg={do_cfg}: per call {frac:.3f} of the lat bound, {sfrac:.3f} of the "
          f"stored-slot bound")


@pytest.mark.parametrize("do_cfg", [True, False])
def test_multistep_free_running(do_cfg):
    B, H, steps = 2, 5, 50
    plan = pndm_schedule(steps)
    assert len(plan) == 51
    lat0, eps = R.schedule_inputs(len(plan), B, H, H, do_cfg, 11)
    got = R.planes(Dev(lat0, do_cfg).run(plan, eps))
    planes = [R.eps_planes(e, B, H * H, do_cfg) for e in eps]
    s = R.multistep_schedule_ref(R.planes(lat0), planes, plan, do_cfg, G)
    ref = R.pndm_ref_run(R.planes(lat0), planes, steps, do_cfg, G)
    assert np.isfinite(ref).all() and np.isfinite(s.E_lat).all()
    frac = float((np.abs(got - ref) / s.E_lat).max())
    assert (np.abs(got - ref) <= s.E_lat).all(), frac
    print(f"cfg_multistep_step free-running cfg={do_cfg}: {frac:.3f} of the propagated bound")


def test_multistep_reused_buffers():
    """A second image on the first one's hist and cur, as the pipeline's _denoise leaves them, equals the same image on
    NaN-filled buffers bit for bit: no slot is read before the schedule has written it."""
    B, H = 2, 5
    plan = pndm_schedule(50)
    lat_a, eps_a = R.schedule_inputs(len(plan), B, H, H, True, 11)
    lat_b, eps_b = R.schedule_inputs(len(plan), B, H, H, True, 101)
    first = Dev(lat_a, True)
    first.run(plan, eps_a)
    assert not torch.isnan(first.hist).any() and not torch.isnan(first.cur).any()
    reused = Dev(lat_b, True, hist=first.hist, cur=first.cur).run(plan, eps_b)
    fresh = Dev(lat_b, True).run(plan, eps_b)
    assert not torch.isnan(fresh).any()
    assert same_bits(reused, fresh)


@pytest.mark.parametrize("case", range(len(R.unit_cases())))
def test_multistep_unit_cases(case):
    """store = -1 leaves hist alone; a store into a slot that is also read uses the old value; src is read before cur is
    saved."""
    B, H = 2, 5
    coef, flags = R.unit_cases()[case]
    lat0, eps = R.schedule_inputs(1, B, H, H, True, 20 + case)
    hist = R.latents(4 * B, H, H, 30 + case).view(4, B, 4, H, H).to(DEV)
    cur = R.latents(B, H, H, 40 + case).to(DEV)
    dev = Dev(lat0, True, hist=hist, cur=cur)
    fails, frac, _ = R.teacher_forced(dev, [(0, coef, flags)], eps, B, H * H, True, G)
    assert not fails, fails


@pytest.mark.parametrize("store", [-2, 4, 7])
def test_multistep_bad_store_slot(store):
    B, H = 1, 5
    lat0, eps = R.schedule_inputs(1, B, H, H, True, 5)
    dev = Dev(lat0, True)
    with pytest.raises(_lib.SdmoeError, match="sdmoe_cfg_multistep_step"):
        dev.call(0, eps[0], R.unit_cases()[0][0], [store, 0, 0])
    assert same_bits(dev.lat, lat0) and torch.isnan(dev.hist).all()


# ---- the grid-stride trip ------------------------------------------------------------------------------------------

def test_grid_stride_prepare_input():
    B, H = GRID_B, GRID_H
    lat = R.prepare_latents(B, H, H, 1)
    rows = B * H * H
    assert rows > 4096 * 256
    out = sentinel(rows + 1, 8)
    ops.prepare_input(lat.to(DEV), out[:rows], 1)
    got = out.cpu()
    assert same_bits(got[:rows, :4], R.prepare_ref(lat, 1))
    assert untouched(got[:rows, 4:]) and untouched(got[rows:])


def test_grid_stride_cfg_ddim_step():
    B, H = GRID_B, GRID_H
    HW = H * H
    a_t, a_prev = R.ddim_alpha_cases()[0]
    lat0 = R.latents(B, H, H, 3)
    buf = R.eps_buffer(2 * B * HW, "dense8", 7)[0]
    eu, ec = R.eps_planes(buf, B, HW, True)
    ref, bound = R.ddim_ref(R.planes(lat0), eu, ec, True, G, a_t, a_prev)
    lat = lat0.to(DEV)
    x_in = sentinel(2 * B * HW + 1, 8)
    ops.cfg_ddim_step(buf.to(DEV), lat, True, G, a_t, a_prev, next_in=x_in)
    lat = lat.cpu()
    err = np.abs(R.planes(lat) - ref)
    assert (err <= bound).all(), float((err / bound).max())
    check_next_in(x_in.cpu(), lat, B, HW, True)
    print(f"cfg_ddim_step grid-stride: {float((err / bound).max()):.3f} of the bound")


def test_grid_stride_cfg_multistep_step():
    B, H = GRID_B, GRID_H
    t, coef, flags = pndm_schedule(50)[10]  # a steady-state call: three history terms and a store
    assert sum(c != 0 for c in coef[1:5]) == 3 and flags[0] >= 0
    lat0, eps = R.schedule_inputs(1, B, H, H, True, 11)
    hist = R.latents(4 * B, H, H, 30).view(4, B, 4, H, H).to(DEV)
    dev = Dev(lat0, True, hist=hist, ldn=8)
    fails, frac, sfrac = R.teacher_forced(dev, [(t, coef, flags)], eps, B, H * H, True, G)
    assert not fails, fails
    check_next_in(dev.x_in.cpu(), dev.lat.cpu(), B, H * H, True)
    print(f"cfg_multistep_step grid-stride: {frac:.3f} of the lat bound, {sfrac:.3f} of the stored-slot bound")


# ---- timestep embedding --------------------------------------------------------------------------------------------

TEMB_PARAMS = [(dim, flip, fs) for dim in (320, 256, 2) for flip in (True, False) for fs in (0.0, 1.0)]


def single_rows(ts, dim, flip, fs, t_dev=None):
    """The single-row kernel once per timestep into one [n, dim] buffer (scalar t, or t_dev[i] with a decoy scalar)."""
    out = torch.empty((len(ts), dim), dtype=torch.float16, device=DEV)
    for i, t in enumerate(ts):
        if t_dev is None:
            ops.timestep_embedding(t, dim, DEV, flip, fs, out=out[i:i + 1])
        else:
            ops.timestep_embedding(-7.0, dim, DEV, flip, fs, out=out[i:i + 1], t_dev=t_dev[i:i + 1])
    return out


@pytest.mark.parametrize("dim,flip,fs", TEMB_PARAMS)
def test_timestep_embedding(dim, flip, fs):
    ts = R.temb_timesteps()
    assert 981.0 in ts and 1.0 in ts and 1024.0 in ts and 0.0 in ts
    out = single_rows(ts, dim, flip, fs)
    host = out.cpu()
    worst, need, fails = 0.0, 0.0, []
    for i, t in enumerate(ts):
        f, frac, c = R.temb_failures(host[i], t, dim, flip, fs)
        fails += f
        worst, need = max(worst, frac), max(need, c)
    assert not fails, fails[:5]
    t_dev = torch.tensor(ts, dtype=torch.float32, device=DEV)
    assert same_bits(single_rows(ts, dim, flip, fs, t_dev=t_dev), out), "t_dev path differs from the scalar path"
    print(f"timestep_embedding dim={dim} flip={flip} shift={fs}: {worst:.4f} of the bound, needs the constant "
          f"{need:.2f}")


def rows_timesteps(n):
    ts = [float(t) for t, _, _ in pndm_schedule(50)]  # 51 calls, 961 twice: what time_embed_table is given
    ids = [1024.0, 1024.0, 0.0, 0.0, 1024.0, 1024.0]
    return {1: ts[:1], 12: ids + ids, 51: ts}[n]


@pytest.mark.parametrize("n", [1, 51])
@pytest.mark.parametrize("dim,flip,fs", TEMB_PARAMS)
def test_timestep_embedding_rows(dim, flip, fs, n):
    ts = rows_timesteps(n)
    want = single_rows(ts, dim, flip, fs).cpu()
    buf = sentinel(n + 1, dim + 8)
    ops.timestep_embedding_rows(torch.tensor(ts, dtype=torch.float32, device=DEV), dim, buf[:n, :dim],
                                flip_sin_to_cos=flip, freq_shift=fs)
    exp = torch.full((n + 1, dim + 8), SENT, dtype=torch.float16)
    exp[:n, :dim] = want
    assert same_bits(buf, exp)


@pytest.mark.parametrize("n", [1, 12, 51])
@pytest.mark.parametrize("dim,flip,fs", TEMB_PARAMS)
def test_timestep_embedding_rows_grouped(dim, flip, fs, n):
    """group = 6 into a [B, p + 6 * dim + 8] buffer at column p, as add_embed_hidden lays out the SDXL time ids:
    sinusoid r lands at (r // 6, p + (r % 6) * dim); n = 1 and n = 51 leave the last image's row partly unwritten."""
    ts = rows_timesteps(n)
    p, nrow = 16, (n + 5) // 6
    want = single_rows(ts, dim, flip, fs).cpu()
    buf = sentinel(nrow + 1, p + 6 * dim + 8)
    ops.timestep_embedding_rows(torch.tensor(ts, dtype=torch.float32, device=DEV), dim, buf[:nrow, p:p + 6 * dim],
                                group=6, flip_sin_to_cos=flip, freq_shift=fs)
    exp = torch.full(tuple(buf.shape), SENT, dtype=torch.float16)
    for r in range(n):
        c = p + (r % 6) * dim
        exp[r // 6, c:c + dim] = want[r]
    assert same_bits(buf, exp)


# ---- add -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 2056, 8 * (4096 * 256 + 3)])
def test_add(n):
    a, b = R.add_inputs(n, 2)
    out = torch.full((n + 8,), SENT, dtype=torch.float16, device=DEV)
    ops.add(a.to(DEV), b.to(DEV), out=out[:n])
    got = out.cpu()
    ref = R.add_ref(a, b)
    assert torch.isinf(ref).any() and not torch.isnan(ref).any()
    assert same_bits(got[:n], ref)
    assert untouched(got[n:])


def test_add_rejects_ragged_length():
    a, b = R.add_inputs(12, 2)
    out = torch.full((12,), SENT, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="sdmoe_add"):
        ops.add(a.to(DEV), b.to(DEV), out=out)
    assert untouched(out)
