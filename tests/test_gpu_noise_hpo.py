"""The HPO path on the MI355X: sdmoe_noise_capture / sdmoe_noise_distance, the pipeline's U-Net output seam and the
BaseUNetReceiver / RemoveNeuronsHPO / RemoveNeuronsNoiseHPO / SaveStates receivers.

Kernel tests compare with tests/noise_ref.py (float64 numpy) on the same fp16 values. Bounds:
  * sums of squares: relative error <= 1e-9 -- float64 sums of <= 2^20 non-negative terms taken in any order differ by
    at most n 2^-53 ~ 1.2e-10 relatively, one division chain adds a little;
  * the L1 sums A, B: EQUAL to numpy's -- with |x| <= 8 every partial sum is an exact multiple of 2^-24 below 2^53
    units, so no order of summation rounds.
Receiver tests start from x, so the device GEMM's fp32 summation order enters: the project's fp16-GEMM bar
1e-2 * max(1, |ref|.max()) against the reference's fixtures (tests/golden/hpo_*.npz, save_states_*.npz).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import neuron_ref as R  # noqa: E402
import noise_ref as NR  # noqa: E402
from sdmoe import _lib, discovery, ops  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 2, 64, 8), (3, 4, 100, 8), (2, 6, 4096, 8), (1, 2, 16384, 4)]  # (T, nimg, HW, ld)
OV16 = np.float16(-0.17).item()


def groups_of(nimg):
    """Image i belongs to prompt i % B, B = nimg / 2 (the rows are [uncond x B ; cond x B])."""
    B = nimg // 2
    return [i % B for i in range(nimg)], B


@functools.lru_cache(maxsize=None)
def case(T, nimg, HW, ld):
    """(a, b on the device as [T, nimg * HW, ld] with zero padding, the float64 reference sums): made once per shape,
    never written. |x| <= 8."""
    g = torch.Generator().manual_seed(T * 1000 + nimg * 100 + HW + ld)
    a4 = torch.randn(T, nimg * HW, 4, generator=g).clamp(-8, 8).half()
    b4 = (a4.float() + 0.05 * torch.randn(T, nimg * HW, 4, generator=g)).clamp(-8, 8).half()
    a = torch.zeros((T, nimg * HW, ld), dtype=torch.float16)
    b = torch.zeros((T, nimg * HW, ld), dtype=torch.float16)
    a[:, :, :4], b[:, :, :4] = a4, b4
    groups, B = groups_of(nimg)
    ref = NR.sums(a4.numpy().reshape(T, nimg, -1), b4.numpy().reshape(T, nimg, -1), groups, B)
    return a.to(DEV), b.to(DEV), ref


def run(a, b, nimg, **kw):
    groups, B = groups_of(nimg)
    table = torch.tensor(groups, dtype=torch.int32, device=DEV)
    out = ops.noise_distance(a, b, nimg, img_group=table, ngroups=B, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def rel(got, ref):
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("T,nimg,HW,ld", SHAPES)
def test_sums_vs_float64_reference(T, nimg, HW, ld):
    a, b, ref = case(T, nimg, HW, ld)
    got = run(a, b, nimg)
    assert got.shape == ref.shape == (T, nimg // 2, 4) and got.dtype == np.float64
    print("rel err S(a-b)^2", rel(got[..., 0], ref[..., 0]), "normalised", rel(got[..., 3], ref[..., 3]))
    assert np.array_equal(got[..., 1], ref[..., 1]) and np.array_equal(got[..., 2], ref[..., 2])  # A, B: exact
    assert rel(got[..., 0], ref[..., 0]) <= 1e-9
    assert rel(got[..., 3], ref[..., 3]) <= 1e-9
    assert (got[..., 0] > 0).all() and (got[..., 3] > 0).all()
    again = run(a, b, nimg)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))  # run to run: bit-identical
    if nimg == 2:  # no table: one group
        none = ops.noise_distance(a, b, nimg).cpu().numpy()
        assert np.array_equal(none.view(np.int64), got.view(np.int64))


@pytest.mark.parametrize("T,nimg,HW,ld", [s for s in SHAPES if s[3] == 8])
def test_poisoned_padding_is_never_read(T, nimg, HW, ld):
    a, b, _ = case(T, nimg, HW, ld)
    clean = run(a, b, nimg)
    pa, pb = a.clone(), b.clone()
    pa[:, :, 4:6], pa[:, :, 6:] = float("nan"), 65504.0
    pb[:, :, 4:6], pb[:, :, 6:] = 65504.0, float("nan")
    got = run(pa, pb, nimg)
    assert np.isfinite(got).all() and np.array_equal(got.view(np.int64), clean.view(np.int64))


@pytest.mark.parametrize("T,nimg,HW,ld", [(3, 4, 100, 8), (1, 2, 16384, 4)])
def test_equal_inputs_give_exact_zero(T, nimg, HW, ld):
    a, _, ref = case(T, nimg, HW, ld)
    got = run(a, a.clone(), nimg)
    assert (got[..., 0] == 0).all() and (got[..., 3] == 0).all()
    assert np.array_equal(got[..., 1], ref[..., 1]) and np.array_equal(got[..., 2], ref[..., 1])
    l2, l1n = discovery.noise_distances(got)
    assert (l2 == 0).all() and (l1n == 0).all()


@pytest.mark.parametrize("T,nimg,HW,ld", [(2, 6, 4096, 8), (3, 4, 100, 8)])
def test_one_fp16_ulp(T, nimg, HW, ld):
    """b = a but for one element one fp16 ulp up: S (a - b)^2 is ulp^2 exactly, and the normalised sum -- every term of
    which is the difference of two nearly equal quotients -- within 1e-9 of the float64 reference. An expanded
    S a^2 / A^2 - 2 S a b / (A B) + S b^2 / B^2, or fp32 accumulation, fails this."""
    a, _, _ = case(T, nimg, HW, ld)
    b = a.clone()
    t, row, ch = T - 1, nimg * HW - 3, 2  # last step, last image: group (nimg - 1) % B
    x = a[t, row, ch].cpu()
    y = torch.nextafter(x, torch.tensor(65504.0, dtype=torch.float16))
    b[t, row, ch] = y
    ulp = float(y.double() - x.double())
    assert ulp > 0
    got = run(a, b, nimg)
    groups, B = groups_of(nimg)
    ref = NR.sums(a[:, :, :4].cpu().numpy().reshape(T, nimg, -1), b[:, :, :4].cpu().numpy().reshape(T, nimg, -1),
                  groups, B)
    g = groups[nimg - 1]
    print("ulp^2", ulp * ulp, "got", got[t, g, 0], "normalised got", got[t, g, 3], "ref", ref[t, g, 3])
    assert got[t, g, 0] == ulp * ulp
    assert ref[t, g, 3] > 0 and abs(got[t, g, 3] - ref[t, g, 3]) <= 1e-9 * ref[t, g, 3]
    other = np.ones((T, B), dtype=bool)
    other[t, g] = False
    assert (got[..., 0][other] == 0).all() and (got[..., 3][other] == 0).all()


def test_all_zero_group_follows_the_clamp():
    """Group 1 (images 1 and 3) is zero in a: A = 0 is clamped to 1e-12, the quotients are 0 and the normalised sum is
    S (b / B)^2; zero in both: every sum is 0. Finite either way."""
    T, nimg, HW, ld = 3, 4, 100, 8
    a, b, _ = case(T, nimg, HW, ld)
    groups, B = groups_of(nimg)
    za = a.clone().view(T, nimg, HW, ld)
    za[:, 1::2] = 0
    za = za.view(T, nimg * HW, ld)
    for zb in (b, None):
        if zb is None:
            zb = b.clone().view(T, nimg, HW, ld)
            zb[:, 1::2] = 0
            zb = zb.view(T, nimg * HW, ld)
        got = run(za, zb, nimg)
        ref = NR.sums(za[:, :, :4].cpu().numpy().reshape(T, nimg, -1), zb[:, :, :4].cpu().numpy().reshape(T, nimg, -1),
                      groups, B)
        assert np.isfinite(got).all() and (got[:, 1, 1] == 0).all()
        assert np.array_equal(got[..., 1:3], ref[..., 1:3])
        assert np.allclose(got[..., 0], ref[..., 0], rtol=1e-9, atol=0)
        assert np.allclose(got[..., 3], ref[..., 3], rtol=1e-9, atol=0)
    assert (got[:, 1] == 0).all()  # zero in both


def test_guarded_outputs_and_workspace():
    """out is a view inside a sentinel-filled buffer, the workspace exactly as large as documented with sentinel cells
    after it: nothing outside changes."""
    T, nimg, HW, ld = 3, 4, 100, 8
    a, b, ref = case(T, nimg, HW, ld)
    groups, B = groups_of(nimg)
    table = torch.tensor(groups, dtype=torch.int32, device=DEV)
    sentinel = -777.0
    obuf = torch.full((T + 2, B, 4), sentinel, dtype=torch.float64, device=DEV)
    need = 4 * T * nimg * -(-HW // 1024)
    wbuf = torch.full((need + 64,), sentinel, dtype=torch.float64, device=DEV)
    out = ops.noise_distance(a, b, nimg, img_group=table, ngroups=B, out=obuf[1:T + 1], workspace=wbuf[:need])
    assert out.data_ptr() == obuf[1].data_ptr()
    assert np.array_equal(out.cpu().numpy()[..., 1], ref[..., 1])
    assert bool((obuf[0] == sentinel).all()) and bool((obuf[T + 1] == sentinel).all())
    assert bool((wbuf[need:] == sentinel).all()) and bool((wbuf[:need] != sentinel).all())


def test_argument_errors_raise():
    T, nimg, HW, ld = 1, 2, 64, 8
    a, b, _ = case(T, nimg, HW, ld)
    table = torch.zeros(nimg, dtype=torch.int32, device=DEV)
    small = torch.empty(4 * T * nimg - 1, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.noise_distance(a, b, nimg, workspace=small)                              # workspace too small
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.noise_distance(a[:, :, 1:], b[:, :, 1:], nimg)                           # 2-byte aligned rows
    six = torch.zeros((T, nimg * HW, 6), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.noise_distance(six, six, nimg)                                           # leading dimension 6
    with pytest.raises(_lib.SdmoeError, match="pointer/size"):
        ops.noise_distance(a, b, nimg, img_group=table, ngroups=0, out=torch.empty((T, 0, 4), dtype=torch.float64,
                                                                                  device=DEV))
    with pytest.raises(_lib.SdmoeError, match="pointer/size"):
        ops.noise_distance(a, b, nimg, ngroups=2)                                    # two groups need a table
    with pytest.raises(_lib.SdmoeError):
        ops.noise_distance(a.cpu(), b.cpu(), nimg)                                   # no CPU path
    with pytest.raises(ValueError):
        ops.noise_distance(a, b, 3)                                                  # 128 rows are not 3 images
    lib = _lib.load()
    args = (a.data_ptr(), ld, 0, b.data_ptr(), ld, 0)
    ws = torch.empty(64, dtype=torch.float64, device=DEV)
    out = torch.empty(4, dtype=torch.float64, device=DEV)
    assert lib.sdmoe_noise_distance(*args, 1, 2, 0, None, 1, out.data_ptr(), ws.data_ptr(), 64, None) == -1  # HW = 0
    assert lib.sdmoe_noise_distance(*args, 1, 2, 64, None, 1, None, ws.data_ptr(), 64, None) == -1
    eps = torch.zeros((10, 8), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.noise_capture(eps[:, 1:7], torch.empty((10, 4), dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError):
        ops.noise_capture(eps, torch.empty((9, 4), dtype=torch.float16, device=DEV))


@pytest.mark.parametrize("rows", [200, 2 * 4096 + 8])
def test_noise_capture(rows):
    g = torch.Generator().manual_seed(rows)
    eps = torch.randn(rows, 8, generator=g).half()
    eps[:, 4:6], eps[:, 6:] = float("nan"), 65504.0
    eps = eps.to(DEV)
    sentinel = 777.0
    sbuf = torch.full((3, rows, 4), sentinel, dtype=torch.float16, device=DEV)
    ops.noise_capture(eps, sbuf[1])
    assert torch.equal(sbuf[1], eps[:, :4])
    assert bool((sbuf[0] == sentinel).all()) and bool((sbuf[2] == sentinel).all())
    wide = torch.full((rows, 8), sentinel, dtype=torch.float16, device=DEV)  # a store with padding of its own
    ops.noise_capture(eps, wide)
    assert torch.equal(wide[:, :4], eps[:, :4]) and bool((wide[:, 4:] == sentinel).all())


# ------------------------------------------------------------------------------------------------ receivers
class FakeTrial:
    def __init__(self, answers):
        self.answers, self.asked = answers, []

    def suggest_categorical(self, name, choices):
        self.asked.append(name)
        return self.answers[name]


def device_module(c, l):
    from sdmoe.unet import GEGLU, LoRACompatibleLinear, _gelu
    w, b = R.weights(c, l)
    m = GEGLU(LoRACompatibleLinear(w.to(DEV), b.to(DEV)))
    m.gelu = torch.nn.functional.relu if str(c["act"]) == "relu" else _gelu
    return m


def close(got, ref):
    got, ref = torch.as_tensor(np.asarray(got)).float(), torch.as_tensor(np.asarray(ref)).float()
    return (got - ref).abs().max().item() <= 1e-2 * max(1.0, ref.abs().max().item())


def fixture_masks(c):
    T, L, Fn = int(c["T"]), int(c["L"]), 4 * int(c["C"])
    return {t: {l: (np.zeros(0) if c["mask_empty"][t, l] else
                    np.unpackbits(c["mask_bits"][t, l], count=Fn, bitorder="little")) for l in range(L)}
            for t in range(T)}


def nhwc_eps(x):
    """[nimg, 4, H, W] fp16 -> the pipeline's [nimg * HW, 8] eps buffer with poisoned padding."""
    nimg, _, H, W = x.shape
    eps = torch.full((nimg * H * W, 8), float("nan"), dtype=torch.float16)
    eps[:, :4] = x.permute(0, 2, 3, 1).reshape(-1, 4)
    return eps.to(DEV)


HPO = R.golden("hpo_remove")
HPO_NOISE = R.golden("hpo_noise_remove")
SAVE = R.golden("save_states")
BASE = R.golden("base_unet")


@pytest.mark.parametrize("name,c", HPO + HPO_NOISE, ids=[n for n, _ in HPO + HPO_NOISE])
def test_hpo_receivers_vs_golden(name, c):
    from neuron_receivers import RemoveNeuronsHPO, RemoveNeuronsNoiseHPO
    T, L = int(c["T"]), int(c["L"])
    masks = fixture_masks(c)
    noise = "answers" not in c
    trial = FakeTrial({} if noise else {"timestep_10": int(c["answers"][0]), "timestep_11": int(c["answers"][1])})
    rec = (RemoveNeuronsNoiseHPO if noise else RemoveNeuronsHPO)(0, None, T, L, float(c["dof"]), float(c["conf"]),
                                                                  trials_per_layer=trial, masks=masks)
    mods = [device_module(c, l) for l in range(L)]
    stored = c["calls"].tolist()
    removed = kept = 0
    for call in range(T * L):
        t, l = call // L, call % L
        assert (rec.timestep, rec.layer) == (t, l)
        out = rec.hook_fn(mods[l], (R.tokens(c, 0, 0, call).to(DEV),), None)
        gate = rec.gates[-1]
        assert not gate.is_cuda and gate.shape == out.shape
        if masks[t][l].size:
            on = torch.from_numpy(np.flatnonzero(masks[t][l]))
            decision = 1 if noise else rec.update_for_t[t]
            if decision == 1:
                assert bool((gate[..., on] == OV16).all())
                removed += 1
            else:
                assert not bool((gate[..., on] == OV16).any())  # the dense product
                kept += 1
        if call in stored:
            i = stored.index(call)
            assert close(out.cpu().numpy(), c["out"][i]) and close(gate.numpy(), c["gate"][i]), call
    if noise:
        assert trial.asked == [] and kept == 0
        for t in range(T):  # the step store, indexed by the seam's step index
            rec.unet_hook_fn(t, nhwc_eps(torch.from_numpy(c["unet_output"][t])), 2, 64)
        rec.materialise_outputs()
        for t in range(T):
            assert rec.unet_output[t].dtype == torch.float16 and not rec.unet_output[t].is_cuda
            assert torch.equal(rec.unet_output[t], torch.from_numpy(c["unet_output"][t]))
        assert rec.output_copies == 1
        rec.reset_time_layer()
        assert rec.unet_output == {t: [] for t in range(T)}
    else:
        assert trial.asked == c["asked"].tolist() and removed and kept == L
        assert [rec.update_for_t[t] for t in range(T)] == c["update_for_t"].tolist()
        assert [rec.timestep, rec.layer] == c["counter_after"].tolist()


def test_base_unet_receiver_vs_golden():
    from neuron_receivers import BaseUNetReceiver
    (_, c), = BASE
    T = int(c["T"])
    rec = BaseUNetReceiver(0, T, int(c["L"]))
    for t in range(T):
        assert rec.timestep == t
        rec.unet_hook_fn(t, nhwc_eps(torch.from_numpy(c["unet_output"][t])), 2, 64)
    assert rec.timestep == int(c["timestep_after"])
    rec.materialise_outputs()
    for t in range(T):
        assert torch.equal(rec.unet_output[t], torch.from_numpy(c["unet_output"][t]))
    rec.reset_time()
    assert rec.timestep == 0 and rec.unet_output == {t: [] for t in range(T)}
    with pytest.raises(IndexError):
        rec.unet_hook_fn(T, nhwc_eps(torch.from_numpy(c["unet_output"][0])), 2, 64)


def test_save_states_vs_golden(tmp_path):
    from neuron_receivers import SaveStates
    (_, c), = SAVE
    T, L = int(c["T"]), int(c["L"])
    rec = SaveStates(0, T, L)
    mods = [device_module(c, l) for l in range(L)]
    for call in range(T * L):
        t, l = call // L, call % L
        out = rec.hook_fn(mods[l], (R.tokens(c, 0, 0, call).to(DEV),), None)
        gate = rec.hidden_states[t][l]
        assert not gate.is_cuda and gate.dtype == torch.float16 and gate.shape == out.shape
        assert close(out.cpu().numpy(), c["out"][call]) and close(gate.numpy(), c["gate"][call])
    assert [rec.timestep, rec.layer] == c["counter_after"].tolist()
    rec.save(str(tmp_path / "states.pt"))
    back = torch.load(str(tmp_path / "states.pt"))
    assert all(torch.equal(back[t][l], rec.hidden_states[t][l]) for t in range(T) for l in range(L))


# ------------------------------------------------------------------------------------------------ pipeline
STEPS, LAYERS = 12, 16  # timesteps 10 and 11 ask the trial
PROMPT = "a photo of a dog"


@functools.lru_cache(maxsize=None)
def tiny():
    """(pipeline, its GEGLU widths, the bare image of PROMPT, 5 % masks): built once."""
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    from sdmoe.unet import GEGLU, UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 3), cfg, DEV)
    pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=STEPS)
    widths = [m.inner_dim for n, m in unet.named_modules() if isinstance(m, GEGLU) and "ff.net" in n]
    assert len(widths) == LAYERS
    torch.manual_seed(0)
    np.random.seed(0)
    bare = pipe(PROMPT).images[0].clone()
    rng = np.random.default_rng(0)
    some = {t: {l: (rng.random(widths[l]) < 0.05) for l in range(LAYERS)} for t in range(STEPS)}
    return pipe, widths, bare, some


def stack(unet_output, T):
    return np.stack([unet_output[t].numpy() for t in range(T)])


def test_base_unet_receiver_through_the_pipeline():
    from neuron_receivers import BaseUNetReceiver
    pipe, _, bare, _ = tiny()
    rec = BaseUNetReceiver(0, STEPS, LAYERS)
    out, uo = rec.observe_activation(pipe, PROMPT)
    assert torch.equal(out, bare)  # no GEGLU hook: the bare loop's kernels
    assert pipe._unet_output_hooks == [] and rec.timestep == STEPS and rec.output_copies == 1
    for t in range(STEPS):
        assert uo[t].shape == (2, 4, 16, 16) and uo[t].dtype == torch.float16 and not uo[t].is_cuda
        assert torch.isfinite(uo[t]).all()
    assert not torch.equal(uo[0], uo[STEPS - 1])
    quiet = BaseUNetReceiver(0, STEPS, LAYERS, store_outputs=False)
    out2, uo2 = quiet.observe_activation(pipe, PROMPT)
    assert torch.equal(out2, bare) and quiet.output_copies == 0 and uo2 == {t: [] for t in range(STEPS)}
    assert torch.equal(quiet.device_outputs()[0].cpu().view(STEPS, 2, 16, 16, 4).permute(0, 1, 4, 2, 3),
                       torch.from_numpy(stack(uo, STEPS)))
    short = BaseUNetReceiver(0, 5, LAYERS)  # the run raises at U-Net call 5: the hook is removed all the same
    with pytest.raises(IndexError):
        short.observe_activation(pipe, PROMPT)
    assert pipe._unet_output_hooks == []
    torch.manual_seed(0)
    np.random.seed(0)
    assert torch.equal(pipe(PROMPT).images[0], bare)


def test_hpo_receiver_through_the_pipeline():
    from neuron_receivers import RemoveNeurons, RemoveNeuronsHPO
    pipe, _, bare, some = tiny()
    trial = FakeTrial({"timestep_10": 1, "timestep_11": 1})
    ones = RemoveNeuronsHPO(0, None, STEPS, LAYERS, 9, 0.95, trials_per_layer=trial, masks=some, store_gates=False)
    out1, _ = ones.observe_activation(pipe, PROMPT)
    assert trial.asked == ["timestep_10", "timestep_11"]
    want, _ = RemoveNeurons.from_masks(0, some, STEPS, LAYERS, store_gates=False).observe_activation(pipe, PROMPT)
    assert torch.equal(out1, want) and not torch.equal(out1, bare)
    seq = RemoveNeuronsHPO(0, None, STEPS, LAYERS, 9, 0.95, trials_per_layer=[1] * 10 + [0, 0], masks=some,
                           store_gates=False)
    out0, _ = seq.observe_activation(pipe, PROMPT)
    assert torch.isfinite(out0).all() and not torch.equal(out0, out1)
    assert seq.update_for_t[10] == 0 and seq.update_for_t[11] == 0 and seq.update_for_t[9] == 1


def test_noise_hpo_through_the_pipeline():
    from neuron_receivers import BaseUNetReceiver, RemoveNeurons, RemoveNeuronsNoiseHPO
    from sdmoe.discovery import NoiseObjective
    pipe, widths, bare, some = tiny()
    zero = {t: {l: np.zeros(widths[l]) for l in range(LAYERS)} for t in range(STEPS)}
    kw = dict(dof_val=9, conf_val=0.95, trials_per_layer=FakeTrial({}), store_gates=False)
    rec0 = RemoveNeuronsNoiseHPO(0, None, STEPS, LAYERS, masks=zero, **kw)
    out0, _ = rec0.observe_activation(pipe, PROMPT)
    want0, _ = RemoveNeurons.from_masks(0, zero, STEPS, LAYERS, store_gates=False).observe_activation(pipe, PROMPT)
    assert torch.equal(out0, want0) and pipe._unet_output_hooks == []
    base = BaseUNetReceiver(0, STEPS, LAYERS)
    base.observe_activation(pipe, PROMPT)
    rem = RemoveNeuronsNoiseHPO(0, None, STEPS, LAYERS, masks=some, **kw)
    rem.reset_time_layer()
    out5, uo = rem.observe_activation(pipe, PROMPT)
    assert torch.isfinite(out5).all() and not torch.equal(out5, bare) and (rem.timestep, rem.layer) == (STEPS, 0)
    assert uo[STEPS - 1].shape == (2, 4, 16, 16) and rem.output_copies == 1 and kw["trials_per_layer"].asked == []
    l2, l1n = rem.noise_distance_to(base)
    assert l2.shape == l1n.shape == (STEPS, 1) and l2.dtype == np.float64
    assert (l2 > 0).all() and (l1n > 0).all()
    r2, r1n = NR.distances(stack(base.unet_output, STEPS), stack(rem.unet_output, STEPS))
    print("l2", l2[:, 0], "\nl1n", l1n[:, 0])
    assert rel(l2, r2) <= 1e-9 and rel(l1n, r1n) <= 1e-9
    obj = NoiseObjective(STEPS)
    obj.update(l2, l1n)
    assert abs(obj.avg_noise_diff - r2.mean()) <= 1e-9 * r2.mean()
    rem.reset_time_layer()
    assert rem.unet_output == {t: [] for t in range(STEPS)}
    # the base run against itself: exactly zero
    z2, z1n = rec0.noise_distance_to(rec0)
    assert (z2 == 0).all() and (z1n == 0).all()


def test_noise_hpo_prompt_list():
    """Two prompts: [T, 2] arrays, prompt p over images p and p + 2 ([uncond x 2 ; cond x 2])."""
    from neuron_receivers import BaseUNetReceiver, RemoveNeuronsNoiseHPO
    pipe, _, _, some = tiny()
    base_prompts, adj_prompts = [PROMPT, "a church"], [PROMPT + " in van gogh style", "a church in van gogh style"]
    base = BaseUNetReceiver(0, STEPS, LAYERS)
    outs, ub = base.observe_activation(pipe, base_prompts)
    assert len(outs) == 2 and ub[0].shape == (4, 4, 16, 16)
    rem = RemoveNeuronsNoiseHPO(0, None, STEPS, LAYERS, 9, 0.95, masks=some, store_gates=False)
    rem.observe_activation(pipe, adj_prompts)
    l2, l1n = rem.noise_distance_to(base)
    assert l2.shape == l1n.shape == (STEPS, 2) and (l2 > 0).all() and (l1n > 0).all()
    r2, r1n = NR.distances(stack(base.unet_output, STEPS), stack(rem.unet_output, STEPS), [0, 1, 0, 1], 2)
    assert rel(l2, r2) <= 1e-9 and rel(l1n, r1n) <= 1e-9
    assert not np.allclose(l2[:, 0], l2[:, 1])
    single = BaseUNetReceiver(0, STEPS, LAYERS)
    single.observe_activation(pipe, PROMPT)
    with pytest.raises(ValueError):
        rem.noise_distance_to(single)  # 2 images against 4
