"""The neuron-level path on the MI355X: sdmoe_geglu_neurons and the NeuronPredictivity / NeuronPredictivityBB /
RemoveNeurons receivers.

Kernel tests take Y = proj(x) as their input, so no GEMM rounding enters and every statement is exact: the product
and the activated gate are compared bit for bit with the existing sdmoe_geglu_route(E = 0), the column maximum as
numbers (-0 == +0) with torch.amax over the same rows of that kernel's gate_out, the overridden columns with
fp16(float(value) * float(fp16(-0.17))) computed by torch on the device.
Receiver tests start from x, so the device GEMM's fp32 summation order enters: outputs and maxima within the project's
fp16-GEMM bar 1e-2 * max(1, |ref|.max()) (tests/test_gpu_discovery.py, tests/test_gpu_wanda.py) of the reference's
fixtures (tests/golden/neuron_*.npz); between two pipelines rel L2 <= 3e-2 (tests/test_gpu_per_prompt.py).
"""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import neuron_ref as R  # noqa: E402
from sdmoe import _lib, discovery, ops  # noqa: E402

DEV = "cuda"
ACTS = {"gelu": ops.ACT_GELU, "relu": ops.ACT_RELU}
OV = -0.17


@functools.lru_cache(maxsize=None)
def case(M, F, act):
    """(Y on the device, the existing kernel's product and activated gate): computed once per shape, never written.
    Every 7th gate column lies in [-3.25, -0.25] on every row, so its maximum is < 0 under gelu (no -0 from a
    saturated tail) and 0 under relu."""
    g = torch.Generator().manual_seed(M * 7 + F)
    y = torch.randn(M, 2 * F, generator=g) * 1.5
    y[:, F::7] = -y[:, F::7].abs().clamp(max=3.0) - 0.25
    y = y.half().to(DEV)
    gate = torch.empty((M, F), dtype=torch.float16, device=DEV)
    out = ops.geglu_route(y, None, ACTS[act], gate_out=gate)
    torch.cuda.synchronize()
    return y, out, gate


def bits_of(mask, F):
    return ops.neuron_bits(mask, DEV)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("M,F", [(128, 320), (512, 1280), (2048, 5120), (200, 1280)])
def test_identity_with_geglu_route(M, F, act):
    y, ref, _ = case(M, F, act)
    assert torch.equal(ops.geglu_neurons(y, ACTS[act]).view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_identity_strided_input(act):
    M, F = 200, 1280
    y, ref, gref = case(M, F, act)
    wide = torch.zeros((M, 2 * F + 64), dtype=torch.float16, device=DEV)
    wide[:, 32:32 + 2 * F] = y
    gate = torch.empty((M, F), dtype=torch.float16, device=DEV)
    out = ops.geglu_neurons(wide[:, 32:32 + 2 * F], ACTS[act], gate_out=gate)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(gate.view(torch.int16), gref.view(torch.int16))


def amax_rows(gate, rpi, groups, ngroups, positions=None):
    g3 = gate.view(-1, rpi, gate.shape[1])
    if positions is not None:
        g3 = g3[:, positions, :]
    return torch.stack([torch.amax(g3[[i for i, gi in enumerate(groups) if gi == g]].reshape(-1, gate.shape[1]), 0)
                        for g in range(ngroups)])


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("rpi,nimg,F", [pytest.param(rpi, nimg, 1280, id=f"{rpi}-{nimg}") for rpi, nimg in
                                        [(64, 4), (256, 4), (1024, 4), (100, 4), (64, 2), (1024, 2), (100, 2)]]
                         + [pytest.param(300, 128, 544, id="300-128-544")])
def test_column_maximum(rpi, nimg, F, act):
    """nimg = 2: img_group None (one group); otherwise image i is in group i % 2. rpi = 100 leaves a partial slab, 1024
    gives several slabs per image; the always-negative columns fail a zero-initialised maximum. Every F = 1280 shape
    runs 64-row slabs (at most 48 blocks of 256 rows). 128 images of 300 rows at F = 544 reach the 256-row slabs:
    128 x 2 x 2 = 512 blocks, the least that takes them, with a 44-row second slab and a partial column block (the
    input of test_gpu_sparsity.test_counts_256_row_slabs)."""
    y, ref, gref = case(nimg * rpi, F, act)
    groups, ng = ([i % 2 for i in range(nimg)], 2) if nimg != 2 else ([0, 0], 1)
    table = torch.tensor(groups, dtype=torch.int32, device=DEV) if nimg != 2 else None
    colmax = torch.full((ng, F), 7.0, dtype=torch.float16, device=DEV)
    out = ops.geglu_neurons(y, ACTS[act], rows_per_img=rpi, img_group=table, ngroups=ng, colmax=colmax)
    want = amax_rows(gref, rpi, groups, ng)
    assert torch.equal(colmax, want)  # equality as numbers
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    if act == "gelu":
        assert bool((colmax[:, ::7] < 0).all())


def box_lists(rpi):
    if rpi == 300:
        return [[256, 270, 299]]  # wholly in the second, 44-row slab of each image: the first contributes nothing
    lists = [[0], [rpi - 1], [0, 3, 5, 17, 31]]
    if rpi == 1024:
        lists.append([1, 40, 63])  # confined to the image's first slab: the others contribute nothing
    return lists


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("rpi", [64, 1024, 300])
def test_bounding_box_positions(rpi, act):
    """rpi = 64 and 1024: 4 images at F = 320, 64-row slabs. rpi = 300: the 128 images at F = 544 of
    test_column_maximum, 256-row slabs (512 blocks), image i in group i % 2."""
    F, nimg = (544, 128) if rpi == 300 else (320, 4)
    groups = [i % 2 for i in range(nimg)]
    y, ref, gref = case(nimg * rpi, F, act)
    table = torch.tensor(groups, dtype=torch.int32, device=DEV)
    for pos in box_lists(rpi):
        colmax = torch.zeros((2, F), dtype=torch.float16, device=DEV)
        out = ops.geglu_neurons(y, ACTS[act], rows_per_img=rpi, img_group=table, ngroups=2, colmax=colmax,
                                pos_bits=ops.position_bits(pos, rpi, DEV))
        assert torch.equal(colmax, amax_rows(gref, rpi, groups, 2, pos)), pos
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), pos


def override_masks(F):
    rng = np.random.default_rng(F)
    last, first = np.zeros(F), np.zeros(F)
    last[F - 1], first[0] = 1, 1
    return {"none": np.zeros(F), "all": np.ones(F), "last": last, "first": first,
            "random": (rng.random(F) < 0.05).astype(np.float64)}


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("which", ["none", "all", "last", "first", "random"])
@pytest.mark.parametrize("M,F,rpi", [(512, 1280, 256), (200, 320, 100)])
def test_gate_override(M, F, rpi, which, act):
    y, ref, gref = case(M, F, act)
    mask = override_masks(F)[which]
    on = torch.from_numpy(mask != 0).to(DEV)
    ov = torch.tensor(OV, dtype=torch.float16, device=DEV)
    assert ov.item() == -0.1700439453125
    want = torch.where(on[None, :], (y[:, :F].float() * ov.float()).half(), ref)
    want_gate = torch.where(on[None, :], ov, gref)
    gate = torch.empty((M, F), dtype=torch.float16, device=DEV)
    colmax = torch.empty((1, F), dtype=torch.float16, device=DEV)
    out = ops.geglu_neurons(y, ACTS[act], override_bits=bits_of(mask, F), override_value=OV, gate_out=gate,
                            rows_per_img=rpi, colmax=colmax)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(gate.view(torch.int16), want_gate.view(torch.int16))
    assert torch.equal(colmax[0], torch.amax(gref, 0))  # the maximum is taken before the override
    if which == "none":
        plain = ops.geglu_neurons(y, ACTS[act], override_bits=None, override_value=OV)
        assert torch.equal(plain.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_guarded_outputs(act):
    """out, gate_out and colmax are views inside poisoned buffers (ldo > F): nothing outside the views changes."""
    M, F, rpi, poison = 200, 320, 100, 777.0
    y, ref, gref = case(M, F, act)
    obuf = torch.full((M + 2, F + 16), poison, dtype=torch.float16, device=DEV)
    gbuf = torch.full((M + 2, F + 16), poison, dtype=torch.float16, device=DEV)
    cbuf = torch.full((4, F), poison, dtype=torch.float16, device=DEV)
    out, gate, colmax = obuf[1:M + 1, 8:8 + F], gbuf[1:M + 1, 8:8 + F], cbuf[1:3]
    mask = override_masks(F)["random"]
    table = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    ops.geglu_neurons(y, ACTS[act], override_bits=bits_of(mask, F), override_value=OV, gate_out=gate, rows_per_img=rpi,
                      img_group=table, ngroups=2, colmax=colmax, out=out)
    assert torch.equal(colmax, amax_rows(gref, rpi, [1, 0], 2))
    off = torch.from_numpy(mask == 0).to(DEV)
    assert torch.equal(out[:, off], ref[:, off]) and torch.equal(gate[:, off], gref[:, off])
    for buf, view in ((obuf, out), (gbuf, gate), (cbuf, colmax)):
        assert bool((view != poison).any())
        view.fill_(poison)
        assert bool((buf == poison).all())


def test_argument_errors_raise():
    y = torch.zeros((64, 656), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.geglu_neurons(y, ops.ACT_RELU)                                   # F = 328
    y = torch.zeros((100, 640), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="pointer/size"):
        ops.geglu_neurons(y, ops.ACT_RELU, rows_per_img=64)                  # M % rows_per_img
    y = torch.zeros((128, 640), dtype=torch.float16, device=DEV)
    colmax = torch.empty((1, 320), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.geglu_neurons(y, ops.ACT_RELU, rows_per_img=64, colmax=colmax,
                          workspace=torch.empty(16, dtype=torch.float32, device=DEV))
    ops.geglu_neurons(y, ops.ACT_RELU, rows_per_img=64, colmax=colmax)       # the shared workspace is large enough
    assert bool((colmax == 0).all())


# ------------------------------------------------------------------------------------------------ receivers
def device_module(c, l):
    from sdmoe.unet import GEGLU, LoRACompatibleLinear, _gelu
    w, b = R.weights(c, l)
    m = GEGLU(LoRACompatibleLinear(w.to(DEV), b.to(DEV)))
    m.gelu = torch.nn.functional.relu if str(c["act"]) == "relu" else _gelu
    return m


def close(got, ref):
    got, ref = torch.as_tensor(np.asarray(got)).float(), torch.as_tensor(np.asarray(ref)).float()
    return (got - ref).abs().max().item() <= 1e-2 * max(1.0, ref.abs().max().item())


PRED = R.golden("neuron_pred")
PRED_BB = R.golden("neuron_pred_bb")
REMOVE = R.golden("remove_neurons")


@pytest.mark.parametrize("name,c", PRED + PRED_BB, ids=[n for n, _ in PRED + PRED_BB])
def test_predictivity_receivers_vs_golden(name, c):
    from neuron_receivers import NeuronPredictivity, NeuronPredictivityBB
    T, L, boxed = int(c["T"]), int(c["L"]), "bb" in c
    mods = [device_module(c, l) for l in range(2)]
    if boxed:
        for m in mods:
            m.bounding_box = None if bool(c["bb_none"]) else c["bb"].tolist()
    rec = (NeuronPredictivityBB if boxed else NeuronPredictivity)(0, T, L)
    for p in range(2):
        rec.reset_time_layer()
        for call in range(T * L):
            out = rec.hook_fn(mods[call % 2], (R.tokens(c, p, 0, call).to(DEV),), None)
            if (p, call) == (0, 0):
                assert out.shape == c["out0"].shape and close(out.cpu().numpy(), c["out0"])
        rec.flush()
        for t in range(T):
            for l in range(L):
                got = rec.max_gate[t][l]
                assert got.dtype == np.float16 and got.shape == (4 * int(c["C"]),)
                assert close(got, c["max_gate_base"][p, t, l]), (p, t, l)
        assert [rec.timestep, rec.layer] == c["counter_after"].tolist()
    if float(c["gate_bias"]) < 0:
        assert (rec.max_gate[0][0] < 0).any()
    assert rec.predictivity.results["time_steps"][T - 1][L - 1]["std"].n == 2


def test_out_of_range_box_equals_all_tokens():
    from neuron_receivers import NeuronPredictivityBB
    _, c = PRED_BB[0]
    m, x = device_module(c, 0), R.tokens(c, 0, 0, 0).to(DEV)
    got = {}
    for tag, bb in (("all", None), ("oor", [0, 3, 40]), ("empty", []), ("box", [0, 3, 5])):
        m.bounding_box = bb
        rec = NeuronPredictivityBB(0, 1, 16)
        rec.hook_fn(m, (x,), None)
        rec.flush()
        got[tag] = rec.max_gate[0][0]
    assert np.array_equal(got["oor"], got["all"]) and np.array_equal(got["empty"], got["all"])
    assert not np.array_equal(got["box"], got["all"])


@pytest.mark.parametrize("name,c", REMOVE, ids=[n for n, _ in REMOVE])
def test_remove_neurons_receiver_vs_golden(name, c):
    from neuron_receivers import RemoveNeurons
    T, L, Fn = int(c["T"]), int(c["L"]), 4 * int(c["C"])
    masks = {t: {l: (np.zeros(0) if c["mask_empty"][t, l] else
                     np.unpackbits(c["mask_bits"][t, l], count=Fn, bitorder="little")) for l in range(L)}
             for t in range(T)}
    rec = RemoveNeurons.from_masks(0, masks, T, L)
    mods = [device_module(c, l) for l in range(L)]
    stored = c["calls"].tolist()
    for call in range(T * L):
        t, l = call // L, call % L
        assert (rec.timestep, rec.layer) == (t, l)
        out = rec.hook_fn(mods[l], (R.tokens(c, 0, 0, call).to(DEV),), None)
        gate = rec.gates[-1]
        assert not gate.is_cuda and gate.shape == out.shape
        if masks[t][l].size:
            on = np.flatnonzero(masks[t][l])
            assert bool((gate[..., on] == np.float16(OV).item()).all())
        if call in stored:
            i = stored.index(call)
            assert close(out.cpu().numpy(), c["out"][i]) and close(gate.numpy(), c["gate"][i])
    assert [rec.timestep, rec.layer] == c["counter_after"].tolist() and len(rec.gates) == T * L


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_prompt_batch_groups_images_by_prompt(act):
    """4 images, 2 prompts: row p of max_gate is the maximum over images p and p + 2 of the device's own activated
    gate (the existing kernel's gate_out over the same proj.run(x)): exact."""
    from neuron_receivers import NeuronPredictivity
    from sdmoe._lib import SdmoeError
    _, c = [pc for pc in PRED if str(pc[1]["act"]) == act][0]
    m = device_module(c, 0)
    x = R.tokens(c, 0, 0, 0, nimg=4).to(DEV)
    rec = NeuronPredictivity(0, 1, 1)
    rec.set_prompts(["one", "two"])
    out = rec.hook_fn(m, (x,), None)
    rec.flush()
    y = m.proj.run(x.reshape(-1, x.shape[-1]))
    gate = torch.empty((y.shape[0], m.inner_dim), dtype=torch.float16, device=DEV)
    dense = ops.geglu_route(y, None, ACTS[act], gate_out=gate)
    want = R.group_max(gate.cpu().view(4, -1, m.inner_dim), [0, 1, 0, 1], 2)
    got = rec.max_gate[0][0]
    assert got.shape == (2, m.inner_dim) and np.array_equal(got, want.numpy())
    assert torch.equal(out.reshape(dense.shape), dense)
    assert rec.predictivity.results["time_steps"][0][0]["std"].n == 2
    rec.set_prompts(["one", "two", "three"])
    with pytest.raises(SdmoeError):
        rec.hook_fn(m, (x,), None)


def test_through_the_pipeline(tmp_path):
    from test_gpu_unet import moefy_tiny, rel_l2
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    from sdmoe.unet import GEGLU, UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    from neuron_receivers import MOEFy, NeuronPredictivity, RemoveNeurons
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 3), cfg, DEV)
    steps, L = 2, 16
    pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=steps)
    prompt = "a photo of a dog"
    torch.manual_seed(0)
    np.random.seed(0)
    plain = pipe(prompt).images[0]
    rec = NeuronPredictivity(0, steps, L)
    out, _ = rec.observe_activation(pipe, prompt)
    assert rel_l2(out, plain) <= 3e-2
    assert (rec.timestep, rec.layer) == (steps, 0)
    geglus = [m for n, m in unet.named_modules() if isinstance(m, GEGLU) and "ff.net" in n]
    assert len(geglus) == L
    for t in range(steps):
        for l in range(L):
            mg = rec.max_gate[t][l]
            assert mg.dtype == np.float16 and mg.shape == (geglus[l].inner_dim,) and np.isfinite(mg).all()
    rec.predictivity.save(str(tmp_path / "predictivity_base.json"))
    with open(tmp_path / "predictivity_base.json") as f:
        saved = json.load(f)
    assert len(saved["time_steps"]["1"]["15"]["avg"]) == geglus[15].inner_dim
    # a prompt list: one row per prompt
    rec.reset_time_layer()
    rec.observe_activation(pipe, [prompt, "a church"])
    assert rec.max_gate[1][3].shape == (2, geglus[3].inner_dim)
    # nothing overridden: the same kernels on the same inputs as the NeuronPredictivity run
    zero = {t: {l: np.zeros(geglus[l].inner_dim) for l in range(L)} for t in range(steps)}
    out0, _ = RemoveNeurons.from_masks(0, zero, steps, L, store_gates=False).observe_activation(pipe, prompt)
    assert torch.equal(out0, out)
    rng = np.random.default_rng(0)
    some = {t: {l: (rng.random(geglus[l].inner_dim) < 0.05) for l in range(L)} for t in range(steps)}
    discovery.save_neuron_masks(some, str(tmp_path / "masks"))
    rem = RemoveNeurons(0, str(tmp_path / "masks"), steps, L)
    out5, gates = rem.observe_activation(pipe, prompt)
    assert len(gates) == steps * L and (rem.timestep, rem.layer) == (steps, 0)
    assert torch.isfinite(out5).all() and not torch.equal(out5, out)


def test_feedforward_takes_plain_down_projection_and_fused_path_returns():
    """Under a RemoveNeurons hook the GEGLU product is in the natural neuron order and FeedForward runs its ordinary
    down projection; once the hook is removed, a MOEFy run over the same module takes the fused routed path again
    (_out_perm set)."""
    from moefication.helper import modify_ffn
    from neuron_receivers import MOEFy, RemoveNeurons
    from sdmoe.unet import FeedForward, LoRACompatibleLinear
    _, c = [rc for rc in REMOVE if int(rc[1]["C"]) == 320 and str(rc[1]["act"]) == "gelu"][0]
    C, Fn = 320, 1280
    geglu = device_module(c, 0)
    wd, bd = R.synth.down_weights(C, 11)
    ff = FeedForward(geglu, LoRACompatibleLinear(torch.from_numpy(wd).half().to(DEV), torch.from_numpy(bd).half().to(DEV)))
    modify_ffn(geglu, None, 0.2, labels=R.synth.balanced_labels(Fn, Fn // 20, 3))
    x = R.tokens(c, 0, 0, 0).to(DEV)
    x2d = x.reshape(-1, C)
    residual = torch.zeros_like(x2d)
    mask = np.random.default_rng(5).random(Fn) < 0.05
    rem = RemoveNeurons.from_masks(0, {0: {0: mask}, 1: {0: mask}}, 2, 1, store_gates=False)
    hook = rem._register(geglu, rem.hook_fn)
    y = ff.run(x2d, 2, residual)
    assert geglu._out_perm is None and geglu._out_keep is None and (rem.timestep, rem.layer) == (1, 0)
    rem.remove_hooks([hook])
    want, _ = geglu.neurons(x, override_bits=ops.neuron_bits(mask, DEV), override_value=OV)
    assert torch.equal(y, ff.net[2].run(want.reshape(-1, Fn), residual=residual))
    mo = MOEFy(seed=0, store_gates=False)
    hook = mo._register(geglu, mo.hook_fn)
    routed = ff.run(x2d, 2, residual)
    mo.remove_hooks([hook])
    assert geglu._out_perm is not None and torch.isfinite(routed).all() and not torch.equal(routed, y)
