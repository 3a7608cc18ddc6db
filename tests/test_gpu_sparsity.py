"""The gate-sparsity measurement on the MI355X: sdmoe_geglu_sparsity and the SparsityMeasure receiver.

Kernel tests take Y = proj(x) as their input, so no GEMM rounding enters and every statement is exact: the product is
compared bit for bit with the existing kernels' (sdmoe_geglu_route(E = 0), which sdmoe_geglu_neurons is pinned to in
tests/test_gpu_neurons.py, and sdmoe_geglu_neurons itself), the counts with torch integer sums on the device over that
kernel's gate_out.
Receiver tests start from x, so the device GEMM's fp32 summation order enters and can move a pre-activation gate
across 0: against the device's own projection the counts stay exact; against the reference's fixtures
(tests/golden/sparsity_*.npz) each count must lie in the bracket spanned by moving every pre-activation gate g of the
CPU restatement by the project's fp16-GEMM bar tol = 1e-2 * max(1, |g|.max()) (tests/test_gpu_neurons.py::close). The
fixtures' generator asserts a relu zero ratio in (0.3, 0.7) and negatives in every gelu call, so no bracket is vacuous.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sparsity_ref as R  # noqa: E402
from sdmoe import _lib, discovery, ops  # noqa: E402
from test_gpu_neurons import ACTS, DEV, case, close, device_module  # noqa: E402  (the shared, never written Y cases)

SPARSITY = R.golden("sparsity")
GROUPS = {"none": None, "1010": [1, 0, 1, 0], "0101": [0, 1, 0, 1]}


def run(y, act, rpi=0, groups=None, ngroups=1, threshold=0.0, arrays=True, totals=True, **kw):
    """One call with fresh, garbage-filled count buffers: (out, col_zero, col_neg, totals)."""
    F = y.shape[1] // 2
    table = None if groups is None else torch.tensor(groups, dtype=torch.int32, device=DEV)
    cz = torch.full((ngroups, F), -7, dtype=torch.int32, device=DEV) if arrays else None
    cn = torch.full((ngroups, F), -7, dtype=torch.int32, device=DEV) if arrays else None
    tt = torch.full((ngroups, 2), -7, dtype=torch.int64, device=DEV) if totals else None
    out = ops.geglu_sparsity(y, act, threshold=threshold, rows_per_img=rpi, img_group=table, ngroups=ngroups,
                             col_zero=cz, col_neg=cn, totals=tt, **kw)
    return out, cz, cn, tt


def want_counts(gate, rpi, groups, ngroups, threshold=0.0):
    nimg = gate.shape[0] // rpi
    return R.group_counts(gate.view(nimg, rpi, -1), groups if groups is not None else [0] * nimg, ngroups, threshold)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("M,F,rpi", [(64, 32, 0), (128, 320, 0), (512, 1280, 0), (200, 1280, 100)])
def test_product_identity(M, F, rpi, act):
    """F = 32: the minimum width; 320: a partially filled column block; 1280: 2.5 blocks; M = 200 in images of 100
    rows: a slab tail (36 rows, 9 per wave) that is not a multiple of the 4-row unroll."""
    y, ref, _ = case(M, F, act)
    out, _, _, _ = run(y, ACTS[act], rpi=rpi)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(out.view(torch.int16), ops.geglu_neurons(y, ACTS[act], rows_per_img=rpi).view(torch.int16))


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_product_identity_strided_input(act):
    M, F = 200, 1280
    y, ref, gref = case(M, F, act)
    wide = torch.zeros((M, 2 * F + 64), dtype=torch.float16, device=DEV)
    wide[:, 32:32 + 2 * F] = y
    gate = torch.empty((M, F), dtype=torch.float16, device=DEV)
    out, cz, cn, tt = run(wide[:, 32:32 + 2 * F], ACTS[act], rpi=100, gate_out=gate)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(gate.view(torch.int16), gref.view(torch.int16))
    wz, wn, wt = want_counts(gref, 100, None, 1)
    assert torch.equal(cz.long(), wz) and torch.equal(cn.long(), wn) and torch.equal(tt, wt)


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("groups", ["none", "1010", "0101"])
@pytest.mark.parametrize("rpi,nimg", [(64, 4), (256, 4), (1024, 4), (100, 4), (100, 2)])
def test_counts(rpi, nimg, groups, act):
    """Every shape here runs 64-row slabs (fewer than 512 blocks of 256 rows): one slab per image at 64, four at 256,
    sixteen at 1024, a 36-row tail at 100. The 256-row slabs are in test_counts_256_row_slabs. Two images take the
    first two entries of the group table."""
    F = 1280
    y, ref, gref = case(nimg * rpi, F, act)
    g = GROUPS[groups] and GROUPS[groups][:nimg]
    ng = 1 if g is None else 2
    out, cz, cn, tt = run(y, ACTS[act], rpi=rpi, groups=g, ngroups=ng)
    wz, wn, wt = want_counts(gref, rpi, g, ng)
    assert torch.equal(cz.long(), wz) and torch.equal(cn.long(), wn) and torch.equal(tt, wt)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    if act == "relu":
        assert int(wt[:, 1].sum()) == 0 and 0 < int(wt[:, 0].sum()) < gref.numel()
    else:
        assert int(wt[:, 1].sum()) > 0


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("groups", ["none", "alternating"])
def test_counts_256_row_slabs(groups, act):
    """The kernel takes 256-row slabs once they give at least 512 blocks: 128 images of 300 rows at F = 544 (two column
    blocks, the second with 4 of 64 chunks) is 128 x 2 x 2 = 512, the smallest such count with a second, partial slab
    per image (44 rows: 11 per wave, a tail that is not a multiple of the unroll) and a partial column block."""
    rpi, nimg, F = 300, 128, 544
    y, ref, gref = case(nimg * rpi, F, act)
    g = None if groups == "none" else [i % 2 for i in range(nimg)]
    ng = 1 if g is None else 2
    out, cz, cn, tt = run(y, ACTS[act], rpi=rpi, groups=g, ngroups=ng)
    wz, wn, wt = want_counts(gref, rpi, g, ng)
    assert torch.equal(cz.long(), wz) and torch.equal(cn.long(), wn) and torch.equal(tt, wt)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_totals_only_and_arrays_only(act):
    rpi, nimg, F = 100, 4, 1280
    y, _, gref = case(nimg * rpi, F, act)
    wz, wn, wt = want_counts(gref, rpi, GROUPS["0101"], 2)
    _, cz, cn, tt = run(y, ACTS[act], rpi=rpi, groups=GROUPS["0101"], ngroups=2, arrays=False)
    assert cz is None and cn is None and torch.equal(tt, wt)
    _, cz, cn, tt = run(y, ACTS[act], rpi=rpi, groups=GROUPS["0101"], ngroups=2, totals=False)
    assert tt is None and torch.equal(cz.long(), wz) and torch.equal(cn.long(), wn)
    with pytest.raises(ValueError):
        ops.geglu_sparsity(y, ACTS[act], col_zero=cz)  # neither totals nor both arrays


def test_special_values():
    """ACT_NONE: the gate columns hold +0, -0, the smallest subnormals of either sign, +-65504 and +-inf (column n
    holds value n % 8 on every row)."""
    M, F = 64, 32
    bits = [0x0000, 0x8000, 0x0001, 0x8001, 0x7bff, 0xfbff, 0x7c00, 0xfc00]
    vals = torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(torch.float16)
    assert vals[2].item() == 2.0 ** -24 and vals[4].item() == 65504.0 and torch.isinf(vals[6:]).all()
    y = torch.ones((M, 2 * F), dtype=torch.float16)
    y[:, F:] = vals.repeat(F // 8)[None, :]
    y = y.to(DEV)
    kind = torch.arange(F) % 8
    for thr, zero_kinds in ((0.0, [0, 1]), (2.0 ** -14, [0, 1, 2, 3])):
        gate = torch.empty((M, F), dtype=torch.float16, device=DEV)
        _, cz, cn, tt = run(y, ops.ACT_NONE, threshold=thr, gate_out=gate)
        assert torch.equal(gate.view(torch.int16), y[:, F:].view(torch.int16))
        want_zero = torch.isin(kind, torch.tensor(zero_kinds)).long() * M
        want_neg = torch.isin(kind, torch.tensor([3, 5, 7])).long() * M   # -0 (kind 1) is not negative
        assert torch.equal(cz[0].long().cpu(), want_zero) and torch.equal(cn[0].long().cpu(), want_neg)
        assert tt.cpu().tolist() == [[int(want_zero.sum()), int(want_neg.sum())]]


@pytest.mark.parametrize("thr", [0.0, 0.05, 0.17])
def test_threshold(thr):
    rpi, nimg, F = 100, 4, 1280
    y, _, gref = case(nimg * rpi, F, "gelu")
    _, cz, cn, tt = run(y, ops.ACT_GELU, rpi=rpi, groups=GROUPS["0101"], ngroups=2, threshold=thr)
    want = (gref.float().abs() <= torch.tensor(thr, dtype=torch.float32, device=DEV)).view(nimg, rpi, F)
    want = torch.stack([want[[0, 2]].sum((0, 1)), want[[1, 3]].sum((0, 1))])
    assert torch.equal(cz.long(), want) and torch.equal(tt[:, 0], want.sum(1))
    assert torch.equal(cn.long(), want_counts(gref, rpi, GROUPS["0101"], 2)[1])  # the threshold leaves these alone
    if thr > 0:
        assert int(want.sum()) > int((gref == 0).sum())


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_guarded_outputs(act):
    """out, col_zero, col_neg and totals are views inside poisoned buffers (ldo > F), the count buffers pre-filled with
    garbage: exact results, nothing outside the views changes, and a second call into the same buffers gives the same
    results (nothing accumulates across calls)."""
    M, F, rpi, poison, ipoison = 200, 320, 100, 777.0, 123456789
    y, ref, gref = case(M, F, act)
    obuf = torch.full((M + 2, F + 16), poison, dtype=torch.float16, device=DEV)
    zbuf = torch.full((4, F), ipoison, dtype=torch.int32, device=DEV)
    nbuf = torch.full((4, F), ipoison, dtype=torch.int32, device=DEV)
    tbuf = torch.full((4, 2), ipoison, dtype=torch.int64, device=DEV)
    out, cz, cn, tt = obuf[1:M + 1, 8:8 + F], zbuf[1:3], nbuf[1:3], tbuf[1:3]
    table = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    wz, wn, wt = want_counts(gref, rpi, [1, 0], 2)
    for _ in range(2):
        ops.geglu_sparsity(y, ACTS[act], rows_per_img=rpi, img_group=table, ngroups=2, col_zero=cz, col_neg=cn,
                           totals=tt, out=out)
        assert torch.equal(cz.long(), wz) and torch.equal(cn.long(), wn) and torch.equal(tt, wt)
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    for buf, view, p in ((obuf, out, poison), (zbuf, cz, ipoison), (nbuf, cn, ipoison), (tbuf, tt, ipoison)):
        assert bool((view != p).any())
        view.fill_(p)
        assert bool((buf == p).all())


def test_argument_errors_raise():
    tt = torch.empty((1, 2), dtype=torch.int64, device=DEV)
    y = torch.zeros((64, 656), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.geglu_sparsity(y, ops.ACT_RELU, totals=tt)                                   # F = 328
    y = torch.zeros((100, 640), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="pointer/size"):
        ops.geglu_sparsity(y, ops.ACT_RELU, rows_per_img=64, totals=tt)                  # M % rows_per_img
    y = torch.zeros((128, 640), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="pointer/size"):
        ops.geglu_sparsity(y, ops.ACT_RELU, rows_per_img=64, totals=tt, threshold=-0.1)  # negative threshold
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.geglu_sparsity(y, ops.ACT_RELU, rows_per_img=64, totals=tt,
                           workspace=torch.empty(16, dtype=torch.float32, device=DEV))
    ops.geglu_sparsity(y, ops.ACT_RELU, rows_per_img=64, totals=tt)       # the shared workspace is large enough
    assert tt.cpu().tolist() == [[128 * 320, 0]]


# ------------------------------------------------------------------------------------------------ receivers
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_receiver_counts_equal_sums_over_the_devices_own_projection(act):
    """4 images, 2 prompts: group p counts images p and p + 2 of the device's own activated gate (the existing
    kernel's gate_out over the same proj.run(x)): exact."""
    from neuron_receivers import SparsityMeasure
    from sdmoe._lib import SdmoeError
    _, c = [nc for nc in SPARSITY if str(nc[1]["act"]) == act and float(nc[1]["gate_bias"]) == 0.0][0]
    m = device_module(c, 0)
    x = R.tokens(c, 0, 0, 0, nimg=4).to(DEV)
    rec = SparsityMeasure(0, per_neuron=True, store_gates=False)
    rec.set_prompts(["one", "two"])
    out = rec.hook_fn(m, (x,), None)
    assert rec.calls == [] and rec.gates == []
    rec.flush()
    y = m.proj.run(x.reshape(-1, x.shape[-1]))
    gate = torch.empty((y.shape[0], m.inner_dim), dtype=torch.float16, device=DEV)
    dense = ops.geglu_route(y, None, ACTS[act], gate_out=gate)
    wz, wn, wt = R.group_counts(gate.view(4, -1, m.inner_dim), [0, 1, 0, 1], 2)
    (call,) = rec.calls
    assert call["zeros"].tolist() == wt[:, 0].tolist() and call["negatives"].tolist() == wt[:, 1].tolist()
    assert call["elements"].tolist() == [2 * x.shape[1] * m.inner_dim] * 2 and call["rows"].tolist() == [2 * x.shape[1]] * 2
    assert call["neuron_zeros"].dtype == np.int32 and np.array_equal(call["neuron_zeros"], wz.cpu().numpy())
    assert torch.equal(out.reshape(dense.shape).view(torch.int16), dense.view(torch.int16))
    assert rec.flush_count == 1
    rec.set_prompts(["one", "two", "three"])
    with pytest.raises(SdmoeError):
        rec.hook_fn(m, (x,), None)


@pytest.mark.parametrize("name,c", SPARSITY, ids=[n for n, _ in SPARSITY])
def test_receiver_vs_golden(name, c):
    """The device GEMM may move a pre-activation gate g of the CPU restatement by up to tol, so every count lies
    between the number of elements that are counted wherever in [g - tol, g + tol] the device's gate falls and the
    number that can be counted somewhere in it.
    relu: act(g') == 0 iff g' <= 0, so zeros lie in [#(g <= -tol), #(g <= tol)], and no element is negative.
    gelu: act(g') < 0 on one interval of g' (below it the fp16 GELU flushes to -0, which is a zero and not a negative:
    the gate-bias -3.0 fixture has hundreds of those per call), so an element is surely negative when both ends of its
    bracket are, and possibly negative when g - tol < 0 and g + tol is not in the flushed tail; surely zero when
    g + tol is in the flushed tail, possibly zero when g - tol is, or when the bracket holds 0."""
    from neuron_receivers import SparsityMeasure
    T, L, P, act = int(c["T"]), int(c["L"]), int(c["P"]), str(c["act"])
    mods = [device_module(c, l) for l in range(L)]
    ws = [R.weights(c, l) for l in range(L)]
    rec = SparsityMeasure(0, store_gates=False)
    for p in range(P):
        rec.calls = []
        for call in range(T * L):
            out = rec.hook_fn(mods[call % L], (R.tokens(c, p, 0, call).to(DEV),), None)
            if (p, call) == (0, 0):
                assert out.shape == c["out0"].shape and close(out.cpu().numpy(), c["out0"])
        rec.flush()
        assert len(rec.calls) == T * L
        for call in range(T * L):
            _, _, g = R.hook(R.tokens(c, p, 0, call), *ws[call % L], act)
            g = g.float()
            tol = 1e-2 * max(1.0, g.abs().max().item())
            zeros, negs = int(rec.calls[call]["zeros"][0]), int(rec.calls[call]["negatives"][0])
            assert int(rec.calls[call]["elements"][0]) == int(c["elements"])
            print(f"{name} p={p} call={call}: zeros {zeros} (reference {int(c['zeros'][p, call])}), "
                  f"negatives {negs} (reference {int(c['negatives'][p, call])}), tol {tol:.4f}")
            if act == "relu":
                assert int((g <= -tol).sum()) <= zeros <= int((g <= tol).sum())
                assert negs == 0
            else:
                lo, hi = (g - tol).half(), (g + tol).half()
                alo, ahi = mods[0].gelu(lo.to(DEV)).float().cpu(), mods[0].gelu(hi.to(DEV)).float().cpu()
                lo, hi = lo.float(), hi.float()
                sure_neg = (alo < 0) & (ahi < 0)
                may_neg = (lo < 0) & ((ahi < 0) | (hi >= 0))
                assert int(sure_neg.sum()) <= negs <= int(may_neg.sum())
                sure_zero = (ahi == 0) & (hi < -1)
                may_zero = ((alo == 0) & (lo < -1)) | ((lo <= 0) & (hi >= 0))
                assert int(sure_zero.sum()) <= zeros <= int(may_zero.sum())
                assert 0 < int(sure_neg.sum())
    assert rec.flush_count == P


def test_through_the_pipeline(tmp_path):
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    from sdmoe.unet import GEGLU, UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    from sparsity.relufy_model import find_and_change_geglu
    from neuron_receivers import NeuronPredictivity, SparsityMeasure
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 3), cfg, DEV)
    steps, L = 2, 16
    pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=steps)
    prompt = "a photo of a dog"
    geglus = [m for n, m in unet.named_modules() if isinstance(m, GEGLU) and "ff.net" in n]
    assert len(geglus) == L
    want, _ = NeuronPredictivity(0, steps, L).observe_activation(pipe, prompt)
    # stored gates (the base default): the reference driver's list, and the counts it would take from it
    rec = SparsityMeasure(0)
    out, gates = rec.observe_activation(pipe, prompt)
    assert torch.equal(out, want)  # the same projection and the same dense product
    assert len(rec.calls) == steps * L and rec.flush_count == 1 and len(gates) == steps * L
    for i, (gate, call) in enumerate(zip(gates, rec.calls)):
        assert not gate.is_cuda and gate.dtype == torch.float16 and gate.shape[-1] == geglus[i % L].inner_dim
        assert call["zeros"].shape == (1,) and int((gate == 0).sum()) == int(call["zeros"][0])
        assert int((gate < 0).sum()) == int(call["negatives"][0]) and gate.numel() == int(call["elements"][0])
    with pytest.raises(AssertionError, match="Relu failed"):
        rec.test(pipe)  # the GELU model
    # counts only, a prompt list: one group per prompt
    rec = SparsityMeasure(0, per_neuron=True, store_gates=False)
    _, gates = rec.observe_activation(pipe, [prompt, "a church"])
    assert gates == [] and len(rec.calls) == steps * L and rec.flush_count == 1
    for i, call in enumerate(rec.calls):
        Fn = geglus[i % L].inner_dim
        assert call["zeros"].shape == (2,) and call["neuron_zeros"].shape == (2, Fn)
        assert call["neuron_zeros"].sum(1).tolist() == call["zeros"].tolist()
    frac = discovery.neuron_zero_fraction(rec.calls, L)
    assert frac[1][15].shape == (2, geglus[15].inner_dim) and 0.0 <= frac[1][15].min() <= frac[1][15].max() <= 1.0
    # the relufied model
    find_and_change_geglu(pipe.unet)
    rec = SparsityMeasure(0, store_gates=False)
    rec.test(pipe)
    assert len(rec.calls) == steps * L and rec.gates == [] and rec.store_gates is False
    for call in rec.calls:
        assert int(call["negatives"][0]) == 0 and 0 < int(call["zeros"][0]) < int(call["elements"][0])
    rec.observe_activation(pipe, prompt)
    assert rec.flush_count == 2 and len(rec.calls) == steps * L
    ratios = discovery.sparsity_ratios(rec.calls)
    assert ratios.shape == (steps * L, 1) and 0.0 < ratios.min() and ratios.max() < 1.0
    meter = discovery.accumulate_sparsity(discovery.StatMeter(steps, L), ratios, L)
    meter.save(str(tmp_path / "sparsity.json"))
    with open(tmp_path / "sparsity.json") as f:
        saved = json.load(f)["time_steps"]
    assert len(saved) == steps and all(len(saved[str(t)]) == L for t in range(steps))
    assert saved["1"]["15"]["avg"] == ratios[31, 0]


def test_feedforward_takes_plain_down_projection_and_fused_path_returns():
    """Under a SparsityMeasure hook the GEGLU product is in the natural neuron order and FeedForward runs its ordinary
    down projection; once the hook is removed, a MOEFy run over the same module takes the fused routed path again."""
    from moefication.helper import modify_ffn
    from neuron_receivers import MOEFy, SparsityMeasure
    from sdmoe.unet import FeedForward, LoRACompatibleLinear
    _, c = [nc for nc in SPARSITY if str(nc[1]["act"]) == "gelu" and float(nc[1]["gate_bias"]) == 0.0][0]
    C, Fn = 320, 1280
    geglu = device_module(c, 0)
    wd, bd = R.synth.down_weights(C, 11)
    ff = FeedForward(geglu, LoRACompatibleLinear(torch.from_numpy(wd).half().to(DEV), torch.from_numpy(bd).half().to(DEV)))
    modify_ffn(geglu, None, 0.2, labels=R.synth.balanced_labels(Fn, Fn // 20, 3))
    x = R.tokens(c, 0, 0, 0).to(DEV)
    x2d = x.reshape(-1, C)
    residual = torch.zeros_like(x2d)
    rec = SparsityMeasure(0, store_gates=False)
    hook = rec._register(geglu, rec.hook_fn)
    y = ff.run(x2d, 2, residual)
    assert geglu._out_perm is None and geglu._out_keep is None and len(rec._pending) == 1
    rec.remove_hooks([hook])
    rec.flush()
    want, _ = geglu.neurons(x)
    assert torch.equal(y, ff.net[2].run(want.reshape(-1, Fn), residual=residual))
    assert int(rec.calls[0]["negatives"][0]) > 0
    mo = MOEFy(seed=0, store_gates=False)
    hook = mo._register(geglu, mo.hook_fn)
    routed = ff.run(x2d, 2, residual)
    mo.remove_hooks([hook])
    assert geglu._out_perm is not None and torch.isfinite(routed).all() and not torch.equal(routed, y)
