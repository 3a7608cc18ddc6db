"""The expert-level discovery path on the MI355X: sdmoe_expert_stats and the ExpertPredictivity / FrequencyMeasure
receivers.

Kernel tests take a synthetic score matrix and synthetic top-k bit words, so no GEMM rounding enters and every statement
is exact: the column maximum as numbers (-0 == +0) with torch.amax over the same rows, the selection counts with the
column sums of the unpacked bits per image.
Receiver tests start from x, so the device GEMM's fp32 summation order enters: outputs, maxima and saved statistics
within the project's fp16-GEMM bar 1e-2 * max(1, |ref|.max()) (tests/test_gpu_neurons.py) of the reference's fixtures
(tests/golden/expert_*.npz). A selection histogram can differ from the reference's only on near-tie rows -- rows whose
k-th / (k+1)-th score gap is within 8 fp16 ulps, test_gpu_route_parity.near_tie_rows -- where one expert may swap for
another: sum_e |dev - ref| <= 2 * n_near / seq_len per (t, l), with n_near the fixture's recorded count (0 for most
calls: the comparison is then exact), capped at 5 % of the rows by the fixture generator and re-asserted here.
Against the device's own scores and selection bits (GEGLU.scored / GEGLU.routed on the same module and x) the receivers
are exact.
"""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import expert_ref as R  # noqa: E402
from sdmoe import _lib, discovery, ops  # noqa: E402

DEV = "cuda"
ACTS = {"gelu": ops.ACT_GELU, "relu": ops.ACT_RELU}
ROWS = [(64, 4), (100, 4), (1024, 4), (64, 2), (100, 2), (1024, 2)]  # (rows per image, images)


def grouping(nimg):
    """2 images: img_group None (one group); 4 or 32 images: image i in group i % 2."""
    if nimg == 2:
        return [0, 0], 1, None
    groups = [i % 2 for i in range(nimg)]
    return groups, 2, torch.tensor(groups, dtype=torch.int32, device=DEV)


def row_cases(Es):
    """ROWS at every E (ids as a stacked parametrize gives them), then 32 images of 300 rows at E = 256: 32 x 2 x 4 =
    256 blocks, the least that takes 256-row slabs, with a 44-row second slab. ROWS reaches the 16-row slabs, and the
    64-row ones only at (1024, 4) with E = 256."""
    return [pytest.param(rpi, nimg, E, id=f"{rpi}-{nimg}-{E}") for E in Es for rpi, nimg in ROWS + [(300, 32)]
            if rpi != 300 or E == 256]


# ------------------------------------------------------------------------------------------------ kernel
@functools.lru_cache(maxsize=None)
def score_case(M, E):
    """A strided [M, E] view (ld_score = E + 24) of a poisoned buffer; every 7th column is negative on every row."""
    g = torch.Generator().manual_seed(M * 11 + E)
    s = torch.randn(M, E, generator=g) * 3.0
    s[:, ::7] = -s[:, ::7].abs() - 0.125
    buf = torch.full((M, E + 24), 900.0, dtype=torch.float16, device=DEV)
    buf[:, 8:8 + E] = s.half().to(DEV)
    return buf[:, 8:8 + E]


@functools.lru_cache(maxsize=None)
def sel_case(M, E):
    """(int32 device words [M, ceil(E / 32)], bool numpy [M, E]): exactly k = max(1, E // 5) bits per row, plus random
    bits at or above E in the last word when E % 32 != 0."""
    rng = np.random.default_rng(M * 13 + E)
    k = max(1, E // 5)
    on = np.zeros((M, E), dtype=bool)
    np.put_along_axis(on, np.argsort(rng.random((M, E)), axis=1)[:, :k], True, axis=1)
    words = R.pack_sel(on).view(np.uint32).copy()
    if E % 32:
        garbage = rng.integers(0, 1 << 32, M, dtype=np.uint64).astype(np.uint32) & ~np.uint32((1 << (E % 32)) - 1)
        assert garbage.any()
        words[:, -1] |= garbage
    return torch.from_numpy(words.view(np.int32)).to(DEV), on


def group_amax(score, rpi, groups, ngroups):
    s3 = score.reshape(-1, rpi, score.shape[1])
    return torch.stack([torch.amax(s3[[i for i, gi in enumerate(groups) if gi == g]].reshape(-1, score.shape[1]), 0)
                        for g in range(ngroups)])


@pytest.mark.parametrize("rpi,nimg,E", row_cases([64, 256, 40]))
def test_column_maximum(rpi, nimg, E):
    """rpi = 100 leaves a partial slab, 1024 gives several slabs per image; the always-negative columns fail a
    zero-initialised maximum. (300, 32) at E = 256 runs 256-row slabs (row_cases), the 32 images in two groups."""
    score = score_case(nimg * rpi, E)
    assert score.stride(0) > E
    groups, ng, table = grouping(nimg)
    colmax = torch.full((ng, E), 7.0, dtype=torch.float16, device=DEV)
    ops.expert_stats(score, rows_per_img=rpi, img_group=table, ngroups=ng, colmax=colmax)
    assert torch.equal(colmax, group_amax(score, rpi, groups, ng))  # equality as numbers
    assert bool((colmax[:, ::7] < 0).all())


@pytest.mark.parametrize("rpi,nimg,E", row_cases([64, 40, 100, 256]))
def test_selection_counts(rpi, nimg, E):
    """(300, 32) at E = 256 runs 256-row slabs (row_cases): the counts of a 256-row and of a 44-row slab per image."""
    M = nimg * rpi
    sel, on = sel_case(M, E)
    count = torch.full((nimg, E), -1, dtype=torch.int32, device=DEV)
    ops.expert_stats(score_case(M, E), sel=sel, rows_per_img=rpi, count=count)
    want = on.reshape(nimg, rpi, E).sum(1)
    assert np.array_equal(count.cpu().numpy(), want)
    assert (want.sum(1) == rpi * max(1, E // 5)).all()


def test_both_statistics_in_one_call():
    rpi, nimg, E = 100, 4, 100
    score = score_case(nimg * rpi, E)
    sel, on = sel_case(nimg * rpi, E)
    groups, ng, table = grouping(nimg)
    colmax = torch.full((ng, E), 7.0, dtype=torch.float16, device=DEV)
    count = torch.full((nimg, E), -1, dtype=torch.int32, device=DEV)
    got = ops.expert_stats(score, sel=sel, rows_per_img=rpi, img_group=table, ngroups=ng, colmax=colmax, count=count)
    assert got[0] is colmax and got[1] is count
    assert torch.equal(colmax, group_amax(score, rpi, groups, ng))
    assert np.array_equal(count.cpu().numpy(), on.reshape(nimg, rpi, E).sum(1))
    # rows_per_img = 0: one image of M rows
    one = torch.full((1, E), -1, dtype=torch.int32, device=DEV)
    cm = torch.empty((1, E), dtype=torch.float16, device=DEV)
    ops.expert_stats(score, sel=sel, colmax=cm, count=one)
    assert np.array_equal(one.cpu().numpy()[0], on.sum(0)) and torch.equal(cm[0], torch.amax(score, 0))


def test_guarded_outputs():
    """colmax and count are carved out of larger poisoned buffers: nothing outside them changes."""
    rpi, nimg, E = 100, 4, 40
    score = score_case(nimg * rpi, E)
    sel, on = sel_case(nimg * rpi, E)
    groups, ng, table = grouping(nimg)
    cbuf = torch.full((ng + 2, E), 777.0, dtype=torch.float16, device=DEV)
    nbuf = torch.full((nimg + 2, E), -12345, dtype=torch.int32, device=DEV)
    colmax, count = cbuf[1:1 + ng], nbuf[1:1 + nimg]
    ops.expert_stats(score, sel=sel, rows_per_img=rpi, img_group=table, ngroups=ng, colmax=colmax, count=count)
    assert torch.equal(colmax, group_amax(score, rpi, groups, ng))
    assert np.array_equal(count.cpu().numpy(), on.reshape(nimg, rpi, E).sum(1))
    assert bool((colmax != 777.0).all()) and bool((count != -12345).all())
    colmax.fill_(777.0)
    count.fill_(-12345)
    assert bool((cbuf == 777.0).all()) and bool((nbuf == -12345).all())
    # the score view's own buffer (the columns around the view) is read-only to the kernel
    base = score._base if score._base is not None else score
    assert bool((base[:, :8] == 900.0).all()) and bool((base[:, 8 + E:] == 900.0).all())


def test_argument_errors_raise():
    E, rpi, nimg = 64, 64, 2
    M = rpi * nimg
    score = score_case(M, E)
    sel, on = sel_case(M, E)
    count = torch.full((nimg, E), -1, dtype=torch.int32, device=DEV)
    colmax = torch.full((1, E), 7.0, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="pointer/size"):
        ops.expert_stats(score, rows_per_img=rpi, count=count)                       # count without sel
    with pytest.raises(_lib.SdmoeError, match="pointer/size"):
        ops.expert_stats(score, sel=sel, rows_per_img=48, colmax=colmax)             # M % rows_per_img
    assert bool((count == -1).all()) and bool((colmax == 7.0).all())
    # M == 0: nothing is launched, nothing is written
    ops.expert_stats(score[:0], sel=sel[:0], colmax=colmax, count=torch.empty((0, E), dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((colmax == 7.0).all())
    wide = torch.zeros((M, 257), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.expert_stats(wide, rows_per_img=rpi, colmax=torch.empty((1, 257), dtype=torch.float16, device=DEV))
    # the documented workspace bound, c = images * ceil(rows_per_img / 16) * E cells: c floats for the counts plus
    # ceil(c / 2) for the fp16 maxima -- exactly enough passes, one float less is refused
    cells = nimg * -(-rpi // 16) * E
    need = cells + (cells + 1) // 2
    with pytest.raises(_lib.SdmoeError, match="shape"):
        ops.expert_stats(score, sel=sel, rows_per_img=rpi, colmax=colmax, count=count,
                         workspace=torch.empty(need - 1, dtype=torch.float32, device=DEV))
    assert bool((count == -1).all()) and bool((colmax == 7.0).all())
    ops.expert_stats(score, sel=sel, rows_per_img=rpi, colmax=colmax, count=count,
                     workspace=torch.empty(need, dtype=torch.float32, device=DEV))
    assert torch.equal(colmax[0], torch.amax(score, 0))
    assert np.array_equal(count.cpu().numpy(), on.reshape(nimg, rpi, E).sum(1))
    with pytest.raises(_lib.SdmoeError, match="shape"):                              # the maxima alone: ceil(c / 2)
        ops.expert_stats(score, rows_per_img=rpi, colmax=colmax,
                         workspace=torch.empty((cells + 1) // 2 - 1, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_chained_with_the_routing_kernel(act):
    M, F, E, k, rpi = 512, 1280, 64, 12, 256
    g = torch.Generator().manual_seed(77)
    y = (torch.randn(M, 2 * F, generator=g) * 1.5).half().to(DEV)
    routing = ops.Routing(torch.from_numpy(R.synth.balanced_labels(F, E, 9)), E, k, DEV)
    sel = torch.zeros((M, E // 32), dtype=torch.int32, device=DEV)
    score = torch.empty((M, E), dtype=torch.float16, device=DEV)
    ops.geglu_route(y, routing, ACTS[act], sel_out=sel, score_out=score)
    colmax = torch.empty((2, E), dtype=torch.float16, device=DEV)
    count = torch.empty((2, E), dtype=torch.int32, device=DEV)
    table = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    ops.expert_stats(score, sel=sel, rows_per_img=rpi, img_group=table, ngroups=2, colmax=colmax, count=count)
    on = R.unpack_sel(sel.cpu().numpy(), E)
    assert (on.sum(1) == k).all()
    assert np.array_equal(count.cpu().numpy(), on.reshape(2, rpi, E).sum(1))
    assert torch.equal(colmax, group_amax(score, rpi, [1, 0], 2))


# ------------------------------------------------------------------------------------------------ receivers
def device_module(c, l):
    from moefication.helper import modify_ffn
    from sdmoe.unet import GEGLU, LoRACompatibleLinear, _gelu
    w, b = R.weights(c, l)
    m = GEGLU(LoRACompatibleLinear(w.to(DEV), b.to(DEV)))
    m.gelu = torch.nn.functional.relu if str(c["act"]) == "relu" else _gelu
    modify_ffn(m, None, float(c["topk"]), labels=c["labels"])
    return m


def bar(ref):
    return 1e-2 * max(1.0, float(np.abs(np.asarray(ref, dtype=np.float32)).max()))


def close(got, ref):
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    return got.shape == ref.shape and float(np.abs(got - ref).max()) <= bar(ref)


PRED = R.golden("expert_pred")
FREQ = R.golden("expert_freq")


@pytest.mark.parametrize("name,c", PRED, ids=[n for n, _ in PRED])
def test_expert_predictivity_vs_golden(name, c, tmp_path):
    from neuron_receivers import ExpertPredictivity
    T, L, P, E = int(c["T"]), int(c["L"]), int(c["P"]), int(c["E"])
    mods = [device_module(c, l) for l in range(L)]
    assert int(mods[0].k) == int(E * float(c["topk"]))
    rec = ExpertPredictivity(0, T, L)
    for p in range(P):
        rec.reset_time_layer()
        for call in range(T * L):
            out = rec.hook_fn(mods[call % L], (R.pred_tokens(c, p, 0, call).to(DEV),), None)
            if (p, call) == (0, 0):
                assert close(out.cpu().numpy(), c["out0"])
        rec.flush()
        assert (rec.timestep, rec.layer) == (T, 0) and rec.flush_count == p + 1
        for t in range(T):
            for l in range(L):
                got = rec.max_gate[t][l]
                assert got.dtype == np.float16 and got.shape == (E,)
                assert close(got, c["max_gate_base"][p, t, l]), (p, t, l)
    if float(c["gate_bias"]) < 0:
        assert (rec.max_gate[0][0] < 0).any()
    rec.predictivity.save(str(tmp_path / "predictivity_base_expert.json"))
    with open(tmp_path / "predictivity_base_expert.json") as f:
        saved = json.load(f)
    ref = json.loads(c["json_base"].tobytes())
    assert list(saved) == list(ref) and list(saved["time_steps"]) == list(ref["time_steps"])
    for t in ref["time_steps"]:
        assert list(saved["time_steps"][t]) == list(ref["time_steps"][t])
        for l, cell in ref["time_steps"][t].items():
            assert list(saved["time_steps"][t][l]) == list(cell)
            for key in cell:
                assert close(saved["time_steps"][t][l][key], cell[key]), (t, l, key)


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_expert_predictivity_equals_scored(act):
    """Against the device's own scores: the output is GEGLU.scored's bit for bit, max_gate the amax of its scores."""
    from neuron_receivers import ExpertPredictivity
    _, c = [pc for pc in PRED if str(pc[1]["act"]) == act and float(pc[1]["gate_bias"]) == 0.0][0]
    m, x = device_module(c, 0), R.pred_tokens(c, 0, 0, 0).to(DEV)
    rec = ExpertPredictivity(0, 1, 1)
    out = rec.hook_fn(m, (x,), None)
    rec.flush()
    want, score = m.scored(x)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert np.array_equal(rec.max_gate[0][0], torch.amax(score, 0).cpu().numpy())
    # without patterns: dense output, no statistic, the counter still advances
    m.patterns = None
    rec = ExpertPredictivity(0, 1, 2)
    out = rec.hook_fn(m, (x,), None)
    rec.flush()
    assert torch.equal(out, m.dense(x)) and rec.max_gate[0][0] == [] and (rec.timestep, rec.layer) == (0, 1)
    assert rec.flush_count == 0


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_frequency_measure_output_equals_moefy(act):
    from neuron_receivers import FrequencyMeasure, MOEFy
    _, c = [fc for fc in FREQ if str(fc[1]["act"]) == act and int(fc[1]["C"]) == 320][0]
    m, x = device_module(c, 0), R.tokens(c, c["x_seeds"][0]).to(DEV)
    E = int(c["E"])
    rec = FrequencyMeasure(0, 1, 1, {"ffn": E}, ["ffn"])
    out = rec.hook_fn(m, (x,), None)
    want = MOEFy(seed=0, store_gates=False).hook_fn(m, (x,), None)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)) and rec.gates == []
    m.patterns = None
    dense = rec.hook_fn(m, (x,), None)
    assert torch.equal(dense, m.dense(x)) and (rec.timestep, rec.layer) == (2, 0)


@pytest.mark.parametrize("name,c", FREQ, ids=[n for n, _ in FREQ])
def test_frequency_measure_vs_golden(name, c):
    """Selection histograms against the reference's. Measured on the MI355X: every fixture exact (sum_e |dev - ref| = 0
    at every (t, l)), relu and gelu alike; the bound below allows one swapped expert per recorded near-tie row."""
    from neuron_receivers import FrequencyMeasure
    from test_gpu_route_parity import near_tie_rows
    T, L, E, k, N = int(c["T"]), int(c["L"]), int(c["E"]), int(c["k"]), int(c["N"])
    # the cap the fixture generator searched its token seeds for, re-derived from the stored reference scores
    for call in range(len(c["x_seeds"])):
        n_near = int(near_tie_rows(c["score0"][call], k, slack_ulps=8).sum())
        assert n_near == int(c["n_near"][call]) and n_near <= 0.05 * N, (call, n_near)
    mods = [device_module(c, l) for l in range(L)]
    names = [f"ffn{l}" for l in range(L)]
    rec = FrequencyMeasure(0, T, L, {n: E for n in names}, names)
    allowed = np.zeros((T, L))
    for call, (t, l) in enumerate(c["call_tl"].tolist()):
        if call == T * L:
            rec.flush()
            assert (rec.timestep, rec.layer) == (T, 0)
            rec.reset_time_layer()  # the counters keep what they hold
        assert (rec.timestep, rec.layer) == (t, l)
        out = rec.hook_fn(mods[l], (R.tokens(c, c["x_seeds"][call]).to(DEV),), None)
        allowed[t, l] += 2.0 * int(c["n_near"][call]) / N
        if call == 0:
            keep = ~near_tie_rows(c["score0"][0], k, slack_ulps=8)
            assert close(out[0].cpu().numpy()[keep], c["out0"][0][keep])
    rec.flush()
    for t in range(T):
        for l in range(L):
            got = rec.label_counter[t][l]
            assert got.dtype == np.float64 and got.shape == (E,)
            dist = float(np.abs(got - c["label_counter"][t, l]).sum())
            print(f"{name} (t, l) = ({t}, {l}): sum |dev - ref| = {dist} (allowed {allowed[t, l]}), "
                  f"near-tie rows {c['n_near'].tolist()}")
            assert dist <= allowed[t, l], (t, l, dist, allowed[t, l])
            assert abs(got.sum() - c["label_counter"][t, l].sum()) == 0.0  # k per token, exactly (a power-of-two N)
    rec.reset()
    assert all(not rec.label_counter[t][l].any() for t in range(T) for l in range(L))


def test_frequency_measure_sequence_length_100():
    """A seq_len that is no power of two: count * (1 / 100) against the reference's 100 additions of 1 / 100 per
    selected expert over the device's own selection bits; rtol 1e-12 (n <= 4096 float64 additions x 2^-53, rounded up)."""
    from neuron_receivers import FrequencyMeasure
    _, c = [fc for fc in FREQ if int(fc[1]["C"]) == 320 and str(fc[1]["act"]) == "gelu"][0]
    m, E, k = device_module(c, 0), int(c["E"]), int(c["k"])
    x = torch.from_numpy(R.synth.tokens((2, 100, 320), 4242)).half().to(DEV)
    rec = FrequencyMeasure(0, 1, 1, {"ffn": E}, ["ffn"])
    rec.hook_fn(m, (x,), None)
    rec.flush()
    sel = torch.zeros((200, (E + 31) // 32), dtype=torch.int32, device=DEV)
    m.routed(x, sel_out=sel)
    on = R.unpack_sel(sel.cpu().numpy(), E)
    assert (on.sum(1) == k).all()
    ref = np.zeros(E)
    for row in on[:100]:
        ref[np.flatnonzero(row)] += (1.0 / 100)
    np.testing.assert_allclose(rec.label_counter[0][0], ref, rtol=1e-12, atol=0)
    assert abs(rec.label_counter[0][0].sum() - k) <= 1e-9


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_prompt_list_groups_images_by_prompt(act):
    """4 images, 2 prompts under guidance ([uncond x 2 ; cond x 2]): exact against the device's own scores and bits."""
    from neuron_receivers import ExpertPredictivity, FrequencyMeasure
    from sdmoe._lib import SdmoeError
    _, c = [pc for pc in PRED if str(pc[1]["act"]) == act and float(pc[1]["gate_bias"]) == 0.0][0]
    m, E, N = device_module(c, 0), int(c["E"]), int(c["N"])
    x = R.pred_tokens(c, 0, 0, 0, nimg=4).to(DEV)
    rec = ExpertPredictivity(0, 1, 1)
    rec.set_prompts(["one", "two"])
    rec.hook_fn(m, (x,), None)
    rec.flush()
    _, score = m.scored(x)
    want = R.group_max(score.cpu().view(4, N, E), [0, 1, 0, 1], 2)
    got = rec.max_gate[0][0]
    assert got.shape == (2, E) and np.array_equal(got, want.numpy())
    assert rec.predictivity.results["time_steps"][0][0]["std"].n == 2
    sel = torch.zeros((4 * N, (E + 31) // 32), dtype=torch.int32, device=DEV)
    m.routed(x, sel_out=sel)
    per_image = R.unpack_sel(sel.cpu().numpy(), E).reshape(4, N, E).sum(1).astype(np.float64)
    for mode, want in (("first", per_image[:2] * (1.0 / N)), ("all", (per_image[:2] + per_image[2:]) / (2 * N))):
        fm = FrequencyMeasure(0, 1, 1, {"ffn": E}, ["ffn"], images=mode)
        fm.set_prompts(["one", "two"])
        fm.hook_fn(m, (x,), None)
        fm.flush()
        assert fm.label_counter[0][0].shape == (2, E) and np.array_equal(fm.label_counter[0][0], want), mode
    for r in (rec, fm):
        with pytest.raises(SdmoeError):
            r.hook_fn(m, (x[:3],), None)


def test_through_the_pipeline(tmp_path):
    from moefication.helper import moefy_synthetic
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    from sdmoe.unet import GEGLU, UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    from neuron_receivers import ExpertPredictivity, FrequencyMeasure, RemoveExperts
    cfg = UNetConfig.tiny(16)
    unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 3), cfg, DEV)
    steps, L = 3, 16
    pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=steps)
    _, layer_names, nexp = moefy_synthetic(pipe, 0.25, 16, seed=1)
    geglus = [m for n, m in unet.named_modules() if isinstance(m, GEGLU) and "ff.net" in n]
    assert len(geglus) == L
    pairs = [("a photo of a dog", "a photo of a dog in the snow"), ("a church", "a church at night"),
             ("a bowl of fruit", "a bowl of rotten fruit")]
    base, adj = ExpertPredictivity(0, steps, L), ExpertPredictivity(0, steps, L)
    diff = {t: {l: discovery.StandardDev() for l in range(L)} for t in range(steps)}
    for i, (pb, pa) in enumerate(pairs):
        for rec, prompt in ((base, pb), (adj, pa)):
            rec.reset_time_layer()
            out, _ = rec.observe_activation(pipe, prompt)
            assert torch.isfinite(out).all()
            assert (rec.timestep, rec.layer) == (steps, 0) and rec.flush_count == i + 1
        for t in range(steps):
            for l in range(L):
                mg = base.max_gate[t][l]
                assert mg.dtype == np.float16 and mg.shape == (geglus[l].patterns.shape[0],) and np.isfinite(mg).all()
                diff[t][l].update(mg - adj.max_gate[t][l])
    dstd = {t: {l: diff[t][l].stddev().tolist() for l in range(L)} for t in range(steps)}
    base.predictivity.save(str(tmp_path / "predictivity_base_expert.json"))
    adj.predictivity.save(str(tmp_path / "predictivity_adj_expert.json"))
    with open(tmp_path / "diff_std_expert.json", "w") as f:
        json.dump(dstd, f)
    for critical in (3.579, 2.92, 1.886, 1.0, 0.5, 0.0):
        lists = discovery.expert_lists_from_statistics(str(tmp_path / "predictivity_base_expert.json"),
                                                       str(tmp_path / "predictivity_adj_expert.json"),
                                                       str(tmp_path / "diff_std_expert.json"), len(pairs), critical)
        if any(lists[t][l] for t in range(steps) for l in range(L)):
            break
    assert any(lists[t][l] for t in range(steps) for l in range(L)), "no expert separates the prompt pairs"
    discovery.save_expert_lists(lists, str(tmp_path / "skilled"))
    rem = RemoveExperts(0, str(tmp_path / "skilled"), steps, L, store_gates=False)
    assert rem.expert_indices == lists
    removed, _ = rem.observe_activation(pipe, pairs[0][1])
    assert torch.isfinite(removed).all() and (rem.timestep, rem.layer) == (steps, 0)
    for mode in ("first", "all"):
        fm = FrequencyMeasure(0, steps, L, nexp, layer_names, images=mode)
        out, gates = fm.observe_activation(pipe, pairs[0][1])
        assert torch.isfinite(out).all() and gates == []
        assert (fm.timestep, fm.layer) == (steps, 0) and fm.flush_count == 1
        for t in range(steps):
            for l in range(L):
                row = fm.label_counter[t][l]
                assert row.dtype == np.float64 and row.shape == (geglus[l].patterns.shape[0],)
                assert abs(row.sum() - int(geglus[l].k)) <= 1e-9, (mode, t, l)
    counter = discovery.accumulate_expert_counter(None, fm.label_counter, layer_names, 1)
    path = discovery.save_expert_counter(counter, str(tmp_path), 0.25)
    with open(path) as f:
        saved = json.load(f)
    assert list(saved) == [str(t) for t in range(steps)] and sorted(saved["0"]) == sorted(layer_names)
