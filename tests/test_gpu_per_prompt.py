"""Per-prompt concept sets on the MI355X: sdmoe_wmask_union_sets, sdmoe_linear_masked_sets (every tile family the
U-Net's shapes take, the forced 64-row tile of the mid block, the per-run fallback under 8x8 latents), the
WandaRemovePerPrompt receiver on the reference's own mask fixture and through the pipeline (plain and routed FFN),
and MultiConceptRemoverWanda.remove_concepts_batch.

The kernel tests are bit-for-bit statements: rows of image i of a mixed call equal rows of image i of the same call
with every image on set s_i (a kernel that ignores the table, or indexes it by the wrong tile, fails), and a uniform
call equals sdmoe_linear_masked wherever the two launches split K alike (existing tests tie that one to
mask-then-plain GEMM). Tolerances elsewhere are the project's own: 1e-2 * max(1, |ref|.max()) against fp32
(tests/test_gpu_wanda.py), 2 fp16 ulps on the reference fixture, rel L2 <= 3e-2 between pipelines.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sdmoe import ops  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import synth  # noqa: E402

DEV = "cuda"


def packed(mask):
    return torch.from_numpy(np.packbits(np.asarray(mask).astype(np.uint8), axis=-1, bitorder="little")).to(DEV)


def keep_words(keepb):
    """bool [M, K] (neuron k of token m kept) -> sdmoe_moe_topk_keep's layout, int64 [K/64, M]."""
    M, K = keepb.shape
    w = np.packbits(keepb.reshape(M, K // 64, 64), axis=-1, bitorder="little").view(np.uint64).reshape(M, K // 64)
    return torch.from_numpy(np.ascontiguousarray(w.T).view(np.int64)).to(DEV)


def fp16_spacing(a):
    return np.spacing(np.abs(a).astype(np.float16)).astype(np.float32)


def problem(rpi, nimg, N, K, seed, densities=(0.03, 0.3, None)):
    """Operands of one down projection on the device: x, w, bias, residual, the sets' dense masks (None = all-zero)
    and their stacked K-major form."""
    M = rpi * nimg
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, generator=g, device=DEV).half()
    w = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).half()
    b = (torch.randn(N, generator=g, device=DEV) * 0.1).half()
    r = torch.randn(M, N, generator=g, device=DEV).half()
    masks = [torch.zeros(N, K, dtype=torch.bool, device=DEV) if d is None
             else torch.rand(N, K, generator=g, device=DEV) < d for d in densities]
    wmasks = torch.stack([ops.wmask_kmajor(packed(m.cpu().numpy())) for m in masks])
    return x, w, b, r, masks, wmasks


def fp32_ref(x, w, b, r, masks, table, rpi, keepb=None):
    xf = x.float() if keepb is None else x.float() * keepb.float()
    out = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    for i, s in enumerate(table):
        rows = slice(i * rpi, (i + 1) * rpi)
        out[rows] = xf[rows] @ (w.float() * (~masks[s]).float()).t()
    return out + b.float() + r.float()


def within_fp32_bound(y, ref):
    err = (y.float() - ref).abs().max().item()
    bound = 1e-2 * max(1.0, ref.abs().max().item())
    print(f"max |y - fp32| = {err:.4e} (bound {bound:.4e})")
    return err <= bound


# ---- sdmoe_wmask_union_sets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [1, 320 * 20 + 3])
def test_wmask_union_sets_is_exact(words):
    rng = np.random.default_rng(words)
    masks = rng.integers(-2 ** 63, 2 ** 63, (5, words), dtype=np.int64)
    selects = [0, 1 << 2, 0b11111, 0b10110]
    out = ops.wmask_union_sets(torch.from_numpy(masks).to(DEV),
                               torch.tensor(selects, dtype=torch.int32, device=DEV)).cpu().numpy()
    assert out.shape == (4, words) and out.dtype == np.int64
    for s, sel in enumerate(selects):
        rows = [c for c in range(5) if (sel >> c) & 1]
        exp = np.bitwise_or.reduce(masks[rows], axis=0) if rows else np.zeros(words, dtype=np.int64)
        assert np.array_equal(out[s], exp), (words, sel)
    # into a caller's buffer, select bit 31 as an int32 bit pattern, bits past the concepts ignored
    buf = torch.full((2, words), -1, dtype=torch.int64, device=DEV)
    sel = torch.from_numpy(np.array([0x80000001, 0xFFFFFFE0], dtype=np.uint32).view(np.int32).copy()).to(DEV)
    got = ops.wmask_union_sets(torch.from_numpy(masks).to(DEV), sel, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert np.array_equal(buf[0].cpu().numpy(), masks[0]) and int(buf[1].abs().sum()) == 0


# ---- sdmoe_linear_masked_sets: K1 row independence, K2 agreement with sdmoe_linear_masked, K3 the forced tile ------
# (rows_per_img, nimg, N, K, the tile rows the launch takes)
SHAPES = [(256, 6, 320, 1280, 64),        # 64-row tile
          (1024, 16, 640, 2560, 128),     # 128x160 tile
          (256, 180, 320, 1280, 256),     # 256x320 tile, one image per tile row
          (4096, 16, 320, 1280, 256),     # the bench's 64x64 shape
          (64, 16, 1280, 5120, 64)]       # the mid block: forced 64-row tile with split-K


@pytest.mark.parametrize("rpi,nimg,N,K,tile_rows", SHAPES, ids=[f"{s[0]}x{s[1]}_{s[2]}x{s[3]}" for s in SHAPES])
def test_linear_masked_sets_rows_take_their_images_set(rpi, nimg, N, K, tile_rows):
    M = rpi * nimg
    x, w, b, r, masks, wmasks = problem(rpi, nimg, N, K, seed=rpi + nimg + N)
    table = [(i + i // 3) % 3 for i in range(nimg)]  # neighbouring images always on different sets
    assert all(table[i] != table[i + 1] for i in range(nimg - 1)) and set(table) == {0, 1, 2}
    g = torch.Generator().manual_seed(M)
    keepb = torch.rand(M, K, generator=g) < 0.25
    keep_dev = keep_words(keepb.numpy())
    img = torch.tensor(table, device=DEV).repeat_interleave(rpi)
    for keep in (None, keep_dev):
        plan = ops.gemm_plan_sets(M, N, K, rpi, keep=keep is not None, residual=True)
        assert plan["tile"][0] == tile_rows, plan
        mode = "wmask" if keep is None else "keepw"
        plain = ops.gemm_plan(mode, M, N, K, residual=True)
        forced = rpi % plain["tile"][0] != 0
        assert forced == ((rpi, N, K) == (64, 1280, 5120))
        if forced:
            assert plan["ksplit"] > 1  # the mid block splits K on its 64-row tiles too
        mixed = ops.linear_masked_sets(x, w, b, wmasks=wmasks, image_set=table, rows_per_img=rpi, keep=keep, residual=r)
        uniform = [ops.linear_masked_sets(x, w, b, wmasks=wmasks, image_set=[s] * nimg, rows_per_img=rpi, keep=keep,
                                          residual=r) for s in range(3)]
        # K1: every row of the mixed call is the row of the uniform call on its image's set, bit for bit
        for s in range(3):
            rows = img == s
            assert torch.equal(mixed[rows], uniform[s][rows]), (s, keep is not None)
        # ... and the sets matter: an image on another set differs
        for i in (0, nimg - 1):
            rows = slice(i * rpi, (i + 1) * rpi)
            other = (table[i] + 1) % 3
            assert not torch.equal(mixed[rows], uniform[other][rows])
        # a device table the caller checked gives the same launch
        tab_dev = torch.tensor(table, dtype=torch.int32, device=DEV)
        assert torch.equal(ops.linear_masked_sets(x, w, b, wmasks=wmasks, image_set=tab_dev, rows_per_img=rpi, keep=keep,
                                                  residual=r), mixed)
        # K2: a uniform table is sdmoe_linear_masked itself wherever the two launches split K alike
        if plan["ksplit"] == plain["ksplit"]:
            assert not forced
            for s in range(3):
                assert torch.equal(uniform[s], ops.linear_masked(x, w, b, keep=keep, wmask=wmasks[s], residual=r)), s
        # K3: the forced tile (and every shape small enough for a quick fp32 product) against fp32
        if M <= 4096:
            ref = fp32_ref(x, w, b, r, masks, table, rpi, None if keep is None else keepb.to(DEV))
            assert within_fp32_bound(mixed, ref)


def test_linear_masked_sets_validates_its_table():
    x, w, b, r, masks, wmasks = problem(64, 2, 320, 1280, seed=3)
    kw = dict(wmasks=wmasks, rows_per_img=64)
    for bad in ([0, 3], [0, -1], [0], [0, 1, 2]):
        with pytest.raises(ValueError):
            ops.linear_masked_sets(x, w, b, image_set=bad, **kw)
    with pytest.raises(ValueError):
        ops.linear_masked_sets(x, w, b, image_set=[0, 1], wmasks=wmasks[:, :-1], rows_per_img=64)
    with pytest.raises(ValueError):
        ops.linear_masked_sets(x, w, b, image_set=[0, 1], wmasks=wmasks, rows_per_img=48)


def test_linear_masked_sets_fallback_runs_per_image_run():
    """rows_per_img = 16: no tile fits an image, so the wrapper runs sdmoe_linear_masked once per run of images on one
    set. Each run equals that call on the run's slice bit for bit; the whole is within the fp32 bound."""
    rpi, nimg, N, K = 16, 6, 320, 1280
    M = rpi * nimg
    from sdmoe import _lib
    with pytest.raises(_lib.SdmoeError):
        ops.gemm_plan_sets(M, N, K, rpi, keep=True, residual=True)
    x, w, b, r, masks, wmasks = problem(rpi, nimg, N, K, seed=16)
    table = [0, 0, 1, 2, 2, 0]
    g = torch.Generator().manual_seed(M)
    keepb = torch.rand(M, K, generator=g) < 0.25
    keep = keep_words(keepb.numpy())
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
    y = ops.linear_masked_sets(x, w, b, wmasks=wmasks, image_set=table, rows_per_img=rpi, keep=keep, residual=r, out=out)
    assert y.data_ptr() == out.data_ptr() and not torch.isnan(out).any()
    runs = ops.image_set_runs(table)
    assert runs == [(0, 2, 0), (2, 3, 1), (3, 5, 2), (5, 6, 0)]
    for i0, i1, s in runs:
        rows = slice(i0 * rpi, i1 * rpi)
        exp = ops.linear_masked(x[rows], w, b, keep=keep[:, rows].contiguous(), wmask=wmasks[s], residual=r[rows])
        assert torch.equal(y[rows], exp), (i0, i1, s)
    assert within_fp32_bound(y, fp32_ref(x, w, b, r, masks, table, rpi, keepb.to(DEV)))
    # the per-run path needs the host form of the table
    with pytest.raises(_lib.SdmoeError):
        ops.linear_masked_sets(x, w, b, wmasks=wmasks, image_set=torch.tensor(table, dtype=torch.int32, device=DEV),
                               rows_per_img=rpi)


# ---- the receiver on the reference's own hook outputs ------------------------------------------------------------------
def test_per_prompt_receiver_on_reference_fixture(parity_report):
    """tests/golden/wanda_320x1280_float16.npz: outputs of the reference's linear_hook_fn for five layer masks on one
    input. The five masks act as five concepts. One launch: image j is the 32 fixture rows twice (64 rows per image),
    its set {concept j}, expected rows out[j] twice. Fallback: the raw [2, 16, 1280] input, sets [{a}, {b}], expected
    out[a][0] and out[b][1]. Both within the 2-ulp unit of test_wanda_hook_on_reference_fixture."""
    from neuron_receivers import WandaRemoveNeuronsFast, WandaRemovePerPrompt
    from sdmoe.unet import LoRACompatibleLinear
    with np.load(os.path.join(GOLD, "wanda_320x1280_float16.npz"), allow_pickle=False) as z:
        c = {k: z[k] for k in z.files}
    bits = c["mask_bits"]  # [5, 320, 160]
    L = bits.shape[0]
    removers = {f"c{j}": WandaRemoveNeuronsFast.from_packed(0, {0: {0: bits[j]}}, 1, 1, store_gates=False)
                for j in range(L)}
    rec = WandaRemovePerPrompt(removers, store_gates=False)
    w, b = synth.down_weights(320, int(c["w_seed"]))
    lin = LoRACompatibleLinear(torch.from_numpy(w).half().to(DEV), torch.from_numpy(b).half().to(DEV))
    x = torch.from_numpy(c["x"]).to(DEV)  # [2, 16, 1280]
    ref_all = c["out"].astype(np.float32)  # [5, 2, 16, 320]

    def ulps(y, ref):
        unit = np.maximum(fp16_spacing(ref), fp16_spacing(np.full_like(ref, 0.25 * np.abs(ref).max())) / 2)
        return float((np.abs(y - ref) / unit).max())

    # one launch: five images of 64 rows, image j on {concept j}
    img = x.reshape(32, 1280).repeat(2, 1)
    rec.set_prompt_concepts([[f"c{j}"] for j in range(L)])
    assert ops.gemm_plan_sets(L * 64, 320, 1280, 64)["tile"][0] == 64
    y = rec.linear_hook_fn(lin, (img.repeat(L, 1).view(L, 64, 1280),), None)
    assert tuple(y.shape) == (L, 64, 320) and (rec.timestep, rec.layer) == (1, 0)
    worst = 0.0
    for j in range(L):
        ref = np.tile(ref_all[j].reshape(32, 320), (2, 1))
        u = ulps(y[j].float().cpu().numpy(), ref)
        worst = max(worst, u)
        assert u <= 2.0, f"image {j}: {u} ulps"
        if j:  # another concept's mask gives another result
            assert np.abs(y[j].float().cpu().numpy() - np.tile(ref_all[j - 1].reshape(32, 320), (2, 1))).max() > 0
    # fallback: two images of 16 rows
    a, bb = 1, 3
    rec.set_prompt_concepts([[f"c{a}"], [f"c{bb}"]])
    rec.reset_time_layer()
    y2 = rec.linear_hook_fn(lin, (x,), None).float().cpu().numpy()
    worst2 = max(ulps(y2[0], ref_all[a][0]), ulps(y2[1], ref_all[bb][1]))
    assert worst2 <= 2.0, worst2
    parity_report("per_prompt_hook_fixture[float16]", layers=L, max_ulps=worst, max_ulps_fallback=worst2)


# ---- through the pipeline --------------------------------------------------------------------------------------
PROMPTS = ["a dog in the style of van gogh", "a painting of a river", "water lilies by monet"]
SETS = [["A"], [], ["A", "B"]]
STEPS = 3


class _Ctx:
    pass


@pytest.fixture(scope="module", params=["plain", "routed", "routed_w320"])
def ctx(request):
    """3 prompts with CFG, 3 DDIM steps, two concepts of random 0.3-density masks; the mixed call's images computed
    once. plain / routed: UNetConfig.tiny(32) (levels 32x32 .. 4x4: one-launch, forced-tile and per-run calls all
    occur; no tiny GEMM splits K, so the per-run calls keep the bits too), routed = MoE-fied with moefy_tiny -- at tiny
    widths (4C = 256 / 512, not a multiple of 80) the routed GEGLU hands over the natural neuron order, so the hook
    runs linear_hook_fn behind it. routed_w320: four 320-channel levels at 64x64 latents, MoE-fied with balanced
    20-neuron experts, where the FeedForward keeps its fused path and calls fused_linear (masks permuted, keep bits in
    the same launch); every level there has >= 64 rows per image, so every call is the one launch."""
    from neuron_receivers import MultiConceptRemoverWanda, WandaRemoveNeuronsFast, WandaRemovePerPrompt
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    from sdmoe.unet import UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    c = _Ctx()
    c.kind = request.param
    if c.kind == "routed_w320":
        cfg = UNetConfig(block_out_channels=(320, 320, 320, 320), attention_heads=8, cross_attention_dim=128,
                         sample_size=64, name="w320")
    else:
        cfg = UNetConfig.tiny(32)
    unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 41), cfg, DEV)
    c.pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=STEPS)
    c.routed = c.kind != "plain"
    if c.kind == "routed":
        from test_gpu_unet import moefy_tiny
        moefy_tiny(c.pipe)
    elif c.kind == "routed_w320":
        from moefication.helper import moefy_synthetic
        from sparsity.relufy_model import find_and_change_geglu
        find_and_change_geglu(c.pipe.unet)
        moefy_synthetic(c.pipe, 0.2, 20, seed=43)
    c.geglus = [m for n, m in unet.named_modules() if n.endswith("ff.net.0")]
    downs = [m for n, m in unet.named_modules() if n.endswith("ff.net.2")]
    c.T, c.L = STEPS, len(downs)
    rng = np.random.default_rng(42)
    masks = {k: {t: {l: (rng.random(tuple(downs[l].weight.shape)) < 0.3).astype(np.int64) for l in range(c.L)}
                 for t in range(c.T)} for k in ("A", "B")}
    c.removers = {k: WandaRemoveNeuronsFast(0, None, c.T, c.L, masks=m, store_gates=False) for k, m in masks.items()}
    c.mc = MultiConceptRemoverWanda(None, 0, c.T, c.L, concepts_to_remove=["A", "B"], removers=c.removers)
    c.rec = WandaRemovePerPrompt(c.removers, seed=0, store_gates=False)

    def run(sets):
        c.rec.set_prompt_concepts(sets)
        c.rec.reset_time_layer()
        out, _ = c.rec.observe_activation(c.pipe, PROMPTS)
        assert (c.rec.timestep, c.rec.layer) == (c.T, 0)
        return [o.clone() for o in out]
    c.run = run
    c.mixed = run(SETS)
    return c


def test_pipeline_images_follow_their_prompts_set(ctx):
    """P1: image i of the mixed call equals, bit for bit, image i of the uniform call with every prompt on set s_i;
    the masked prompts differ from their unmasked versions, the {} prompt equals its own."""
    stacks = [k for k in ctx.rec._dev if k[0] == "stack"]  # one per (t, l), built once, in the layer's neuron order
    assert len(stacks) == ctx.T * ctx.L
    if ctx.kind == "routed_w320":  # fused_linear ran at every layer: masks permuted into the experts' neuron order
        assert all(k[3] is False for k in stacks), "the fused routed path did not run"
        assert all(m._out_keep is not None for m in ctx.geglus)
    else:
        assert all(k[3] is True for k in stacks)
    uniform = [ctx.run([s] * len(PROMPTS)) for s in SETS]
    empty = uniform[1]
    for i in range(len(PROMPTS)):
        assert torch.equal(ctx.mixed[i], uniform[i][i]), i
        for j in range(len(PROMPTS)):
            if j != i:
                assert not torch.equal(ctx.mixed[i], uniform[j][i]), (i, j)
    assert torch.equal(ctx.mixed[1], empty[1])
    assert not torch.equal(ctx.mixed[0], empty[0]) and not torch.equal(ctx.mixed[2], empty[2])
    assert len([k for k in ctx.rec._dev if k[0] == "stack"]) == len(stacks)  # reused by the later calls


def test_pipeline_uniform_union_matches_the_union_remover(ctx, parity_report):
    """P2: every prompt on {A, B} through the new receiver vs the existing union remover's batched call with the mask
    applied in the GEMM. The two differ only in split order at the forced-tile and per-run levels."""
    from test_gpu_unet import rel_l2
    got = ctx.run([["A", "B"]] * len(PROMPTS))
    ctx.mc.reset_union_remover()
    ctx.mc.handle_multiple_concepts(["A", "B"])
    u = ctx.mc.union_neuron_remover
    u.bake_budget_bytes = 0
    u.reset_time_layer()
    exp, _ = u.observe_activation(ctx.pipe, PROMPTS)
    assert (u.timestep, u.layer) == (ctx.T, 0)
    rel = rel_l2(torch.stack(got), torch.stack(exp))
    print(f"rel L2 vs the union remover = {rel:.3e}")
    parity_report(f"per_prompt_uniform_vs_union_remover[{ctx.kind}]", rel_l2=rel)
    assert rel <= 3e-2


def test_remove_concepts_batch(ctx, parity_report):
    """One batched call returns the removal images in prompt order: the mixed call's images; image 0 (set {A}) is, bit
    for bit, image 0 of the existing remover of A run over the same batch. On the tiny U-Net each image is also within
    the pipeline's bound of the one-prompt path (removers[c] / the union remover / the unedited pipeline) started from
    the same latents (prompt_offset = i).
    routed_w320 leaves the one-prompt comparison out: under relu top-k routing at SD widths a batch of 3 and a batch
    of 1 take different split-K plans in the convs, and the near-tie expert flips that follow make the EXISTING
    removers differ between the two batch sizes by as much (measured 3.6e-2 for prompt 0 with these 0.3-density
    masks); at equal batch the new path is bit-identical to the existing one (above, and P2)."""
    from test_gpu_unet import rel_l2
    imgs = ctx.mc.remove_concepts_batch(ctx.pipe, PROMPTS, SETS)
    assert len(imgs) == len(PROMPTS)
    for i in range(len(PROMPTS)):
        assert torch.equal(imgs[i], ctx.mixed[i]), i
    ctx.removers["A"].reset_time_layer()
    same_batch, _ = ctx.removers["A"].observe_activation(ctx.pipe, PROMPTS)
    assert torch.equal(imgs[0], same_batch[0])
    with pytest.raises(ValueError):
        ctx.mc.remove_concepts_batch(ctx.pipe, PROMPTS, SETS[:2])
    if ctx.kind == "routed_w320":
        return
    worst = 0.0
    try:
        for i, (p, cs) in enumerate(zip(PROMPTS, SETS)):
            ctx.pipe.prompt_offset = i
            if not cs:
                torch.manual_seed(0)
                one = ctx.pipe(p).images[0]
            elif len(cs) == 1:
                ctx.removers[cs[0]].reset_time_layer()
                one, _ = ctx.removers[cs[0]].observe_activation(ctx.pipe, p)
            else:
                ctx.mc.reset_union_remover()
                ctx.mc.handle_multiple_concepts(cs)
                ctx.mc.union_neuron_remover.reset_time_layer()
                one, _ = ctx.mc.union_neuron_remover.observe_activation(ctx.pipe, p)
            rel = rel_l2(imgs[i], one)
            print(f"prompt {i} {cs}: rel L2 vs the one-prompt path = {rel:.3e}")
            worst = max(worst, rel)
            assert rel <= 3e-2, (i, rel)
    finally:
        ctx.pipe.prompt_offset = 0
    parity_report(f"remove_concepts_batch_vs_one_prompt[{ctx.kind}]", rel_l2=worst)
