"""The device object-erasure scorer on the MI355X: csrc/imagenet.hip, sdmoe.resnet and sdmoe.scoring.ObjectScorer.

Kernels (stem_rows, maxpool3x3s2, avgpool_rows, add_relu, topk_hits) and the front end are integer-exact or correctly
rounded, so every output is held EQUAL (bit for bit) to tests/resnet_ref.py, Pillow or torch on the same values.
Output buffers sit inside poisoned allocations that are checked afterwards; inputs and outputs are also passed as
strided or misaligned views, which take the kernels' element-wise paths.

Network, layer by layer (each layer fed the device's own previous output, so a wrong layer is named): against the
restatement's fp16-storage mode on the same input. Bar per layer: rel-L2 <= 4 * 2^-11 = 1.95e-3. Reasoning: between a
block's input and output there are four places where the two sides round to fp16 or not (conv1, conv2, and -- only in
the restatement, the device's projection blocks fuse them -- conv3 and the shortcut), each at most 2^-11 relative per
element of a tensor whose norm is comparable to the output's; fp32 accumulation order adds ~1e-6. A wrong layout,
stride or bias is an O(1) error.
Not yet measured on an MI355X: the test prints each layer's figure before it asserts.

End-to-end logits against the fp32 restatement (BatchNorm unfolded, fp32 weights): bar = 3 x the rel-L2 gap between
the restatement's fp32 and fp16-storage modes, computed on the CPU for the same seed in the test; the factor covers
the accumulation order and the fp16 products, which that mode does not model.
Not yet measured on an MI355X: the test prints both figures; CPU gaps are in profiles/object_score_parity.txt.

Top-5 sets, per-image hits and acc: EQUAL to the fp32 restatement's on every image whose reference 5th-to-6th logit
gap exceeds delta = 4 x the largest |logit difference| between the two CPU modes; at most 10 % of the images may be
excluded (resnet_ref.TOPK_SEEDS: none, none and one of 12)."""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resnet_ref as R  # noqa: E402
from sdmoe import _lib, ops  # noqa: E402
from sdmoe.resnet import ResNet, ResNetConfig, make_resnet_state_dict  # noqa: E402
from sdmoe.scoring import ObjectScorer  # noqa: E402

DEV = "cuda:0"
POISON16 = 777.0
LAYER_BAR = 4 * 2.0 ** -11


def poisoned(rows, cols, ld=None, offset=64, dtype=torch.float16, fill=POISON16):
    """A [rows, cols] view (row stride ld) `offset` elements into a poisoned allocation -> (flat, view, mask of the
    view's own elements)."""
    ld = cols if ld is None else ld
    n = offset + rows * ld + 64
    flat = torch.full((n,), fill, dtype=dtype, device=DEV)
    view = flat[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[offset:offset + rows * ld].view(rows, ld)[:, :cols] = True
    return flat, view, mask


def poison_intact(flat, mask, fill=POISON16):
    return bool((flat[~mask] == fill).all())


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


# ------------------------------------------------------------------------------------------------------- stem_rows
@pytest.mark.parametrize("B,S,offset,ld", [(2, 8, 64, 192), (2, 15, 64, 192), (2, 224, 64, 192), (1, 16, 64, 192),
                                           (2, 15, 65, 192), (1, 16, 64, 200), (2, 8, 64, 196)])
def test_stem_rows_exact(B, S, offset, ld):
    """Aligned (16-byte stores) and, with an odd offset or a row stride that is no multiple of 8, element-wise."""
    u8 = np.random.default_rng(S * 10 + B).integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    u8[0, 0, 0] = (0, 255, 128)
    u8[-1, -1, -1] = (255, 0, 1)
    ref = R.stem_rows(u8)
    So = (S - 1) // 2 + 1
    flat, out, mask = poisoned(B * So * So, ops.STEM_KPAD, ld, offset)
    ops.stem_rows(torch.from_numpy(u8).to(DEV), out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.int16), ref.view(np.int16))
    assert not got[:, ops.STEM_K:].any()
    # border rows: the first output pixel's taps with ky < 3 or kx < 3 lie in the padding and are exactly zero
    first = got[0, :ops.STEM_K].reshape(3, 7, 7)
    assert not first[:, :3, :].any() and not first[:, :, :3].any() and first[:, 3, 3].all()
    assert poison_intact(flat, mask)


# --------------------------------------------------------------------------------------------------------- maxpool
@pytest.mark.parametrize("H,W", [(8, 8), (7, 5), (112, 112)])
@pytest.mark.parametrize("C,ldx,offset", [(64, 64, 64), (8, 8, 64), (64, 72, 64), (8, 12, 65)])
@pytest.mark.parametrize("kind", ["normal", "negative"])
def test_maxpool_equals_torch(H, W, C, ldx, offset, kind):
    B = 2
    g = torch.Generator().manual_seed(H * 100 + W + C)
    x = torch.randn(B, H, W, C, generator=g).half()
    if kind == "negative":  # a zero-padding bug would win everywhere
        x = -x.abs() - 1
    else:
        x[0, 0, 0, 0] = float("nan")
        x[1, H - 1, W - 1, C - 1] = float("-inf")
    ref = torch.nn.functional.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).half()
    OH, OW = ref.shape[1:3]
    assert (OH, OW) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    _, xin, _ = poisoned(B * H * W, C, ldx, offset)
    xin.copy_(x.reshape(-1, C))
    flat, out, mask = poisoned(B * OH * OW, C, ldx, offset)
    ops.maxpool3x3s2(xin, B, H, W, out=out)
    torch.cuda.synchronize()
    got, ref = out.cpu().reshape(-1), ref.reshape(-1)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) == (0 if kind == "negative" else 1)
    assert np.array_equal(bits(got[~nan]), bits(ref[~nan]))
    assert poison_intact(flat, mask)


# --------------------------------------------------------------------------------------------------------- avgpool
@pytest.mark.parametrize("HW", [1, 4, 49])
@pytest.mark.parametrize("C,ldx,offset", [(64, 64, 64), (2048, 2048, 64), (64, 72, 65)])
def test_avgpool_rows_exact(HW, C, ldx, offset):
    B = 3
    x = (torch.randn(B, HW, C, generator=torch.Generator().manual_seed(HW + C)) * 3 + 1).half()
    acc = torch.zeros(B, C, dtype=torch.float32)
    for r in range(HW):  # fp32 sum in row order
        acc = acc + x[:, r].float()
    ref = (acc / torch.tensor(float(HW), dtype=torch.float32)).half()
    _, xin, _ = poisoned(B * HW, C, ldx, offset)
    xin.copy_(x.reshape(-1, C))
    flat, out, mask = poisoned(B, C, ldx, offset)
    ops.avgpool_rows(xin, B, HW, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu()), bits(ref))
    assert poison_intact(flat, mask)


# -------------------------------------------------------------------------------------------------------- add_relu
SPECIAL = [0.0, -0.0, 6e-8, -6e-8, 5.96e-8, 6.1e-5, -6.1e-5, 65504.0, -65504.0, 1.0, -1.0, 0.333, 2048.0, 2049.0]


@pytest.mark.parametrize("n", [1, 7, 8 * 37 + 3, 8 * 4099 + 3])
@pytest.mark.parametrize("offset", [64, 65])      # 16-byte aligned / 2-byte aligned
@pytest.mark.parametrize("inplace", [False, True])
def test_add_relu_bitwise(n, offset, inplace):
    g = torch.Generator().manual_seed(n)
    sp = torch.tensor(SPECIAL).half()
    a = torch.randn(n, generator=g).half()
    b = torch.randn(n, generator=g).half()
    m = min(n, len(sp) ** 2)  # every pair of special values where there is room
    a[:m] = sp.repeat_interleave(len(sp))[:m]
    b[:m] = sp.repeat(len(sp))[:m]
    ref = torch.relu(a + b)
    fa, av, ma = poisoned(1, n, None, offset)
    _, bv, _ = poisoned(1, n, None, offset)
    av.copy_(a[None])
    bv.copy_(b[None])
    if inplace:
        flat, out, mask = fa, av, ma
    else:
        flat, out, mask = poisoned(1, n, None, offset)
    ops.add_relu(av[0], bv[0], out=out[0])
    torch.cuda.synchronize()
    assert np.array_equal(bits(out[0].cpu()), bits(ref))
    assert poison_intact(flat, mask)
    if n > 16:
        assert (bits(ref) == np.int16(-32768)).any()  # -0 + -0 stays -0, as in torch


# ------------------------------------------------------------------------------------------------------- topk_hits
def topk_rows(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g).half()
    x[0] = 0.5                                   # all equal: ids 0 .. k-1
    x[1, : C // 2] = x[1, C // 2:C // 2 * 2]     # exact ties in pairs
    x[2, C - 1] = float("nan")                   # NaN ranks first
    x[2, 0] = float("inf")
    x[3] = float("-inf")
    x[3, C // 2] = -1.0
    x[4, 0], x[4, 1] = 0.0, -0.0                 # -0 == +0: the lower id first
    x[4, 2:] = -x[4, 2:].abs() - 1
    return x


@pytest.mark.parametrize("C,k,ld", [(5, 5, 5), (5, 1, 8), (40, 5, 40), (1000, 5, 1000), (1000, 8, 1003), (70, 3, 70)])
def test_topk_hits_exact(C, k, ld):
    n, G = 9, 4
    x = topk_rows(n, C, C + k)
    rng = np.random.default_rng(C)
    words = (C + 31) // 32
    member = rng.random((G, C)) < (0.5 if C <= 40 else 0.004)
    member[3] = False
    member[3, C - 1] = True
    table = np.zeros((G, words), np.uint32)
    for g_, c in zip(*np.nonzero(member)):
        table[g_, c >> 5] |= np.uint32(1 << (c & 31))
    label = rng.integers(0, G, n).astype(np.int32)
    label[2] = 3  # the NaN row: class C - 1 is in its top-k
    _, lg, _ = poisoned(n, C, ld, 65)
    lg.copy_(x)
    topk, hit, total = ops.topk_hits(lg, torch.from_numpy(table.view(np.int32)).to(DEV),
                                     torch.from_numpy(label).to(DEV), k)
    torch.cuda.synchronize()
    ref = R.topk_stable(x.float().numpy(), k)
    assert np.array_equal(topk.cpu().numpy(), ref)
    assert ref[2, 0] == C - 1 and (C == 5 or ref[0].tolist() == list(range(k)))
    ref_hit = np.array([int(member[label[i], ref[i]].any()) for i in range(n)], np.int32)
    assert np.array_equal(hit.cpu().numpy(), ref_hit) and ref_hit[2] == 1
    assert total.item() == int(ref_hit.sum())


def test_topk_hits_label_out_of_range_is_an_error_status():
    n, C, G = 6, 40, 3
    x = topk_rows(n, C, 1)
    table = torch.full((G, 2), -1, dtype=torch.int32, device=DEV)  # every class hits
    for bad in (G, -1, 1 << 30):
        label = torch.zeros(n, dtype=torch.int32)
        label[4] = bad
        topk, hit, total = ops.topk_hits(x.to(DEV), table, label.to(DEV), 5)
        assert hit.cpu().tolist() == [1, 1, 1, 1, -1, 1] and total.item() == -1
        assert np.array_equal(topk.cpu().numpy(), R.topk_stable(x.float().numpy(), 5))
    with pytest.raises(ValueError):
        ops.topk_hits(x.to(DEV), table, torch.zeros(n, dtype=torch.int32, device=DEV), 9)
    lib = _lib.load()
    assert lib.sdmoe_topk_hits(1, 40, 1, 40, 41, 1, 1, 1, 1, 1, 1, None) == -1
    assert lib.sdmoe_maxpool3x3s2(1, 12, 1, 4, 4, 12, 1, 12, None) == -2
    assert lib.sdmoe_add_relu(1, 2, 2, 8, None) == -2


# ------------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("shape,resize,crop", [((64, 64), 40, 36), ((40, 56), 36, 36), ((43, 56), 39, 36),
                                               ((512, 512), 232, 224)])
def test_front_end_crop_equals_pillow(shape, resize, crop):
    B = 2
    u8 = np.random.default_rng(shape[1]).integers(0, 256, (B,) + shape + (3,), dtype=np.uint8)
    ref = np.stack([R.preprocess_u8(i, crop, resize) for i in u8])
    flat = torch.full((ref.size + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    out = flat[64:64 + ref.size].view(B, crop, crop, 3)
    ops.clip_preprocess(torch.from_numpy(u8).to(DEV), crop, u8_out=out, resize=resize, filter="bilinear",
                        half_even=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    assert bool((flat[:64] == 0xA5).all()) and bool((flat[64 + ref.size:] == 0xA5).all())


# --------------------------------------------------------------------------------------------------------- network
@functools.lru_cache(maxsize=None)
def net_case(name):
    """tiny() at crop 64 or resnet50() at 224, B = 2: weights, crops, the model on the device."""
    cfg, crop, resize = (ResNetConfig.tiny(), 64, 72) if name == "tiny" else (ResNetConfig.resnet50(), 224, 232)
    sd = make_resnet_state_dict(cfg, 0)
    images = R.smooth_images(7, ((crop + 40, crop + 8), (crop + 16, crop + 64)))
    u8 = R.crops(images, crop, resize)
    return {"cfg": cfg, "sd": sd, "u8": u8, "model": ResNet.from_state_dict(sd, cfg, DEV)}


@pytest.mark.parametrize("name", ["tiny", "resnet50"])
def test_network_layer_by_layer(name):
    case = net_case(name)
    cfg, model, u8 = case["cfg"], case["model"], case["u8"]
    ref = R.ResNetRef(case["sd"], cfg, fp16_storage=True)
    B, S = u8.shape[0], u8.shape[1]
    figures = []

    def check(layer, got, want, H, W, C):
        assert tuple(got.shape) == (B * H * W, C), (layer, tuple(got.shape), (B * H * W, C))
        err = R.rel_l2(got.float().cpu(), R.to_rows(want))
        figures.append((layer, err, got.float().abs().max().item()))
        print(f"{name} {layer}: rel-L2 {err:.3e}, max |activation| {figures[-1][2]:.2f}")
        assert err <= LAYER_BAR, (layer, err)

    with torch.no_grad():
        x, So = model.stem_conv(torch.from_numpy(u8).to(DEV))
        assert So == S // 2
        check("stem", x, ref.stem_conv(R.pixel_values(u8)), So, So, cfg.stem_width)
        H = W = So // 2
        pooled = ops.maxpool3x3s2(x, B, So, So)
        want = ref.maxpool(R.from_rows(x.float().cpu(), B, So, So))
        assert np.array_equal(bits(pooled.cpu()), bits(R.to_rows(want).half()))  # a max of the same values: equal
        x = pooled
        for blk, spec in zip(model.blocks, cfg.blocks()):
            want = ref.block(R.from_rows(x.float().cpu(), B, H, W), spec)
            x, H, W = blk.run(x, B, H, W)
            assert (H, W) == tuple(want.shape[2:])
            check(spec[0], x, want, H, W, spec[3])
        assert (H, W) == (S // 32, S // 32)
        want = ref.head(R.from_rows(x.float().cpu(), B, H, W))
        logits = model.head(x, B, H * W)
        check("head", logits, want[:, :, None, None], 1, 1, cfg.num_classes)
    assert max(f[2] for f in figures) < 1000  # far inside fp16's range
    # the whole pass in one call gives the same logits as the staged one
    assert torch.equal(model(torch.from_numpy(u8).to(DEV)), logits)


@functools.lru_cache(maxsize=None)
def resnet50_refs():
    case = net_case("resnet50")
    pix = R.pixel_values(case["u8"])
    return R.ResNetRef(case["sd"], case["cfg"]).forward(pix), R.ResNetRef(case["sd"], case["cfg"], True).forward(pix)


def test_logits_end_to_end_resnet50():
    case = net_case("resnet50")
    ref32, ref16 = resnet50_refs()
    gap = R.rel_l2(ref16, ref32)
    got = case["model"](torch.from_numpy(case["u8"]).to(DEV)).float().cpu()
    err = R.rel_l2(got, ref32)
    print(f"resnet50 224 B=2: device vs fp32 restatement rel-L2 {err:.3e}; fp16-storage mode vs fp32 {gap:.3e}; "
          f"bar {3 * gap:.3e}")
    assert torch.isfinite(got).all() and err <= 3 * gap


@functools.lru_cache(maxsize=None)
def scored(seed):
    """One top-5 case through ObjectScorer, images as a mixed-size list on the device."""
    case = R.topk_case(seed)
    model = ResNet.from_state_dict(case["sd"], case["cfg"], DEV)
    scorer = ObjectScorer(model, R.categories40(), size=R.TOPK_CROP, resize=R.TOPK_RESIZE)
    images = [i.to(DEV) for i in case["images"]]
    labels = R.topk_labels(len(images))
    return case, scorer, images, labels, scorer.score_erasure(images, labels)


@pytest.mark.parametrize("seed", R.TOPK_SEEDS)
def test_scorer_front_end_and_logits(seed):
    case, scorer, images, labels, _ = scored(seed)
    assert np.array_equal(scorer.preprocess_u8(images).cpu().numpy(), case["u8"])  # mixed sizes, through Pillow
    gap = R.rel_l2(case["ref16"], case["ref32"])
    got = scorer.logits(images).float().cpu()
    err = R.rel_l2(got, case["ref32"])
    print(f"tiny 64 seed {seed}: device vs fp32 restatement rel-L2 {err:.3e}; fp16-storage mode vs fp32 {gap:.3e}; "
          f"bar {3 * gap:.3e}")
    assert err <= 3 * gap


@pytest.mark.parametrize("seed", R.TOPK_SEEDS)
def test_top5_hits_and_acc_equal_reference(seed, tmp_path):
    case, scorer, images, labels, res = scored(seed)
    n, keep = len(images), case["keep"]
    assert n - int(keep.sum()) <= R.TOPK_MAX_EXCLUDED * n
    ref_topk = R.topk_stable(case["ref32"].numpy(), 5)
    ref_hits = R.hits(ref_topk, R.categories40(), labels)
    assert tuple(res["topk"].shape) == (n, 5) and res["topk"].dtype == torch.int32
    for i in np.flatnonzero(keep):
        assert set(res["topk"][i].tolist()) == set(ref_topk[i].tolist()), i
        assert res["hits"][i].item() == ref_hits[i], i
    assert res["acc"] == res["hits"].sum().item() / n
    if keep.all():
        assert res["acc"] == ref_hits.sum() / n
    else:
        assert abs(res["acc"] - ref_hits.sum() / n) <= (n - int(keep.sum())) / n
    assert torch.equal(scorer.topk(images), res["topk"])
    # the device's own top-k is the stable ranking of the device's own logits
    assert np.array_equal(res["topk"].numpy(), R.topk_stable(scorer.logits(images).float().cpu().numpy(), 5))
    scorer.write_results(tmp_path / "results.json", res)
    assert json.loads((tmp_path / "results.json").read_text()) == {"acc": res["acc"]}
    with pytest.raises(ValueError, match="labels"):
        scorer.score_erasure(images, labels[:-1])
    with pytest.raises(ValueError, match="categories"):
        ObjectScorer(scorer.model, None, size=R.TOPK_CROP, resize=R.TOPK_RESIZE).score_erasure(images, labels)
