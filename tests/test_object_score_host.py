"""Host logic of the object-erasure scorer (no GPU): the bilinear tables against Pillow, the ImageClassification size
and crop rule, BatchNorm folding, state-dict coverage, the reference's name match and the config checks; and the CPU
side of the GPU parity cases in tests/resnet_ref.py (the seeds it commits do what its comment says)."""
import numpy as np
import pytest
import torch
from PIL import Image

import clip_score_ref as C
import resnet_ref as R
from sdmoe import ops
from sdmoe.resnet import (ResNetConfig, fold_bn, make_resnet_state_dict, prepare_weights, resnet_param_specs)
from sdmoe.scoring import ObjectScorer, match_table

# (H, W) -> (out_h, out_w): the shapes of the issue's table check, downscales, an upscale and the identity
RESIZE_SHAPES = [((512, 512), (232, 232)), ((64, 64), (40, 40)), ((40, 56), (36, 50)), ((96, 64), (54, 36)),
                 ((17, 23), (36, 48)), ((36, 36), (36, 36)), ((768, 512), (348, 232))]


def table_resize(img, oh, ow, filter):
    """Pillow's two 8bpc passes driven by ops.clip_resample_coeffs' tables."""
    def tab(n_in, n_out):
        b, k, _ = ops.clip_resample_coeffs(n_in, n_out, filter=filter)
        return np.array(b, np.int32), np.array(k, np.int32)

    h, w = img.shape[:2]
    bx, kx = tab(w, ow)
    by, ky = tab(h, oh)
    return C._pass(C._pass(img, bx, kx, 1), by, ky, 0)


@pytest.mark.parametrize("shape,out", RESIZE_SHAPES)
def test_bilinear_tables_equal_pillow(shape, out):
    img = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((out[1], out[0]), Image.BILINEAR))
    assert np.array_equal(table_resize(img, out[0], out[1], "bilinear"), ref)


@pytest.mark.parametrize("n_in,n_out", [(512, 224), (64, 28), (56, 39), (23, 48), (36, 36), (768, 336)])
def test_bicubic_tables_unchanged(n_in, n_out):
    """The default filter still builds the tables of tests/clip_score_ref.py (the builder from before the filter
    argument, restated there), whole and for a crop window."""
    b, k, ks = ops.clip_resample_coeffs(n_in, n_out)
    rb, rk = C.coeffs(n_in, n_out)
    assert ks == rk.shape[1] and np.array_equal(np.array(b), rb) and np.array_equal(np.array(k), rk)
    assert (b, k, ks) == ops.clip_resample_coeffs(n_in, n_out, filter="bicubic")
    first, count = n_out // 4, n_out // 2
    bw, kw, _ = ops.clip_resample_coeffs(n_in, n_out, first, count)
    assert np.array_equal(np.array(bw), rb[first:first + count]) and np.array_equal(np.array(kw), rk[first:first + count])
    with pytest.raises(ValueError):
        ops.clip_resample_coeffs(n_in, n_out, filter="lanczos")


def test_size_rule_and_half_even_crop():
    assert ops.clip_resize_shape(512, 512, 232) == (232, 232) == R.resize_shape(512, 512, 232)
    assert ops.clip_resize_shape(768, 512, 232) == (348, 232) == R.resize_shape(768, 512, 232)
    assert ops.clip_resize_shape(40, 56, 36) == (36, 50) == R.resize_shape(40, 56, 36)
    assert ops.clip_resize_shape(500, 333, 232) == (348, 232)  # int(232 * 500 / 333) = int(348.35)
    # (h - crop) / 2 ending in .5: 3.5 -> 4 and 2.5 -> 2 under half-even, 3 and 2 under the CLIP path's floor
    assert ops.centre_crop_offsets(231, 229, 224, half_even=True) == (4, 2) == R.crop_offsets(231, 229, 224)
    assert ops.centre_crop_offsets(231, 229, 224) == (3, 2)
    assert ops.centre_crop_offsets(232, 348, 224, half_even=True) == (4, 62)
    # 40 x 56 -> 36 x 50, crop 36: left = round(7.0) = 7; 41 x 56 at resize 37: left = round(6.5) = 6 (floor too),
    # 43 x 56 at resize 39 crop 36: 39 x 50 -> top round(1.5) = 2, left round(7.0) = 7
    assert R.crop_offsets(*R.resize_shape(43, 56, 39), 36) == (2, 7)
    assert ops.centre_crop_offsets(*ops.clip_resize_shape(43, 56, 39), 36, half_even=True) == (2, 7)
    assert ops.centre_crop_offsets(*ops.clip_resize_shape(43, 56, 39), 36) == (1, 7)


@pytest.mark.parametrize("shape,resize,crop", [((43, 56), 39, 36), ((64, 64), 40, 36), ((96, 64), 72, 64)])
def test_plan_window_equals_pillow_crop(shape, resize, crop):
    """The plan's crop-window tables (what the device kernels are given) reproduce Pillow's resize + the half-even
    centre crop, including a case whose top offset ends in .5."""
    img = np.random.default_rng(7).integers(0, 256, shape + (3,), dtype=np.uint8)
    plan = ops.ClipResamplePlan(shape[0], shape[1], crop, "cpu", resize=resize, filter="bilinear", half_even=True)
    tmp = C._pass(img, plan.bx.numpy(), plan.kx.numpy(), 1)
    got = C._pass(tmp, plan.by.numpy(), plan.ky.numpy(), 0)
    assert np.array_equal(got, R.preprocess_u8(img, crop, resize))
    assert plan.row0 >= 0 and plan.row0 + plan.nrows <= shape[0]
    with pytest.raises(ValueError):
        ops.ClipResamplePlan(shape[0], shape[1], crop, "cpu", resize=crop - 1)


def test_default_plan_is_the_clip_plan():
    a = ops.ClipResamplePlan(40, 56, 28, "cpu")
    assert (a.top, a.left, a.resize) == ((28 - 28) // 2, (39 - 28) // 2, 28)
    bx, kx = C.coeffs(56, 39)
    assert np.array_equal(a.bx.numpy(), bx[a.left:a.left + 28]) and np.array_equal(a.kx.numpy(), kx[a.left:a.left + 28])


def test_bn_folding_against_unfolded_fp32():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 9, 7, generator=g)
    w = torch.randn(32, 64, 3, 3, generator=g) * 0.05
    gamma, beta = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    mean, var = torch.randn(32, generator=g), torch.rand(32, generator=g) + 0.5
    ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x.double(), w.double(), None, 2, 1), mean.double(),
                                         var.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    wf, bf = fold_bn(w, gamma, beta, mean, var)
    assert wf.dtype == torch.float32 and bf.dtype == torch.float32
    got = torch.nn.functional.conv2d(x.double(), wf.double(), bf.double(), 2, 1)
    # folding reorders fp32 roundings of the scale only: a few fp32 ulps of the outputs' scale
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    rf, rb = R.fold_bn(w, gamma, beta, mean, var)
    assert torch.equal(rf, wf) and torch.equal(rb, bf)


def test_state_dict_coverage_and_layouts():
    cfg = ResNetConfig.tiny()
    sd = make_resnet_state_dict(cfg, 0)
    specs = resnet_param_specs(cfg)
    assert set(sd) == {n for n, _ in specs}
    for key in ("conv1.weight", "bn1.running_var", "layer1.0.downsample.0.weight", "layer1.0.downsample.1.bias",
                "layer4.0.conv2.weight", "layer4.0.bn3.running_mean", "fc.weight", "fc.bias"):
        assert key in sd
    assert "layer1.1.conv1.weight" not in sd
    w = prepare_weights(sd, cfg)
    assert all(t.dtype == torch.float16 for t in w.values())
    assert tuple(w["stem.w"].shape) == (64, 192) and not w["stem.w"][:, 147:].any()
    assert tuple(w["layer1.0.w3"].shape) == (256, 64 + 64) and tuple(w["layer2.0.w3"].shape) == (512, 128 + 256)
    assert tuple(w["layer2.0.w2"].shape) == (128, 2, 3, 3, 64) and tuple(w["fc.w"].shape) == (40, 2048)
    # the concatenated bias is the fp32 sum of the two folded biases, rounded once
    _, b3 = fold_bn(sd["layer2.0.conv3.weight"], *(sd[f"layer2.0.bn3.{n}"] for n in
                                                    ("weight", "bias", "running_mean", "running_var")))
    _, bd = fold_bn(sd["layer2.0.downsample.0.weight"], *(sd[f"layer2.0.downsample.1.{n}"] for n in
                                                          ("weight", "bias", "running_mean", "running_var")))
    assert torch.equal(w["layer2.0.b3"], (b3 + bd).half())
    for key in ("layer3.0.bn2.running_var", "fc.bias", "layer1.0.downsample.0.weight"):
        short = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            prepare_weights(short, cfg)
    bad = dict(sd)
    bad["fc.weight"] = bad["fc.weight"][:, :-1]
    with pytest.raises(ValueError):
        prepare_weights(bad, cfg)
    full = ResNetConfig.resnet50()
    assert [sum(1 for b in full.blocks() if b[0].startswith(f"layer{i}.")) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    assert [b[4] for b in full.blocks() if b[5]] == [1, 2, 2, 2] and len(resnet_param_specs(full)) == 267


def test_config_validation():
    cfg = ResNetConfig.resnet50()
    assert (cfg.layers, cfg.widths, cfg.expansion, cfg.num_classes, cfg.features) == ((3, 4, 6, 3),
                                                                                      (64, 128, 256, 512), 4, 1000, 2048)
    assert ResNetConfig.tiny().layers == (1, 1, 1, 1) and ResNetConfig.tiny().num_classes == 40
    for size in (224, 64, 32):
        cfg.check_size(size)
    for size in (0, 16, 48, 225, 232):  # 48 -> 24 -> 12 -> 6 -> 3: stage 4 would see an odd extent
        with pytest.raises(ValueError):
            cfg.check_size(size)
    for kw in (dict(layers=(1, 1, 1)), dict(widths=(64, 128, 256, 500)), dict(num_classes=10), dict(layers=(1, 0, 1, 1))):
        with pytest.raises(ValueError):
            ResNetConfig(**kw)


def bit(table, g, c):
    return (int(table[g, c >> 5]) >> (c & 31)) & 1


def test_match_table_reference_rule():
    cats = ["tench", "English springer", "cassette player", "tape player", "garbage truck", "golf ball"] + \
           [f"filler{i}" for i in range(60)] + ["player piano"]
    labels = ["cassette player", "english springer", " golf ball ", "church", "garbage truck golf"]
    t = match_table(cats, labels)
    assert t.dtype == torch.int32 and tuple(t.shape) == (5, 3)
    rows = [[c for c in range(len(cats)) if bit(t, g, c)] for g in range(len(labels))]
    assert rows[0] == [2, 3, 66]   # "cassette" or "player": every class with either word, past word 1 of the table
    assert rows[1] == [1]          # through "springer" only: "English" != "english" (the reference's case quirk)
    assert rows[2] == [5]          # the label is stripped
    assert rows[3] == []
    assert rows[4] == [4, 5]       # multi-word label: any word of it
    assert match_table(cats, ["english"])[0].tolist() == [0, 0, 0]
    # the host rule in one line, as resnet_ref.hits applies it per image
    for g, lab in enumerate(labels):
        for c in range(len(cats)):
            assert R.hits([[c]], cats, [lab])[0] == bit(t, g, c)
    # bit 31 survives the int32 storage
    t31 = match_table([f"w{i}" for i in range(32)], ["w31"])
    assert t31.tolist() == [[-(1 << 31)]]


def test_scorer_needs_names_and_a_device():
    class FakeModel:
        config = ResNetConfig.tiny()
        device = torch.device("cpu")

    s = ObjectScorer(FakeModel(), None, size=64, resize=72)
    with pytest.raises(ValueError, match="categories"):
        s._table(["a"])
    with pytest.raises(ValueError):
        ObjectScorer(FakeModel(), ["a"] * 39, size=64, resize=72)
    with pytest.raises(ValueError):
        ObjectScorer(FakeModel(), None, size=72, resize=72)
    with pytest.raises(ValueError):
        ObjectScorer(FakeModel(), None, size=64, resize=48)


def test_write_results_format(tmp_path):
    import json
    p = tmp_path / "results.json"
    ObjectScorer.write_results(p, {"acc": 0.25, "hits": None, "topk": None})
    assert json.loads(p.read_text()) == {"acc": 0.25}


def test_reference_ranking_helpers():
    lg = np.array([[1.0, np.nan, 3.0, 3.0, -np.inf, np.inf, -0.0, 0.0]])
    assert R.topk_stable(lg, 8).tolist() == [[1, 5, 2, 3, 0, 6, 7, 4]]
    v, i = torch.topk(torch.tensor([1.0, float("nan"), 3.0, 2.5, -float("inf")]), 5)
    assert i.tolist() == R.topk_stable([[1.0, float("nan"), 3.0, 2.5, -float("inf")]], 5)[0].tolist()


def test_stem_rows_restatement_is_the_conv():
    """resnet_ref.stem_rows x the flattened [64, 3, 7, 7] weight is F.conv2d(stride 2, padding 3) of the fp16 pixels."""
    u8 = np.random.default_rng(5).integers(0, 256, (2, 15, 15, 3), dtype=np.uint8)
    a = torch.from_numpy(R.stem_rows(u8)).float()
    assert not a[:, 147:].any()
    w = torch.randn(8, 3, 7, 7, generator=torch.Generator().manual_seed(1))
    pix = R.pixel_values(u8).half().float()
    ref = R.to_rows(torch.nn.functional.conv2d(pix.double(), w.double(), None, 2, 3))
    got = a[:, :147].double() @ w.reshape(8, 147).double().t()
    assert torch.allclose(got, ref, rtol=0, atol=1e-9)


@pytest.mark.parametrize("seed", R.TOPK_SEEDS)
def test_topk_seeds_keep_enough_images(seed):
    """The committed seeds: the fp32 reference alone leaves at most 10 % of the images inside delta, both outcomes of
    the name match occur, and the fp16-storage mode agrees with it on every kept image."""
    case = R.topk_case(seed)
    n = len(case["images"])
    print(f"seed {seed}: delta {case['delta']:.3e}, min kept gap {case['gap'][case['keep']].min():.3e}, "
          f"excluded {n - int(case['keep'].sum())} of {n}, mode gap rel-L2 {R.rel_l2(case['ref16'], case['ref32']):.3e}")
    assert n - int(case["keep"].sum()) <= R.TOPK_MAX_EXCLUDED * n
    cats, labels = R.categories40(), R.topk_labels(n)
    t32, t16 = R.topk_stable(case["ref32"].numpy(), 5), R.topk_stable(case["ref16"].numpy(), 5)
    h = R.hits(t32, cats, labels)
    assert 0 < h.sum() < n
    for i in np.flatnonzero(case["keep"]):
        assert set(t32[i]) == set(t16[i])
