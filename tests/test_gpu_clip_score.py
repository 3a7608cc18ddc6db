"""The device CLIP scorer on the MI355X: csrc/clip_image.hip, the vision tower of sdmoe.clip and sdmoe.scoring.

Front end (quantise, Pillow-exact bicubic resample + centre crop, normalise + patchify): integer / correctly rounded
arithmetic, so every output is held EQUAL to tests/clip_score_ref.py (itself bit-exact against Pillow 12.2 and within
1 fp16 ulp of transformers' pixel_values, tests/test_clip_score_host.py). Output buffers sit inside poisoned
allocations that are checked afterwards.

Vision tower: against fp32 transformers CLIPModel on the same fp16-rounded weights, fed the device's own pixel values;
the bar is the text tower's (tests/test_gpu_clip.py): rel-L2 <= 1e-2 -- same layer types, same fp16 storage.
Measured on the MI355X, rel-L2 of hidden / pooled / image_embeds (width 128, head_dim 64, 2 layers, B = 3):
  S = 28, p = 4  (50 tokens, sdmoe_attention_short unmasked)   5.99e-4 / 6.09e-4 / 8.06e-4
  S = 56, p = 4  (197 tokens, sdmoe_attention, ragged Nq / Nk) 5.97e-4 / 6.09e-4 / 5.69e-4
  S = 28, p = 14 (5 tokens, K = 588 padded to 640)             6.80e-4 / 6.98e-4 / 7.45e-4

sdmoe_clip_scores: float64 on the same fp16 rows against torch float64, relative 1e-12 (a D <= 512 float64 dot
product in another order differs by at most D 2^-53 ~ 6e-14 relatively; sqrt and the division add 2^-52 each); the
accuracy count is an integer and EQUAL; two runs are bit-identical.

End to end (ClipScorer.score_removal on the committed seeds of clip_score_ref.ACC_SEEDS): every cosine within 2e-2 of
the fp32 oracle's -- to first order two unit vectors each off by the feature bar delta = 1e-2 move a cosine by at most
2 delta -- and, every pair being decided by more than 4e-2 under the oracle, average_acc EQUAL to the oracle's.
Measured: max |device - oracle| over the 18 cosines of a seed 1.6e-4 (seed 1) and 2.9e-4 (seed 26)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_score_ref as R  # noqa: E402
from sdmoe import ops  # noqa: E402
from sdmoe.clip import (CLIPModel, CLIPTextConfig, CLIPTextModel, CLIPVisionConfig, CLIPVisionModel,  # noqa: E402
                        SyntheticCLIPTokenizer, make_clip_state_dict, make_clip_vision_state_dict)
from sdmoe.scoring import ClipScorer  # noqa: E402

DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def rand_u8(b, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- quantise
def all_fp16_unit_values():
    """Every fp16 in [0, 1] -- all k/255 roundings with both neighbours and every x with x * 255 on a .5 tie -- plus
    values outside the range (the clamp)."""
    bits = np.arange(0, 0x3c01, dtype=np.uint16)
    v = bits.view(np.float16)
    return np.concatenate([v, np.array([-0.25, -0.0, 1.001, 1.5, 2.0], np.float16)])


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("W,offset", [(64, 32), (37, 32), (64, 33)])  # dword stores, ragged rows, unaligned output
def test_quantise_exact(dtype, W, offset):
    v = all_fp16_unit_values().astype(dtype)
    if dtype == np.float32:  # fp32 neighbours of k/255 and of the (m + .5)/255 ties
        k = (np.arange(0, 511, dtype=np.float64) / 510.0).astype(np.float32)
        v = np.concatenate([v, k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))])
    prod = v.astype(np.float32) * np.float32(255.0)
    # the data holds exact .5 ties: among fp16 inputs x * 255 is exact and only 0.5 -> 127.5 ties (255 is odd); the fp32
    # products round onto 256 more
    assert np.count_nonzero((prod - np.floor(prod)) == 0.5) >= (1 if dtype == np.float16 else 200)
    H = 5
    B = -(-v.size // (3 * H * W))
    x = np.resize(v, (B, 3, H, W))
    ref = R.quantise(x)
    flat = torch.full((ref.size + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    out = flat[offset:offset + ref.size].view(B, H, W, 3)
    ops.clip_quantise(torch.from_numpy(x).to(DEV), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    assert bool((flat[:offset] == 0xA5).all()) and bool((flat[offset + ref.size:] == 0xA5).all())


# ------------------------------------------------------------------------------------------- resample and crop
def device_preprocess(u8, S, patch):
    """ops.clip_preprocess into poisoned allocations -> (A operand, uint8 crop) as numpy, poison checked."""
    B = u8.shape[0]
    G2, kpad = (S // patch) ** 2, ops.clip_padded_k(patch)
    na, nu = B * G2 * kpad, B * S * S * 3
    fa = torch.full((na + 128,), 777.0, dtype=torch.float16, device=DEV)
    fu = torch.full((nu + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    a, o = fa[64:64 + na].view(B * G2, kpad), fu[64:64 + nu].view(B, S, S, 3)
    ops.clip_preprocess(torch.from_numpy(u8).to(DEV), S, patch, a_out=a, u8_out=o)
    torch.cuda.synchronize()
    assert bool((fa[:64] == 777.0).all()) and bool((fa[64 + na:] == 777.0).all())
    assert bool((fu[:64] == 0xA5).all()) and bool((fu[64 + nu:] == 0xA5).all())
    return a.cpu().numpy(), o.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(a.view(np.int16), b.view(np.int16))


@pytest.mark.parametrize("B,H,W,S", [(2, 64, 64, 28), (3, 40, 56, 28), (2, 96, 64, 28), (2, 17, 23, 28),
                                     (1, 28, 28, 28), (2, 512, 512, 224)])
def test_preprocess_u8_bit_exact(B, H, W, S):
    u8 = rand_u8(B, H, W, H + W)
    u8[-1] = np.where(u8[-1] > 127, 255, 0)  # a 0 / 255 image: bicubic overshoot drives clip8 both ways
    patch = 4 if S == 28 else 32
    a, o = device_preprocess(u8, S, patch)
    ref = np.stack([R.preprocess_u8(i, S) for i in u8])
    assert np.array_equal(o, ref)
    assert same_bits(a, R.patchify(R.normalise(ref), patch))


@pytest.mark.parametrize("patch,K,kpad", [(14, 588, 640), (4, 48, 64)])
def test_a_operand_bit_exact(patch, K, kpad):
    u8 = rand_u8(3, 40, 56, patch)
    lv = np.arange(256, dtype=np.uint8)  # every level in every channel reaches the normalise (28 x 28 > 256 pixels)
    a, _ = device_preprocess(u8, 28, patch)
    ref = R.a_operand(list(u8), 28, patch)
    assert a.shape == ref.shape == (3 * (28 // patch) ** 2, kpad) and same_bits(a, ref)
    assert not a[:, K:].view(np.int16).any()  # padding columns: +0.0 exactly
    ident = np.resize(lv, (1, 28, 28, 3))  # 28 x 28 -> 28 x 28 is the identity: levels pass straight through
    a2, o2 = device_preprocess(ident, 28, patch)
    assert np.array_equal(o2, ident) and same_bits(a2, R.patchify(R.normalise(ident), patch))


def scorer_for(vc, seed=3, tc=None):
    tc = tc or CLIPTextConfig.tiny(128, 2, 2, projection_dim=vc.projection_dim)
    sd = {**make_clip_state_dict(tc, seed), **make_clip_vision_state_dict(vc, seed)}
    model = CLIPModel.from_state_dict(sd, tc, vc, DEV)
    return ClipScorer(model, SyntheticCLIPTokenizer(pad_token_id=tc.pad_token_id), size=vc.image_size), sd, tc


def test_scorer_preprocess_batch_offsets_and_inputs():
    """A list of batches of different sizes and kinds (uint8 NHWC, fp16 / fp32 NCHW, a single 3-D image) lands in one
    A operand at the right batch offsets."""
    sc, _, _ = scorer_for(CLIPVisionConfig.tiny())
    u1, u2 = rand_u8(2, 40, 56, 1), rand_u8(1, 96, 64, 2)
    f3 = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    f4 = torch.rand(3, 17, 23, generator=torch.Generator().manual_seed(1)).half()
    imgs = [torch.from_numpy(u1).to(DEV), torch.from_numpy(u2).to(DEV), f3.to(DEV), f4.to(DEV)]
    ref_u8 = list(u1) + list(u2) + list(R.quantise(f3.numpy())) + list(R.quantise(f4[None].numpy()))
    got_u8 = sc.preprocess_u8(imgs).cpu().numpy()
    assert np.array_equal(got_u8, np.stack([R.preprocess_u8(i, 28) for i in ref_u8]))
    assert same_bits(sc.preprocess(imgs).cpu().numpy(), R.a_operand(ref_u8, 28, 4))


# ------------------------------------------------------------------------------------------------ vision tower
TOWERS = [("s28_p4_short", CLIPVisionConfig.tiny(128, 2, 2, patch=4, image=28)),     # 50 tokens: attention_short
          ("s56_p4_flash", CLIPVisionConfig.tiny(128, 2, 2, patch=4, image=56)),     # 197 tokens: ragged Nq / Nk
          ("s28_p14_pad", CLIPVisionConfig.tiny(128, 2, 2, patch=14, image=28))]     # K = 588 -> 640, 5 tokens


@pytest.mark.parametrize("name,vc", TOWERS, ids=[t[0] for t in TOWERS])
def test_vision_tower_vs_transformers(name, vc):
    sc, sd, tc = scorer_for(vc, seed=5)
    B, S, p, G = 3, vc.image_size, vc.patch_size, vc.grid
    a = sc.preprocess(torch.from_numpy(rand_u8(B, 80, 112, 9)).to(DEV))
    r = sc.model.vision_model.encode(a, hidden=True)
    torch.cuda.synchronize()
    # the device's own pixel values, un-patchified
    pv = a[:, :3 * p * p].float().cpu().view(B, G, G, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, S, S)
    m = R.hf_clip_model(tc, vc, R.h16(sd))
    with torch.no_grad():
        o = m.vision_model(pixel_values=pv.contiguous())
        emb = m.visual_projection(o.pooler_output)
    got = (rel_l2(r["hidden"], o.last_hidden_state.reshape(-1, vc.hidden_size)), rel_l2(r["pooled"], o.pooler_output),
           rel_l2(r["image_embeds"], emb))
    print(f"vision tower {name}: rel-L2 hidden {got[0]:.3e} pooled {got[1]:.3e} image_embeds {got[2]:.3e}")
    assert max(got) <= 1e-2, got
    assert torch.equal(sc.model.get_image_features(a), r["image_embeds"])


def test_text_features_vs_transformers():
    sc, sd, tc = scorer_for(CLIPVisionConfig.tiny(), seed=5)
    prompts = ["a photo of a cat", "", "The Starry Night, a painting by Vincent van Gogh"]
    t = sc.text_features(prompts)
    m = R.hf_clip_model(tc, sc.model.vision_model.config, R.h16(sd))
    ref = R.hf_text_features(m, sc.tokenizer(prompts).input_ids)
    assert rel_l2(t, ref) <= 2e-2  # the projected-output bar of tests/test_gpu_clip.py


def test_full_size_configs_build_and_run():
    """ViT-B/32 at full size, one image: shapes, finiteness, and the text config that pairs with it."""
    vc, tc = CLIPVisionConfig.vit_b32(), CLIPTextConfig.vit_b32()
    assert (vc.hidden_size, vc.num_hidden_layers, vc.num_attention_heads, vc.patch_size, vc.projection_dim) == \
        (768, 12, 12, 32, 512)
    l14 = CLIPVisionConfig.vit_l14()
    assert (l14.hidden_size, l14.num_hidden_layers, l14.num_attention_heads, l14.patch_size, l14.num_positions,
            l14.projection_dim) == (1024, 24, 16, 14, 257, 768)
    assert (tc.hidden_size, tc.num_attention_heads, tc.num_hidden_layers, tc.projection_dim) == (512, 8, 12, 512)
    vis = CLIPVisionModel.from_state_dict(make_clip_vision_state_dict(vc, 0), vc, DEV)
    a = torch.empty((49, ops.clip_padded_k(32)), dtype=torch.float16, device=DEV)
    ops.clip_preprocess(torch.from_numpy(rand_u8(1, 256, 320, 0)).to(DEV), 224, 32, a_out=a)
    f = vis.encode(a)["image_embeds"]
    assert f.shape == (1, 512) and bool(torch.isfinite(f).all())


# ------------------------------------------------------------------------------------------------------ scores
@functools.lru_cache(maxsize=None)
def score_rows(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    T, A, Rm = (torch.randn(n, D, generator=g).half() for _ in range(3))
    Rm.copy_((A.float() * 0.7 + Rm.float() * 0.5).half())
    if n > 4:
        A[3] = 0  # the eps clamp
        T[5 % n] = 0
    return T, A, Rm


@pytest.mark.parametrize("n,D", [(1, 64), (37, 64), (37, 512), (1, 512), (300, 64)])
@pytest.mark.parametrize("text", [True, False])
def test_clip_scores_vs_float64(n, D, text):
    T, A, Rm = score_rows(n, D, n + D)
    dev = [t.to(DEV) for t in (T, A, Rm)]
    if not text:
        dev[0] = None
    out = ops.clip_scores(*dev)
    out2 = ops.clip_scores(*dev)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)  # bit-identical from run to run
    out = out.cpu()
    cs = torch.nn.functional.cosine_similarity
    exp = [cs(T.double(), A.double()), cs(T.double(), Rm.double()), cs(A.double(), Rm.double())]
    if not text:
        exp[0] = exp[1] = torch.zeros(n, dtype=torch.float64)
    for j, e in enumerate(exp):
        got = out[j * n:(j + 1) * n]
        assert bool(((got - e).abs() <= 1e-12 * e.abs()).all()), j
    if n > 4:
        assert out[2 * n + 3] == 0.0 and (not text or (out[3] == 0.0 and out[n + 5 % n] == 0.0))
    si = out[2 * n:3 * n]
    assert abs(out[3 * n] - si.sum()) <= 1e-12 * si.abs().sum()
    assert abs(out[3 * n + 1] - (si * si).sum()) <= 1e-12 * (si * si).sum()
    assert out[3 * n + 2].item() == (int((out[:n] > out[n:2 * n]).sum()) if text else 0)


def test_clip_scores_strided_rows():
    T, A, Rm = score_rows(37, 64, 1)
    wide = torch.cat([T, A, Rm], 1).to(DEV)
    a = ops.clip_scores(wide[:, :64], wide[:, 64:128], wide[:, 128:])
    b = ops.clip_scores(T.to(DEV), A.to(DEV), Rm.to(DEV))
    assert torch.equal(a, b)


# -------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("seed", R.ACC_SEEDS)
def test_score_removal_end_to_end(seed, tmp_path):
    case = R.accuracy_case(seed)
    oracle = R.accuracy_oracle(case)
    tc, vc = case["text_cfg"], case["vision_cfg"]
    model = CLIPModel(CLIPTextModel.from_state_dict(case["sd"], tc, DEV),
                      CLIPVisionModel.from_state_dict(case["sd"], vc, DEV))
    sc = ClipScorer(model, SyntheticCLIPTokenizer(pad_token_id=tc.pad_token_id), size=vc.image_size)
    orig, removed = [i.to(DEV) for i in case["orig"]], [i.to(DEV) for i in case["removed"]]
    res = sc.score_removal(case["prompts"], orig, removed)
    for k in ("similarity_orig", "similarity_removed", "image_sim"):
        d = np.abs(res[k].numpy() - oracle[k])
        print(f"seed {seed} {k}: max |device - oracle| = {d.max():.3e}")
        assert res[k].dtype == torch.float64 and d.max() <= 2e-2, k
    assert res["average_acc"] == oracle["average_acc"]
    assert abs(res["average_clipscore"] - oracle["average_clipscore"]) <= 2e-2
    assert res["average_clipscore"] == pytest.approx(res["image_sim"].mean().item(), rel=1e-12)
    # art_removal.py:114-125 on the same pairs
    sim = sc.image_similarity(orig, removed)
    assert torch.equal(sim["sim"], res["image_sim"])
    assert sim["mean_sim"] == pytest.approx(np.mean(sim["sim"].numpy()), rel=1e-12)
    assert sim["std"] == pytest.approx(np.std(sim["sim"].numpy()), rel=1e-6, abs=1e-9)
    # results.txt in the reference's format
    path = tmp_path / "results.txt"
    sc.write_results(path, res)
    lines = path.read_text().splitlines()
    assert len(lines) == 2 and lines[0].startswith("Average CLIP score: ") and lines[1].startswith("Average accuracy: ")
    assert float(lines[0].split(": ")[1]) == res["average_clipscore"]
    assert float(lines[1].split(": ")[1]) == res["average_acc"]
