"""tests/clip_score_ref.py -- the CPU restatement the CLIP scorer's HIP kernels are held to -- pinned against Pillow,
transformers and torch, and the host-side tables of sdmoe.ops pinned against the restatement. No GPU.

Normalise: for all 256 levels x 3 channels the fp16 rounding of ((u8 * (1/255)) - mean) / std in fp32 is within 1 fp16
ulp of the fp16 rounding of CLIPImageProcessorPil's own pixel_values; measured (transformers 5.15, Pillow 12.2): 3 of
768 values differ, each by exactly 1 ulp (the processor folds rescale and normalise differently in fp32; 325 of 768
differ in the last fp32 bit)."""
import numpy as np
import pytest
import torch
from PIL import Image

import clip_score_ref as R
from sdmoe import ops

RESIZE_SHAPES = [(512, 512, 224, 224), (64, 64, 28, 28), (40, 56, 28, 39), (96, 64, 42, 28), (17, 23, 28, 37),
                 (28, 28, 28, 28)]  # (H, W, out H, out W)


def rand_u8(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def processor(size):
    from transformers import CLIPImageProcessorPil
    return CLIPImageProcessorPil(size={"shortest_edge": size}, crop_size={"height": size, "width": size})


@pytest.mark.parametrize("h,w,oh,ow", RESIZE_SHAPES)
def test_resize_bit_exact_vs_pillow(h, w, oh, ow):
    for seed, img in ((0, rand_u8(h, w, 0)), (1, np.where(rand_u8(h, w, 1) > 127, 255, 0).astype(np.uint8))):
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
        assert np.array_equal(R.resize_u8(img, oh, ow), ref), seed  # the 0 / 255 image drives clip8 both ways


@pytest.mark.parametrize("h,w", [(40, 56), (96, 64), (17, 23), (64, 64)])
def test_resize_crop_and_pixels_vs_processor(h, w):
    img = rand_u8(h, w, 2)
    pv = processor(28)(images=Image.fromarray(img), return_tensors="pt")["pixel_values"][0].numpy()
    oh, ow = R.resize_shape(h, w, 28)
    top, left = R.crop_offsets(oh, ow, 28)
    pil = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))[top:top + 28, left:left + 28]
    u8 = R.preprocess_u8(img, 28)
    assert np.array_equal(u8, pil)
    # one uint8 level is 1 / (255 * 0.276) = 1.4e-2 in pixel_values: 1e-5 pins every uint8, and allows the last fp32 bit
    assert np.abs(R.normalise(u8).transpose(2, 0, 1) - pv).max() <= 1e-5


def test_normalise_levels_within_one_fp16_ulp():
    lv = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16)[:, :, None], 3, axis=2)
    pv = processor(16)(images=Image.fromarray(lv), return_tensors="pt")["pixel_values"][0].numpy()
    a = pv.astype(np.float16).view(np.int16).astype(np.int64)
    b = R.normalise(lv).transpose(2, 0, 1).astype(np.float16).view(np.int16).astype(np.int64)
    assert np.all((a < 0) == (b < 0))  # same sign: the bit patterns then order as the values
    diff = np.abs(a - b)
    print(f"normalise: {int((diff != 0).sum())} of {diff.size} fp16 values differ, max {int(diff.max())} ulp")
    assert diff.max() <= 1


@pytest.mark.parametrize("n_in,n_out", [(512, 224), (64, 28), (56, 39), (96, 42), (17, 28), (23, 37), (28, 28),
                                        (640, 280), (7, 224)])
def test_coefficient_tables(n_in, n_out):
    bounds, kk = R.coeffs(n_in, n_out)
    for (lo, n), row in zip(bounds, kk):
        assert 0 <= lo and n >= 1 and lo + n <= n_in
        assert abs(int(row[:n].sum()) - (1 << 22)) <= n and not row[n:].any()
    # the package's host tables (what the kernels read) are the restatement's, whole and as a crop window
    b2, k2, ksize = ops.clip_resample_coeffs(n_in, n_out)
    assert ksize == kk.shape[1] and np.array_equal(np.array(b2), bounds) and np.array_equal(np.array(k2), kk)
    first, count = n_out // 3, max(1, n_out // 2)
    b3, k3, _ = ops.clip_resample_coeffs(n_in, n_out, first, count)
    assert np.array_equal(np.array(b3), bounds[first:first + count])
    assert np.array_equal(np.array(k3), kk[first:first + count])


@pytest.mark.parametrize("h,w,s", [(40, 56, 28), (96, 64, 28), (512, 512, 224), (17, 23, 28), (300, 200, 224)])
def test_resize_shape_matches_restatement(h, w, s):
    assert ops.clip_resize_shape(h, w, s) == R.resize_shape(h, w, s)


@pytest.mark.parametrize("patch,S", [(4, 28), (14, 28), (32, 64)])
def test_patchify_matches_conv2d(patch, S):
    g = torch.Generator().manual_seed(patch)
    pix = torch.randn(2, S, S, 3, generator=g).half().float()  # fp16-exact values: the cast in patchify is lossless
    w = torch.randn(24, 3, patch, patch, generator=g)
    a = R.patchify(pix.numpy(), patch)
    K, kpad = 3 * patch * patch, R.padded_k(patch)
    assert a.shape == (2 * (S // patch) ** 2, kpad) and kpad % 64 == 0 and kpad == ops.clip_padded_k(patch)
    assert not a[:, K:].any()
    wp = torch.zeros(24, kpad)
    wp[:, :K] = w.reshape(24, K)
    got = torch.from_numpy(a.astype(np.float32)).double() @ wp.double().t()
    ref = torch.nn.functional.conv2d(pix.permute(0, 3, 1, 2).double(), w.double(), stride=patch)
    ref = ref.flatten(2).transpose(1, 2).reshape(-1, 24)  # CLIPVisionEmbeddings' patch order
    assert torch.allclose(got, ref, rtol=0, atol=1e-9)


def test_score_arithmetic_matches_reference_lines():
    g = torch.Generator().manual_seed(3)
    T, A, Rm = (torch.randn(9, 64, generator=g).half() for _ in range(3))
    A[4] = 0  # a zero row: the eps clamp
    got = R.removal_scores(T.numpy(), A.numpy(), Rm.numpy())
    cs = torch.nn.functional.cosine_similarity
    clip, acc = 0, 0
    for i in range(9):  # artist_removal.py:196-207, one prompt per iteration, on float64 upcasts
        t, a, r = T[i:i + 1].double(), A[i:i + 1].double(), Rm[i:i + 1].double()
        so, sr, si = cs(t, a), cs(t, r), cs(a, r)
        acc += 1 if so > sr else 0
        clip += si.item()
        for k, v in (("similarity_orig", so), ("similarity_removed", sr), ("image_sim", si)):
            assert abs(got[k][i] - v.item()) <= 1e-14
    assert abs(got["average_clipscore"] - clip / 9) <= 1e-14 and got["average_acc"] == acc / 9
    assert got["image_sim"][4] == 0.0


@pytest.mark.parametrize("seed", R.ACC_SEEDS)
def test_accuracy_seeds_have_margin(seed):
    """Every pair of the GPU accuracy test's inputs is decided by more than ACC_MARGIN under the fp32 oracle, so the
    device's cosines (each within 2e-2) cannot flip a comparison. Seeds found by a search over 0..39."""
    o = R.accuracy_oracle(R.accuracy_case(seed))
    d = np.abs(o["similarity_orig"] - o["similarity_removed"])
    print(f"seed {seed}: margins {np.round(d, 4)}, accuracy {o['average_acc']}")
    assert len(d) == R.ACC_PAIRS and d.min() > R.ACC_MARGIN
    assert 0.0 < o["average_acc"] < 1.0  # both outcomes occur
