"""Torch-facing wrappers of the HIP kernels (libsdmoe_hip.so).

PyTorch is used only for device memory and streams: every op here validates its operands, hands raw device
pointers plus sizes to the C ABI (include/sdmoe.h) on the current HIP stream, and returns. Nothing falls back
to an eager or CPU implementation; a missing library or a non-GPU tensor raises.

Activations are 2-D row-major views [rows, channels] whose row stride may exceed the channel count (channel
slices of a concatenation buffer, fused QKV outputs); spatial tensors are NHWC flattened to [images*H*W, C].
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib

ACT_NONE, ACT_SILU, ACT_GELU, ACT_RELU, ACT_QUICK_GELU = 0, 1, 2, 3, 4
ACT_BY_NAME = {"none": ACT_NONE, "silu": ACT_SILU, "gelu": ACT_GELU, "relu": ACT_RELU, "quick_gelu": ACT_QUICK_GELU}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_dev = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream on the current device. The C accessors skip the Python Stream object
    and device-index resolution of torch.cuda.current_stream() (2.7 us -> ~0.3 us per launch; ~370 launches per
    U-Net evaluation)."""
    if _raw_stream is not None and _cur_dev is not None:
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rows(t: torch.Tensor, name: str):
    """(data_ptr, row stride) of a 2-D row-major fp16 device view."""
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a 2-D [rows, channels] view, got shape {tuple(t.shape)}")
    if not t.is_cuda:
        raise _lib.SdmoeError(f"{name}: tensor is not on a GPU device; sdmoe has no CPU path")
    if t.dtype != torch.float16:
        raise TypeError(f"{name}: expected float16, got {t.dtype}")
    if t.stride(1) != 1 and t.shape[1] > 1:
        raise ValueError(f"{name}: inner dimension must be contiguous")
    return t.data_ptr(), t.stride(0)


def _dev(t: torch.Tensor, name: str, dtype=torch.float16):
    if not t.is_cuda:
        raise _lib.SdmoeError(f"{name}: tensor is not on a GPU device; sdmoe has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return t.data_ptr()


_WS = {}
WS_FLOATS = 32 * 1024 * 1024  # split-K fp32 partial slabs (128 MB per device), reused stream-ordered


def _workspace(device):
    ws = _WS.get(device)
    if ws is None:
        ws = _WS[device] = torch.empty(WS_FLOATS, dtype=torch.float32, device=device)
    return ws


_GN_WS = {}


def _gn_workspace(device, floats):
    """GroupNorm partial-sum scratch (reused across calls; no allocation per call)."""
    ws = _GN_WS.get(device)
    if ws is None or ws.numel() < floats:
        ws = _GN_WS[device] = torch.zeros(max(floats, 1 << 16), dtype=torch.float32, device=device)
    return ws


def groupnorm_apply(x, nimg, HW, scale, shift, silu, out=None):
    """out = (SiLU?)(x * scale[img, c] + shift[img, c]) on [nimg*HW, C] views."""
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    C = x.shape[1]
    if out is None:
        out = torch.empty((x.shape[0], C), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    st = lib.sdmoe_groupnorm_apply(xp, ldx, nimg, HW, C, scale.data_ptr(), shift.data_ptr(), int(bool(silu)), op,
                                   ldy, _stream())
    _lib.check(st, "sdmoe_groupnorm_apply")
    return out


def mask_weight(w, bits, out=None):
    """Wanda-masked copy of w [N, K]: bit (n, k) of bits [N, K/8] set -> 0."""
    lib = _lib.load()
    N, K = w.shape
    if tuple(bits.shape) != (N, K // 8) or bits.dtype != torch.uint8:
        raise ValueError(f"mask bits {tuple(bits.shape)} {bits.dtype} do not match weight {tuple(w.shape)}")
    if out is None:
        out = torch.empty_like(w)
    st = lib.sdmoe_mask_weight(_dev(w, "w"), _dev(bits, "bits", torch.uint8), N, K, _dev(out, "out"), _stream())
    _lib.check(st, "sdmoe_mask_weight")
    return out


def wmask_kmajor(bits, perm=None, out=None):
    """Packed Wanda bits [N, K/8] (bit set = weight removed) -> the masked GEMM's K-step-major layout int64
    [K/64, N] (sdmoe_wmask_kmajor); perm (int32 [K], optional): column j of the result = column perm[j] of the
    mask (the routed FFN's expert-major neuron order). Made once per (t, l) mask, not per call."""
    lib = _lib.load()
    if bits.dim() != 2 or bits.dtype != torch.uint8:
        raise ValueError(f"wmask bits must be uint8 [N, K/8], got {bits.dtype} {tuple(bits.shape)}")
    N, K = bits.shape[0], bits.shape[1] * 8
    if out is None:
        out = torch.empty((K // 64, N), dtype=torch.int64, device=bits.device)
    pp = None
    if perm is not None:
        if perm.dtype != torch.int32 or perm.numel() != K:
            raise ValueError("perm must be int32 [K]")
        pp = _dev(perm, "perm", torch.int32)
    st = lib.sdmoe_wmask_kmajor(_dev(bits, "bits", torch.uint8), bits.stride(0), N, K, pp,
                                _dev(out, "out", torch.int64), _stream())
    _lib.check(st, "sdmoe_wmask_kmajor")
    return out


GEMM_PLAN_MODES = {"plain": 0, "keep": 4, "wmask": 5, "keepw": 6, "ln": 7, "geglu": 3, "geglu_ln": 8, "geglu_gt": 15}


def gemm_plan(mode, M, N, K, residual=False, act=ACT_NONE, workspace_floats=WS_FLOATS):
    """The launch sdmoe_linear / _linear_masked / _linear_ln would make for an M x N x K product, or sdmoe_linear_geglu
    ("geglu"; "geglu_gt" with the registered GELU table) / _geglu_ln for M x 2F x K (N = 2F): {"tile": (rows, cols),
    "waves": (along M, along N), "ksplit": k}. sdmoe_gemm_plan touches no device memory and launches nothing, but it
    asks the current device for its CU count, which starts the HIP runtime (256 CUs are assumed without a device)."""
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    _lib.check(lib.sdmoe_gemm_plan(GEMM_PLAN_MODES[mode], M, N, K, int(bool(residual)), act, workspace_floats, out),
               "sdmoe_gemm_plan")
    return {"tile": (out[0], out[1]), "waves": (out[2], out[3]), "ksplit": out[4]}


def conv_plan(nimg, H, W, Cin, Cout, *, Cin2=0, stride=1, upsample=False, residual=False, gn=False, act=ACT_NONE,
              workspace_floats=WS_FLOATS):
    """The launch sdmoe_conv3x3 (Cin2 > 0: sdmoe_conv3x3_sc; gn: sdmoe_conv3x3_gn, SdmoeError where it would refuse)
    would make (sdmoe_conv_plan; queries the CU count as gemm_plan does): {"halo", "tile", "waves", "bk", "stages",
    "ksplit", "kchunk", "kchunk2"}."""
    lib = _lib.load()
    out = (ctypes.c_int * 10)()
    _lib.check(lib.sdmoe_conv_plan(nimg, H, W, Cin, Cin2, Cout, stride, int(bool(upsample)), int(bool(residual)),
                                   int(bool(gn)), act, workspace_floats, out), "sdmoe_conv_plan")
    return {"halo": bool(out[0]), "tile": (out[1], out[2]), "waves": (out[3], out[4]), "bk": out[5], "stages": out[6],
            "ksplit": out[7], "kchunk": out[8], "kchunk2": out[9]}


def linear_masked(x, w, bias=None, *, keep=None, wmask=None, residual=None, out=None):
    """out = (x ⊙ keep) @ (w ⊙ (1 - M))^T + bias + residual (sdmoe_linear_masked): keep int64 [K/64, M] (A keep bits,
    sdmoe_moe_topk_keep), wmask int64 [K/64, N] (wmask_kmajor). Either may be None."""
    lib = _lib.load()
    xp, lda = _rows(x, "x")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear_masked: weight {tuple(w.shape)} does not match input K={K}")
    if keep is not None and (tuple(keep.shape) != (K // 64, M) or keep.dtype != torch.int64):
        raise ValueError(f"keep must be int64 [{K // 64}, {M}], got {keep.dtype} {tuple(keep.shape)}")
    if wmask is not None and (tuple(wmask.shape) != (K // 64, N) or wmask.dtype != torch.int64):
        raise ValueError(f"wmask must be int64 [{K // 64}, {N}], got {wmask.dtype} {tuple(wmask.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    op, ldc = _rows(out, "out")
    rp, ldr = (None, 0) if residual is None else _rows(residual, "residual")
    ws = _workspace(x.device)
    st = lib.sdmoe_linear_masked(xp, lda, None if keep is None else _dev(keep, "keep", torch.int64), _dev(w, "w"),
                                 w.stride(0), None if wmask is None else _dev(wmask, "wmask", torch.int64),
                                 _ptr(bias), rp, ldr, op, ldc, M, N, K, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "sdmoe_linear_masked")
    return out


def gemm_plan_sets(M, N, K, rows_per_img, *, keep=False, residual=False, workspace_floats=WS_FLOATS):
    """The launch sdmoe_linear_masked_sets would make (sdmoe_gemm_plan_sets; queries the CU count as gemm_plan does):
    the same dict as gemm_plan, its tile rows dividing rows_per_img. SdmoeError where the launch would refuse
    (rows_per_img % 64 != 0 and the shape's own tile straddles images): linear_masked_sets then runs per image run."""
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    _lib.check(lib.sdmoe_gemm_plan_sets(int(bool(keep)), M, N, K, rows_per_img, int(bool(residual)), workspace_floats,
                                        out), "sdmoe_gemm_plan_sets")
    return {"tile": (out[0], out[1]), "waves": (out[2], out[3]), "ksplit": out[4]}


def wmask_union_sets(masks, select, out=None):
    """out[s] = OR of masks[c] over the concepts c with bit c of select[s] set (sdmoe_wmask_union_sets): masks int64
    [nconcepts <= 32, ...] (any trailing shape, e.g. wmask_kmajor's [K/64, N]), select int32 [nsets] (bit patterns of
    uint32 words); returns int64 [nsets, ...]. select[s] == 0 gives the all-zero (unmasked) set."""
    lib = _lib.load()
    if masks.dim() < 2 or masks.dtype != torch.int64:
        raise ValueError(f"masks must be int64 [nconcepts, ...], got {masks.dtype} {tuple(masks.shape)}")
    if masks.shape[0] > 32:
        raise ValueError(f"at most 32 concepts, got {masks.shape[0]}")
    if select.dim() != 1 or select.dtype != torch.int32:
        raise ValueError(f"select must be int32 [nsets], got {select.dtype} {tuple(select.shape)}")
    nc, nsets = masks.shape[0], select.shape[0]
    words = masks[0].numel()
    if out is None:
        out = torch.empty((nsets,) + tuple(masks.shape[1:]), dtype=torch.int64, device=masks.device)
    elif out.dtype != torch.int64 or out.numel() != nsets * words:
        raise ValueError(f"out must be int64 with {nsets * words} words, got {out.dtype} {tuple(out.shape)}")
    st = lib.sdmoe_wmask_union_sets(_dev(masks, "masks", torch.int64), words, nc, _dev(select, "select", torch.int32),
                                    nsets, words, _dev(out, "out", torch.int64), _stream())
    _lib.check(st, "sdmoe_wmask_union_sets")
    return out


def image_set_runs(image_set):
    """Maximal runs of consecutive images sharing a set: [(first image, one past the last, set id)]."""
    runs = []
    for i, s in enumerate(image_set):
        if runs and runs[-1][2] == s:
            runs[-1] = (runs[-1][0], i + 1, s)
        else:
            runs.append((i, i + 1, s))
    return runs


def linear_masked_sets(x, w, bias=None, *, wmasks, image_set, rows_per_img, keep=None, residual=None, out=None,
                       image_set_dev=None):
    """out[m] = (x[m] ⊙ keep[m]) @ (w ⊙ (1 - wmasks[image_set[m // rows_per_img]]))^T + bias + residual[m]
    (sdmoe_linear_masked_sets): linear_masked with one Wanda mask per image. wmasks int64 [nsets, K/64, N]
    (wmask_union_sets / stacked wmask_kmajor), image_set the set id of every image: a host sequence of ints (checked
    against nsets here, uploaded per call unless image_set_dev, its int32 device copy, comes with it) or an int32 device
    tensor the caller has already checked.
    Where gemm_plan_sets refuses the shape (rows_per_img % 64 != 0: latents under 8x8) the call runs linear_masked
    once per maximal run of consecutive images sharing a set, on row slices of x / residual / out and a contiguous
    copy of the run's keep columns; that path needs the host form of image_set."""
    lib = _lib.load()
    xp, lda = _rows(x, "x")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear_masked_sets: weight {tuple(w.shape)} does not match input K={K}")
    if rows_per_img <= 0 or M % rows_per_img:
        raise ValueError(f"linear_masked_sets: {M} rows are not whole images of {rows_per_img}")
    nimg = M // rows_per_img
    if wmasks.dim() != 3 or tuple(wmasks.shape[1:]) != (K // 64, N) or wmasks.dtype != torch.int64:
        raise ValueError(f"wmasks must be int64 [nsets, {K // 64}, {N}], got {wmasks.dtype} {tuple(wmasks.shape)}")
    nsets = wmasks.shape[0]
    if keep is not None and (tuple(keep.shape) != (K // 64, M) or keep.dtype != torch.int64):
        raise ValueError(f"keep must be int64 [{K // 64}, {M}], got {keep.dtype} {tuple(keep.shape)}")
    host_ids = None
    if not isinstance(image_set, torch.Tensor):
        host_ids = [int(s) for s in image_set]
        if len(host_ids) != nimg or any(s < 0 or s >= nsets for s in host_ids):
            raise ValueError(f"image_set must hold {nimg} set ids in [0, {nsets}), got {host_ids}")
    elif image_set.dtype != torch.int32 or tuple(image_set.shape) != (nimg,):
        raise ValueError(f"image_set must be int32 [{nimg}], got {image_set.dtype} {tuple(image_set.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    op, ldc = _rows(out, "out")
    rp, ldr = (None, 0) if residual is None else _rows(residual, "residual")
    plan = (ctypes.c_int * 5)()
    st = lib.sdmoe_gemm_plan_sets(int(keep is not None), M, N, K, rows_per_img, int(residual is not None), WS_FLOATS,
                                  plan)
    if st == -3:  # a tile would straddle two images: one launch per run of images on one set
        if host_ids is None:
            raise _lib.SdmoeError(f"linear_masked_sets: rows_per_img = {rows_per_img} runs per image run, which needs "
                                  "image_set as a host sequence")
        for i0, i1, s in image_set_runs(host_ids):
            r0, r1 = i0 * rows_per_img, i1 * rows_per_img
            linear_masked(x[r0:r1], w, bias, keep=None if keep is None else keep[:, r0:r1].contiguous(),
                          wmask=wmasks[s], residual=None if residual is None else residual[r0:r1], out=out[r0:r1])
        return out
    _lib.check(st, "sdmoe_gemm_plan_sets")
    if host_ids is None:
        ids = image_set
    elif image_set_dev is not None:
        ids = image_set_dev
        if ids.dtype != torch.int32 or tuple(ids.shape) != (nimg,):
            raise ValueError(f"image_set_dev must be int32 [{nimg}], got {ids.dtype} {tuple(ids.shape)}")
    else:
        ids = torch.tensor(host_ids, dtype=torch.int32, device=x.device)
    ws = _workspace(x.device)
    st = lib.sdmoe_linear_masked_sets(xp, lda, None if keep is None else _dev(keep, "keep", torch.int64), _dev(w, "w"),
                                      w.stride(0), _dev(wmasks, "wmasks", torch.int64), wmasks.stride(0),
                                      _dev(ids, "image_set", torch.int32), nsets, rows_per_img, _ptr(bias), rp, ldr,
                                      op, ldc, M, N, K, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "sdmoe_linear_masked_sets")
    return out


def linear(x, w, bias=None, *, out=None, residual=None, act=ACT_NONE, coladd=None, coladd_bstride=0,
           rows_per_batch=0, gn=None, wmask=None, wmask_bits=None):
    """out = act(GN?(x) @ w.T + bias + coladd) + residual.  w: [N, K] fp16 (nn.Linear layout).
    gn = (scale, shift, silu): per-(image, channel) GroupNorm apply on x first (rows_per_batch rows/image).
    wmask: Wanda mask in the GEMM's layout (wmask_kmajor) applied to the W fragments in the GEMM
    (remove_wanda_neurons_fast.py:69-83); wmask_bits: the same mask packed [N, K/8], converted on this call."""
    lib = _lib.load()
    if gn is not None:
        x = groupnorm_apply(x, x.shape[0] // rows_per_batch, rows_per_batch, gn[0], gn[1], gn[2])
    if wmask_bits is not None:
        if tuple(wmask_bits.shape) != (w.shape[0], w.shape[1] // 8):
            raise ValueError(f"mask bits {tuple(wmask_bits.shape)} do not match weight {tuple(w.shape)}")
        wmask = wmask_kmajor(wmask_bits)
    if wmask is not None:
        if act != ACT_NONE or coladd is not None:
            raise ValueError("linear: a Wanda weight mask combines with bias/residual only")
        return linear_masked(x, w, bias, wmask=wmask, residual=residual, out=out)
    xp, lda = _rows(x, "x")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear: weight {tuple(w.shape)} does not match input K={K}")
    wp = _dev(w, "w")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    op, ldc = _rows(out, "out")
    rp, ldr = (None, 0) if residual is None else _rows(residual, "residual")
    ws = _workspace(x.device)
    st = lib.sdmoe_linear(xp, lda, wp, w.stride(0), _ptr(bias), _ptr(coladd), coladd_bstride, rows_per_batch,
                          rp, ldr, op, ldc, M, N, K, act, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "sdmoe_linear")
    return out


def conv_weight(w):
    """Conv weight in the kernel's layout [Cout, Cin/64, 3, 3, 64] from [Cout, 3, 3, Cin] (taps-last NHWC filter)
    or a torch [Cout, Cin, 3, 3] filter (pass nchw=True-shaped tensors through conv_weight_from_torch). K runs over
    (64-channel slice, tap, channel): the 9 taps of one slice are consecutive K-steps of the implicit GEMM."""
    Cout, kh, kw, Cin = w.shape
    if (kh, kw) != (3, 3) or Cin % 64:
        raise ValueError(f"conv_weight: expected [Cout, 3, 3, Cin] with Cin % 64 == 0, got {tuple(w.shape)}")
    return w.reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).reshape(Cout, Cin // 64, 3, 3, 64).contiguous()


def conv_weight_from_torch(w):
    """torch.nn.Conv2d weight [Cout, Cin, 3, 3] -> conv_weight layout."""
    return conv_weight(w.permute(0, 2, 3, 1))


def conv_weight_with_shortcut(w, w_sc):
    """[Cout, 9*Cin + Cin2]: the conv3x3 weight (conv_weight layout) with a 1x1 shortcut's [Cout, Cin2] columns
    appended — the operand of conv3x3(..., shortcut=x2) (sdmoe_conv3x3_sc)."""
    return torch.cat([w.reshape(w.shape[0], -1), w_sc.reshape(w.shape[0], -1)], 1).contiguous()


def conv3x3(x, nimg, H, W, w, bias=None, *, stride=1, upsample=False, out=None, residual=None, act=ACT_NONE,
            coladd=None, coladd_bstride=0, gn=None, shortcut=None):
    """3x3 conv (pad 1) on NHWC x viewed as [nimg*H*W, Cin]; w: [Cout, Cin/64, 3, 3, 64] fp16 (conv_weight).
    gn = (scale, shift, silu): GroupNorm(+SiLU) applied to x once (one read + write of x) before the conv.
    shortcut = x2 [nimg*H*W, Cin2]: a 1x1 projection of x2 folded in as extra K-steps (stride 1, no residual);
    w is then conv_weight_with_shortcut(...) [Cout, 9*Cin + Cin2]."""
    lib = _lib.load()
    if gn is not None:
        if stride == 1 and not upsample and act == ACT_NONE and conv_gn_fusable(H, W, x.shape[1], w.shape[0]):
            y = _conv3x3_gn(lib, x, nimg, H, W, w, bias, out, residual, coladd, coladd_bstride, gn, shortcut)
            if y is not None:
                return y
        x = groupnorm_apply(x, nimg, H * W, gn[0], gn[1], gn[2])
    xp, ldx = _rows(x, "x")
    Cin = x.shape[1]
    Cout = w.shape[0]
    if shortcut is not None:
        x2p, ldx2 = _rows(shortcut, "shortcut")
        Cin2 = shortcut.shape[1]
        if w.dim() != 2 or w.shape[1] != 9 * Cin + Cin2 or Cin % 64 or Cin2 % 64:
            raise ValueError(f"conv3x3: weight {tuple(w.shape)} is not [Cout, 9*{Cin} + {Cin2}] "
                             "(ops.conv_weight_with_shortcut)")
        if stride != 1 or upsample or residual is not None or shortcut.shape[0] != x.shape[0]:
            raise ValueError("conv3x3: a folded shortcut needs stride 1, no upsample, no residual, same rows")
        if x.shape[0] != nimg * H * W:
            raise ValueError("conv3x3: rows != nimg*H*W")
        if out is None:
            out = torch.empty((nimg * H * W, Cout), dtype=torch.float16, device=x.device)
        op, ldy = _rows(out, "out")
        return conv3x3_launch(xp, ldx, nimg, H, W, Cin, w, bias, coladd, coladd_bstride, None, 0, out, op, ldy, Cout,
                              1, False, act, sc=(x2p, ldx2, Cin2))
    if w.dim() != 5 or tuple(w.shape[1:]) != (Cin // 64, 3, 3, 64) or Cin % 64:
        raise ValueError(f"conv3x3: weight {tuple(w.shape)} is not the [Cout, Cin/64, 3, 3, 64] layout for "
                         f"Cin={Cin} (ops.conv_weight)")
    if x.shape[0] != nimg * H * W:
        raise ValueError("conv3x3: rows != nimg*H*W")
    if upsample:
        OH, OW = 2 * H, 2 * W
    else:
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((nimg * OH * OW, Cout), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    rp, ldr = (None, 0) if residual is None else _rows(residual, "residual")
    return conv3x3_launch(xp, ldx, nimg, H, W, Cin, w, bias, coladd, coladd_bstride, rp, ldr, out, op, ldy, Cout,
                          stride, upsample, act)


FUSED_GN = os.environ.get("SDMOE_FUSED_GN", "1") != "0"  # GroupNorm(+SiLU) inside the halo conv (0: apply pass)


def conv_gn_fusable(H, W, Cin, Cout):
    """Shapes whose conv applies a GroupNorm in the kernel (sdmoe_conv3x3_gn: the 64-wide halo tiles)."""
    return (FUSED_GN and W == 64 and (H * W) % 256 == 0 and Cin <= 1280 and Cin % 64 == 0 and Cout % 320 == 0
            and _lib.has(_lib.load(), "sdmoe_conv3x3_gn"))


def _conv3x3_gn(lib, x, nimg, H, W, w, bias, out, residual, coladd, coladd_bstride, gn, shortcut):
    """conv3x3(act(GroupNorm(x))) with the norm applied to the staged input inside the conv; None if unsupported."""
    xp, ldx = _rows(x, "x")
    Cin, Cout = x.shape[1], w.shape[0]
    if x.shape[0] != nimg * H * W:
        raise ValueError("conv3x3: rows != nimg*H*W")
    x2p, ldx2, Cin2 = None, 0, 0
    if shortcut is not None:
        x2p, ldx2 = _rows(shortcut, "shortcut")
        Cin2 = shortcut.shape[1]
        if w.dim() != 2 or w.shape[1] != 9 * Cin + Cin2 or residual is not None:
            raise ValueError(f"conv3x3: weight {tuple(w.shape)} is not [Cout, 9*{Cin} + {Cin2}] or a residual was given")
    elif w.dim() != 5 or tuple(w.shape[1:]) != (Cin // 64, 3, 3, 64):
        raise ValueError(f"conv3x3: weight {tuple(w.shape)} is not the [Cout, Cin/64, 3, 3, 64] layout for Cin={Cin}")
    sc, sh, silu = gn
    if tuple(sc.shape) != (nimg, Cin) or sc.dtype != torch.float32 or tuple(sh.shape) != (nimg, Cin):
        raise ValueError("conv3x3: gn scale / shift must be fp32 [nimg, Cin]")
    if out is None:
        out = torch.empty((nimg * H * W, Cout), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    rp, ldr = (None, 0) if residual is None else _rows(residual, "residual")
    return conv3x3_gn_launch(xp, ldx, nimg, H, W, Cin, w, bias, coladd, coladd_bstride, rp, ldr, out, op, ldy, Cout,
                             (sc, sh, silu), sc=(x2p, ldx2, Cin2) if shortcut is not None else None)


def conv3x3_gn_launch(xp, ldx, nimg, H, W, Cin, w, bias, coladd, coladd_bstride, rp, ldr, out, op, ldy, Cout, gn,
                      sc=None):
    """The sdmoe_conv3x3_gn launch alone (argument order of conv3x3_launch: bench.py times both families); None when
    the shape is not one the kernel normalises itself."""
    lib = _lib.load()
    ws = _workspace(out.device)
    x2p, ldx2, Cin2 = sc if sc is not None else (None, 0, 0)
    st = lib.sdmoe_conv3x3_gn(xp, ldx, nimg, H, W, Cin, gn[0].data_ptr(), gn[1].data_ptr(), int(bool(gn[2])),
                              _dev(w, "w"), _ptr(bias), _ptr(coladd), coladd_bstride, rp, ldr, x2p, ldx2, Cin2, op, ldy,
                              Cout, ws.data_ptr(), ws.numel(), _stream())
    if st == -3:
        return None
    _lib.check(st, "sdmoe_conv3x3_gn")
    return out


def conv3x3_launch(xp, ldx, nimg, H, W, Cin, w, bias, coladd, coladd_bstride, rp, ldr, out, op, ldy, Cout, stride,
                   upsample, act, sc=None):
    """The sdmoe_conv3x3 launch alone (bench.py times exactly this with HIP events); sc = (x2 ptr, ldx2, Cin2):
    sdmoe_conv3x3_sc with the folded 1x1 shortcut."""
    lib = _lib.load()
    ws = _workspace(out.device)
    if sc is not None:
        st = lib.sdmoe_conv3x3_sc(xp, ldx, nimg, H, W, Cin, _dev(w, "w"), _ptr(bias), _ptr(coladd), coladd_bstride,
                                  sc[0], sc[1], sc[2], op, ldy, Cout, act, ws.data_ptr(), ws.numel(), _stream())
        _lib.check(st, "sdmoe_conv3x3_sc")
        return out
    st = lib.sdmoe_conv3x3(xp, ldx, nimg, H, W, Cin, _dev(w, "w"), _ptr(bias), _ptr(coladd), coladd_bstride, rp, ldr,
                           op, ldy, Cout, stride, int(bool(upsample)), act, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "sdmoe_conv3x3")
    return out


# Nearest-2x upsample + 3x3 conv as four 2x2 convs on the low-resolution image (sdmoe_conv_up2x):
# [phase row or column p][2x2 row or column a] -> the 3x3 taps that land on that input pixel
_UP2X_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))


def up2x_collapse(w):
    """[Cout, 3, 3, Cin] -> [4, Cout, 2, 2, Cin] in w's dtype: phase 2 py + px of a nearest-2x upsampled image reads
    a 2x2 input neighbourhood, and the taps that land on one input pixel are summed (_UP2X_TAPS, rows and columns
    alike). Exact in exact arithmetic: output pixel (2r + py, 2q + px) = sum over (a, c) of
    result[2 py + px, :, a, c] . x[r + py + a - 1, q + px + c - 1]."""
    Cout, kh, kw, Cin = w.shape
    if (kh, kw) != (3, 3):
        raise ValueError(f"up2x_collapse: expected [Cout, 3, 3, Cin], got {tuple(w.shape)}")
    out = w.new_empty((4, Cout, 2, 2, Cin))
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for c in range(2):
                    taps = [w[:, i, j] for i in _UP2X_TAPS[py][a] for j in _UP2X_TAPS[px][c]]
                    out[2 * py + px, :, a, c] = sum(taps[1:], taps[0])
    return out


def conv_up2x_weight(w):
    """The operand of conv_up2x from a [Cout, 3, 3, Cin] filter (taps-last, as conv_weight takes): fp16
    [4, Cout, Cin/64, 2, 2, 64] -- phase, then conv_weight's K order (64-channel slice, tap, channel). Summed in fp32,
    rounded to fp16 once. Made once per weight version (16/9 of the filter's bytes), not per call."""
    Cout, _, _, Cin = w.shape
    if Cin % 64:
        raise ValueError(f"conv_up2x_weight: Cin % 64 != 0 in {tuple(w.shape)}")
    wc = up2x_collapse(w.float()).half()
    return wc.reshape(4, Cout, 4, Cin // 64, 64).permute(0, 1, 3, 2, 4).reshape(4, Cout, Cin // 64, 2, 2, 64).contiguous()


def conv_up2x_plan(nimg, H, W, Cin, Cout, workspace_floats=WS_FLOATS):
    """The launch sdmoe_conv_up2x would make for nimg H x W x Cin images: {"tile", "waves", "stages", "ksplit",
    "kchunk"}, or None where it refuses the shape (or the loaded library is an SDMOE_AB=1 build without it)."""
    lib = _lib.load()
    if not _lib.has(lib, "sdmoe_conv_up2x_plan"):
        return None
    out = (ctypes.c_int * 7)()
    st = lib.sdmoe_conv_up2x_plan(nimg, H, W, Cin, Cout, workspace_floats, out)
    if st in (-2, -3):
        return None
    _lib.check(st, "sdmoe_conv_up2x_plan")
    return {"tile": (out[0], out[1]), "waves": (out[2], out[3]), "stages": out[4], "ksplit": out[5], "kchunk": out[6]}


def conv_up2x(x, nimg, H, W, wc, bias=None, out=None, *, fallback=None):
    """conv3x3(nearest-2x upsample of x) on NHWC x viewed as [nimg*H*W, Cin] -> [nimg*2H*2W, Cout], from the
    phase-collapsed weight wc (conv_up2x_weight). Where the kernel refuses the shape (-3: Cout no multiple of the
    chosen tile's columns) the conv runs as conv3x3(..., upsample=True) on `fallback`, the filter in conv_weight's
    layout; without one that is an error."""
    xp, ldx = _rows(x, "x")
    Cin = x.shape[1]
    if wc.dim() != 6 or wc.shape[0] != 4 or tuple(wc.shape[2:]) != (Cin // 64, 2, 2, 64) or Cin % 64:
        raise ValueError(f"conv_up2x: weight {tuple(wc.shape)} is not the [4, Cout, Cin/64, 2, 2, 64] layout for "
                         f"Cin={Cin} (ops.conv_up2x_weight)")
    Cout = wc.shape[1]
    if x.shape[0] != nimg * H * W:
        raise ValueError("conv_up2x: rows != nimg*H*W")
    if out is None:
        out = torch.empty((nimg * 4 * H * W, Cout), dtype=torch.float16, device=x.device)
    elif out.shape[0] != nimg * 4 * H * W or out.shape[1] != Cout:
        raise ValueError(f"conv_up2x: out {tuple(out.shape)} is not [{nimg * 4 * H * W}, {Cout}]")
    op, ldy = _rows(out, "out")
    if conv_up2x_launch(xp, ldx, nimg, H, W, Cin, wc, bias, out, op, ldy, Cout) is not None:
        return out
    if fallback is None:
        raise _lib.SdmoeError(f"sdmoe_conv_up2x refuses Cout={Cout} at {nimg} x {H} x {W} and no fallback filter was given")
    return conv3x3(x, nimg, H, W, fallback, bias, upsample=True, out=out)


def conv_up2x_launch(xp, ldx, nimg, H, W, Cin, wc, bias, out, op, ldy, Cout):
    """The sdmoe_conv_up2x launch alone; None when the kernel refuses the shape (-3). Not a conv3x3_launch: that
    function's callers count 9-tap FLOPs per launch, and this kernel executes 4/9 of them."""
    lib = _lib.load()
    ws = _workspace(out.device)
    st = lib.sdmoe_conv_up2x(xp, ldx, nimg, H, W, Cin, _dev(wc, "wc"), _ptr(bias), op, ldy, Cout, ws.data_ptr(),
                             ws.numel(), _stream())
    if st == -3:
        return None
    _lib.check(st, "sdmoe_conv_up2x")
    return out


def groupnorm_stats(x, nimg, HW, gamma, beta, eps, groups=32):
    """Per-(image, channel) fp32 (scale, shift) of GroupNorm(groups) over x viewed as [nimg*HW, C]."""
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    C = x.shape[1]
    scale = torch.empty((nimg, C), dtype=torch.float32, device=x.device)
    shift = torch.empty((nimg, C), dtype=torch.float32, device=x.device)
    ws = _gn_workspace(x.device, nimg * groups * 64 * 2)
    st = lib.sdmoe_groupnorm_stats(xp, ldx, nimg, HW, C, groups, _dev(gamma, "gamma"), _dev(beta, "beta"),
                                   float(eps), scale.data_ptr(), shift.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream())
    _lib.check(st, "sdmoe_groupnorm_stats")
    return scale, shift


def groupnorm(x, nimg, HW, gamma, beta, eps, groups=32, silu=False, out=None):
    """act(GroupNorm(x)) as a new [nimg*HW, C] fp16 tensor (sdmoe_groupnorm: statistics + apply)."""
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    C = x.shape[1]
    scale = torch.empty((nimg, C), dtype=torch.float32, device=x.device)
    shift = torch.empty((nimg, C), dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty((x.shape[0], C), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    ws = _gn_workspace(x.device, nimg * groups * 64 * 2)
    st = lib.sdmoe_groupnorm(xp, ldx, nimg, HW, C, groups, _dev(gamma, "gamma"), _dev(beta, "beta"), float(eps),
                             int(bool(silu)), op, ldy, scale.data_ptr(), shift.data_ptr(), ws.data_ptr(), ws.numel(),
                             _stream())
    _lib.check(st, "sdmoe_groupnorm")
    return out


def gn_fold(w, bias, scale, shift):
    """Per-image GroupNorm-folded weights of a linear (sdmoe_gn_fold): Wf [nimg, N, K] fp16 and colbias [nimg, N]
    fp32 with x . Wf[i]^T + colbias[i] = GN(x) . w^T + bias on the rows of image i (scale / shift from
    groupnorm_stats). Wf[i] = fp16(w * scale[i]) and colbias[i] = bias + Wf[i] . (shift[i] / scale[i]), the bias taken
    from the rounded weights (w * shift where |scale| < 2^-14, e.g. gamma == 0): the rounding of Wf then multiplies x + shift / scale, an
    activation centred on its group, and the fold holds the accuracy of groupnorm + linear at any group offset."""
    lib = _lib.load()
    N, K = w.shape
    nimg = scale.shape[0]
    if tuple(scale.shape) != (nimg, K) or tuple(shift.shape) != (nimg, K):
        raise ValueError(f"gn_fold: scale/shift {tuple(scale.shape)} do not match weight {tuple(w.shape)}")
    wf = torch.empty((nimg, N, K), dtype=torch.float16, device=w.device)
    cb = torch.empty((nimg, N), dtype=torch.float32, device=w.device)
    st = lib.sdmoe_gn_fold(_dev(w, "w"), w.stride(0), N, K, _ptr(bias), _dev(scale, "scale", torch.float32),
                           _dev(shift, "shift", torch.float32), nimg, wf.data_ptr(), cb.data_ptr(), _stream())
    _lib.check(st, "sdmoe_gn_fold")
    return wf, cb


def linear_per_image(x, wf, colbias, rows_per_batch, *, residual=None, out=None):
    """out[m] = x[m] . wf[m // rows_per_batch]^T + colbias[m // rows_per_batch] (+ residual): the GEMM behind a folded
    GroupNorm (sdmoe_linear_per_image; rows_per_batch % 256 == 0)."""
    lib = _lib.load()
    xp, lda = _rows(x, "x")
    M, K = x.shape
    nimg, N, Kw = wf.shape
    if Kw != K or M != nimg * rows_per_batch or tuple(colbias.shape) != (nimg, N):
        raise ValueError(f"linear_per_image: x {tuple(x.shape)}, wf {tuple(wf.shape)}, colbias "
                         f"{tuple(colbias.shape)}, rows_per_batch {rows_per_batch}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    op, ldc = _rows(out, "out")
    rp, ldr = (None, 0) if residual is None else _rows(residual, "residual")
    ws = _workspace(x.device)
    st = lib.sdmoe_linear_per_image(xp, lda, _dev(wf, "wf"), wf.stride(1), wf.stride(0),
                                    _dev(colbias, "colbias", torch.float32), colbias.stride(0), rows_per_batch, rp,
                                    ldr, op, ldc, M, N, K, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "sdmoe_linear_per_image")
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    M, C = x.shape
    if out is None:
        out = torch.empty((M, C), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    st = lib.sdmoe_layernorm(xp, ldx, op, ldy, M, C, _dev(gamma, "gamma"), _dev(beta, "beta"), float(eps), _stream())
    _lib.check(st, "sdmoe_layernorm")
    return out


class LNFold:
    """LayerNorm(gamma, beta) folded into a following linear W [N, K] (+ bias): wf = fp16(W diag(gamma)), bias_f =
    bias + W beta and wsum = rowsum(wf) in fp32 (sdmoe_ln_fold) — the operands of sdmoe_linear_ln /
    sdmoe_linear_geglu_ln. Built once per (weight, norm) version by the owning module."""

    def __init__(self, w, gamma, beta, eps, bias=None):
        lib = _lib.load()
        N, K = w.shape
        self.eps = float(eps)
        self.w = torch.empty((N, K), dtype=torch.float16, device=w.device)
        self.bias = torch.empty(N, dtype=torch.float32, device=w.device)
        self.wsum = torch.empty(N, dtype=torch.float32, device=w.device)
        if bias is not None:
            _dev(bias, "bias")
        st = lib.sdmoe_ln_fold(_dev(w, "w"), w.stride(0), N, K, _dev(gamma, "gamma"), _dev(beta, "beta"), _ptr(bias),
                               self.w.data_ptr(), K, self.bias.data_ptr(), self.wsum.data_ptr(), _stream())
        _lib.check(st, "sdmoe_ln_fold")

    def rows(self, idx):
        """The fold with its rows reordered (torch index tensor): a view-free copy for permuted layouts."""
        f = LNFold.__new__(LNFold)
        f.eps, f.w, f.bias, f.wsum = self.eps, self.w[idx].contiguous(), self.bias[idx].contiguous(), \
            self.wsum[idx].contiguous()
        return f


def linear_ln(x, fold: LNFold, out=None):
    """out = LayerNorm(x) @ W^T + bias with the norm folded into the GEMM (sdmoe_linear_ln): x is the
    un-normalised [M, K] input; no normalised copy of x is written."""
    lib = _lib.load()
    xp, lda = _rows(x, "x")
    M, K = x.shape
    N = fold.w.shape[0]
    if fold.w.shape[1] != K:
        raise ValueError(f"linear_ln: folded weight {tuple(fold.w.shape)} does not match input K={K}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    op, ldc = _rows(out, "out")
    st = lib.sdmoe_linear_ln(xp, lda, fold.w.data_ptr(), fold.w.stride(0), fold.bias.data_ptr(), fold.wsum.data_ptr(),
                             fold.eps, op, ldc, M, N, K, _stream())
    _lib.check(st, "sdmoe_linear_ln")
    return out


def attention(q, k, v, nimg, Nq, Nk, heads, out=None, scale=None):
    """softmax(q k^T * scale) v per (image, head); q [nimg*Nq, heads*d], k/v [nimg*Nk, heads*d] views."""
    lib = _lib.load()
    qp, ldq = _rows(q, "q")
    kp, ldk = _rows(k, "k")
    vp, ldv = _rows(v, "v")
    C = q.shape[1]
    d = C // heads
    if out is None:
        out = torch.empty((nimg * Nq, C), dtype=torch.float16, device=q.device)
    op, ldo = _rows(out, "out")
    if scale is None:
        scale = d ** -0.5
    st = lib.sdmoe_attention(qp, ldq, kp, ldk, vp, ldv, op, ldo, nimg, Nq, Nk, heads, d, float(scale), _stream())
    _lib.check(st, "sdmoe_attention")
    return out


class Routing:
    """Device-side expert layout of one MoE-fied GEGLU: labels [F] int32 and the per-expert neuron lists
    (CSR), built once from the reference's `module.patterns` [E, F] (helper.py:48-62) or its label file."""

    def __init__(self, labels: torch.Tensor, num_experts: int, k: int, device):
        labels = labels.to(torch.int64).cpu()
        F = labels.numel()
        if labels.min() < 0 or labels.max() >= num_experts:
            raise ValueError("expert labels out of range")
        order = torch.argsort(labels, stable=True)
        counts = torch.bincount(labels, minlength=num_experts)
        off = torch.zeros(num_experts + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(counts, 0)
        self.F, self.E, self.k = F, int(num_experts), int(k)
        self.labels = labels.to(torch.int32).to(device)
        self.e_off = off.to(torch.int32).to(device)
        self.e_nid = order.to(torch.int32).to(device)
        # fused path (sdmoe_linear_geglu + sdmoe_moe_topk_mask): balanced experts (the reference's
        # KMeansConstrained split), permuted expert-major so every expert is a contiguous neuron slice
        sizes = set(counts.tolist())
        self.esize = sizes.pop() if len(sizes) == 1 else 0
        self.perm = order  # new neuron position -> original neuron id (cpu int64)
        self.perm_dev = order.to(torch.int32).to(device)  # the same on the device (Wanda mask column permutation)
        self.fusable = bool(self.esize and 40 % self.esize == 0 and F % 80 == 0 and self.E <= 256)

    @classmethod
    def from_patterns(cls, patterns: torch.Tensor, k: int, device=None):
        p = patterns.detach().float().cpu()
        E, F = p.shape
        if not torch.all((p == 0) | (p == 1)) or not torch.all(p.sum(0) == 1):
            raise ValueError("patterns must be a 0/1 [E, F] matrix with exactly one expert per neuron")
        labels = p.argmax(0)
        return cls(labels, E, k, device or patterns.device)


def geglu_rows(F: int, perm: torch.Tensor | None, device) -> torch.Tensor:
    """Source row of proj.weight [2F, K] (value rows, then gate rows) for every row of the layout sdmoe_linear_geglu
    reads (include/sdmoe.h): neurons permuted by `perm`, value and gate rows interleaved per neuron pair [v 2 | g 2]
    (rows 4 q .. 4 q + 3 = value 2 q, value 2 q + 1, gate 2 q, gate 2 q + 1), so each lane of the kernel's swapped
    MFMA fragments holds both halves of two neurons."""
    if F % 2:
        raise ValueError(f"GEGLU layout: F = {F} is odd")
    idx = torch.arange(F, device=device) if perm is None else perm.to(device)
    r = torch.arange(2 * F, device=device)
    q, e = r // 4, r % 4
    c = 2 * q + (e & 1)
    return torch.where(e < 2, idx[c], F + idx[c])


def interleave_geglu(weight: torch.Tensor, bias: torch.Tensor | None, perm: torch.Tensor | None):
    """proj.weight [2F, K] -> rows in geglu_rows' order (neurons permuted by `perm`), the layout sdmoe_linear_geglu
    reads; bias likewise (zeros if None)."""
    F2, K = weight.shape
    rows = geglu_rows(F2 // 2, perm, weight.device)
    b = torch.zeros(F2, dtype=weight.dtype, device=weight.device) if bias is None else bias
    return weight[rows].contiguous(), b[rows].contiguous()


def interleave_ln_fold(fold: LNFold, perm: torch.Tensor | None) -> LNFold:
    """An LNFold of proj.weight [2F, K] with its rows in interleave_geglu's order."""
    F = fold.w.shape[0] // 2
    return fold.rows(geglu_rows(F, perm, fold.w.device))


_GELU_TABLES = {}


def gelu_table_values() -> torch.Tensor:
    """The 16384 fp16 inputs x with 2^-5 <= |x| < 8 in sdmoe_set_gelu_table's index order (int16 bit patterns:
    index i -> |x| bits 0x2800 + (i & 8191), sign i >> 13), as an fp16 CPU tensor."""
    i = torch.arange(16384, dtype=torch.int32)
    bits = (0x2800 + (i & 8191)) | ((i >> 13) << 15)
    return bits.to(torch.int16).view(torch.float16)


def ensure_gelu_table(device) -> torch.Tensor:
    """Register (once per device) the GELU table the GEGLU kernels apply for act == GELU: the reference module's
    activation itself -- diffusers GEGLU.gelu is F.gelu, which the hook applies to the fp16 gate (moefy.py:13,
    remove_skilled_experts.py:27) -- evaluated on every fp16 input of the table's range, so the device gates equal
    the reference's fp16 gates bit for bit (sdmoe_set_gelu_table, include/sdmoe.h). Must run outside graph capture
    (one host->device copy); the first GELU call on a device does it."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _GELU_TABLES.get(idx)
    if t is None:
        # F.gelu on the DEVICE fp16 tensor: the reference hook applies module.gelu to the gate on the GPU the model
        # sits on (base_receiver.py model.to(args.gpu); moefy.py:13, remove_skilled_experts.py:27)
        t = torch.nn.functional.gelu(gelu_table_values().to(torch.device("cuda", idx))).contiguous()
        lib = _lib.load()
        if _lib.has(lib, "sdmoe_set_gelu_table"):  # (an older A/B build evaluates GELU itself)
            with torch.cuda.device(idx):
                _lib.check(lib.sdmoe_set_gelu_table(t.data_ptr()), "sdmoe_set_gelu_table")
        _GELU_TABLES[idx] = t
    return t


def linear_geglu(x, w_il, b_il, act=ACT_GELU, *, score=None, esize=0, out=None, ln: LNFold | None = None):
    """P = value * act(gate) from the interleaved projection (interleave_geglu), plus per-expert gate sums
    into score [M, E] (experts = contiguous esize-neuron slices) when given. ln (interleave_ln_fold): x is the
    un-normalised input and the LayerNorm is folded into the GEMM (w_il / b_il are then ignored)."""
    lib = _lib.load()
    if act == ACT_GELU:
        ensure_gelu_table(x.device)
    if ln is not None:
        xp, lda = _rows(x, "x")
        M, K = x.shape
        F = ln.w.shape[0] // 2
        if out is None:
            out = torch.empty((M, F), dtype=torch.float16, device=x.device)
        op, ldp = _rows(out, "out")
        sp, lds = (None, 0) if score is None else _rows(score, "score")
        st = lib.sdmoe_linear_geglu_ln(xp, lda, ln.w.data_ptr(), ln.w.stride(0), ln.bias.data_ptr(),
                                       ln.wsum.data_ptr(), ln.eps, op, ldp, M, F, K, act, sp, lds, int(esize),
                                       _stream())
        _lib.check(st, "sdmoe_linear_geglu_ln")
        return out
    xp, lda = _rows(x, "x")
    M, K = x.shape
    F = w_il.shape[0] // 2
    if w_il.shape[1] != K:
        raise ValueError(f"linear_geglu: weight {tuple(w_il.shape)} does not match input K={K}")
    if out is None:
        out = torch.empty((M, F), dtype=torch.float16, device=x.device)
    op, ldp = _rows(out, "out")
    sp, lds = (None, 0) if score is None else _rows(score, "score")
    st = lib.sdmoe_linear_geglu(xp, lda, _dev(w_il, "w"), w_il.stride(0), _dev(b_il, "bias"), op, ldp, M, F, K,
                                act, sp, lds, int(esize), _stream())
    _lib.check(st, "sdmoe_linear_geglu")
    return out


def moe_topk_mask(P, score, routing: "Routing", removed=None, sel_out=None, k=None):
    """In place on the fused product P [M, F]: zero the neurons of experts outside each token's top-k. k overrides
    routing.k."""
    lib = _lib.load()
    pp, ldp = _rows(P, "P")
    sp, lds = _rows(score, "score")
    st = lib.sdmoe_moe_topk_mask(pp, ldp, P.shape[0], P.shape[1], routing.E, routing.esize,
                                 routing.k if k is None else int(k), sp, lds, _ptr(removed), _ptr(sel_out), _stream())
    _lib.check(st, "sdmoe_moe_topk_mask")
    return P


def moe_topk_keep(score, routing: "Routing", M: int, removed=None, sel_out=None, keep=None, k=None):
    """Top-k selection of sdmoe_moe_topk_mask as keep bits for sdmoe_linear_keep: int64 [F/64, M] words, bit j of
    word (s, m) = expert-major neuron 64 s + j of token m kept. k overrides routing.k."""
    lib = _lib.load()
    sp, lds = _rows(score, "score")
    F = routing.E * routing.esize
    if keep is None:
        keep = torch.empty((F // 64, M), dtype=torch.int64, device=score.device)
    if tuple(keep.shape) != (F // 64, M) or keep.dtype != torch.int64:
        raise ValueError(f"keep must be int64 [{F // 64}, {M}], got {keep.dtype} {tuple(keep.shape)}")
    st = lib.sdmoe_moe_topk_keep(M, F, routing.E, routing.esize, routing.k if k is None else int(k), sp, lds,
                                 _ptr(removed), _dev(keep, "keep", torch.int64), _ptr(sel_out), _stream())
    _lib.check(st, "sdmoe_moe_topk_keep")
    return keep


def linear_keep(x, keep, w, bias=None, *, residual=None, out=None, wmask=None):
    """out = (x with the neurons whose keep bit is clear zeroed) @ w.T + bias + residual (sdmoe_linear_keep);
    with wmask (wmask_kmajor layout) the Wanda weight mask too (sdmoe_linear_masked)."""
    if wmask is not None:
        return linear_masked(x, w, bias, keep=keep, wmask=wmask, residual=residual, out=out)
    lib = _lib.load()
    xp, lda = _rows(x, "x")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(keep.shape) != (K // 64, M) or keep.dtype != torch.int64:
        raise ValueError(f"linear_keep: x {tuple(x.shape)}, keep {tuple(keep.shape)}, w {tuple(w.shape)} mismatch")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    op, ldc = _rows(out, "out")
    rp, ldr = (None, 0) if residual is None else _rows(residual, "residual")
    ws = _workspace(x.device)
    st = lib.sdmoe_linear_keep(xp, lda, _dev(keep, "keep", torch.int64), _dev(w, "w"), w.stride(0), _ptr(bias), rp,
                               ldr, op, ldc, M, N, K, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "sdmoe_linear_keep")
    return out


def removed_bits(expert_ids, num_experts: int, device) -> torch.Tensor:
    """uint32-packed (as int32) bitmask of removed experts."""
    nw = (num_experts + 31) // 32
    words = [0] * nw
    for e in expert_ids:
        e = int(e)
        if not 0 <= e < num_experts:
            raise IndexError(f"expert id {e} out of range [0, {num_experts})")
        words[e >> 5] |= 1 << (e & 31)
    words = [w - (1 << 32) if w >= (1 << 31) else w for w in words]
    return torch.tensor(words, dtype=torch.int32, device=device)


def expert_bias(expert_ids, std, E: int, device, scale=5.0) -> torch.Tensor:
    """The per-expert score bias of AddExperts (add_skilled_experts.py:55) as fp16 [E] on `device`:
    scale * torch.tensor(std).to(float16) -- the reference's own torch operations on the CPU, so its two roundings
    (std to fp16, then the scalar product to fp16) -- at the listed expert ids, +0 elsewhere. A duplicate id is applied
    once, as the reference's indexed assignment does. Raises IndexError for an id outside [0, E) and, unlike the
    reference (which would add it to the scores), ValueError when a LISTED expert's std or bias is NaN or infinite
    (StatMeter writes NaN for a cell it never updated)."""
    E = int(E)
    std = [float(v) for v in std]
    if len(std) != E:
        raise ValueError(f"expert_bias: std has {len(std)} entries, the module has {E} experts")
    ids = []
    for e in expert_ids:
        e = int(e)
        if not 0 <= e < E:
            raise IndexError(f"expert id {e} out of range [0, {E})")
        ids.append(e)
    bias = torch.zeros(E, dtype=torch.float16)
    if ids:
        idx = torch.tensor(sorted(set(ids)), dtype=torch.int64)
        std16 = torch.tensor(std).to(torch.float16)
        listed = (float(scale) * std16)[idx]
        if not bool(torch.isfinite(std16[idx]).all() and torch.isfinite(listed).all()):
            bad = [int(e) for e in idx[~(torch.isfinite(std16[idx]) & torch.isfinite(listed))]]
            raise ValueError(f"expert_bias: std or bias of listed experts {bad} is NaN or infinite")
        bias[idx] = listed
    return bias.to(device)


def score_bias(score, bias, out=None):
    """out[m, e] = fp16(score[m, e] + bias[e]) (sdmoe_score_bias): score [M, E] fp16 (a row-strided view is fine),
    bias fp16 [E] (expert_bias). out None: in place on score. Returns out."""
    lib = _lib.load()
    sp, lds = _rows(score, "score")
    M, E = score.shape
    if tuple(bias.shape) != (E,):
        raise ValueError(f"score_bias: bias {tuple(bias.shape)} is not {(E,)}")
    if out is None:
        out = score
    if tuple(out.shape) != (M, E):
        raise ValueError(f"score_bias: out {tuple(out.shape)} is not {(M, E)}")
    op, ldo = _rows(out, "out")
    st = lib.sdmoe_score_bias(sp, lds, M, E, _dev(bias, "bias"), op, ldo, _stream())
    _lib.check(st, "sdmoe_score_bias")
    return out


def geglu_route(y, routing: Routing | None, act=ACT_GELU, removed=None, out=None, gate_out=None, sel_out=None,
                score_out=None, k=None, bias=None):
    """Routed GEGLU over y = proj(x) [M, 2F]; routing None -> dense value*act(gate). k overrides routing.k
    (k = E: every expert kept, i.e. the dense product plus the per-token expert scores). bias (fp16 [E],
    expert_bias): added to the fp16 expert scores before they are ranked and written (sdmoe_geglu_route_bias)."""
    lib = _lib.load()
    if act == ACT_GELU:
        ensure_gelu_table(y.device)
    yp, ldy = _rows(y, "y")
    M = y.shape[0]
    F = y.shape[1] // 2
    if out is None:
        out = torch.empty((M, F), dtype=torch.float16, device=y.device)
    op, ldo = _rows(out, "out")
    gp, ldg = (None, 0) if gate_out is None else _rows(gate_out, "gate_out")
    if routing is None:
        E, k, lab, off, nid = 0, 0, None, None, None
    else:
        if routing.F != F:
            raise ValueError(f"routing has F={routing.F}, projection gives F={F}")
        E, k = routing.E, (routing.k if k is None else int(k))
        lab, off, nid = routing.labels.data_ptr(), routing.e_off.data_ptr(), routing.e_nid.data_ptr()
    if bias is not None:
        if routing is None or tuple(bias.shape) != (E,):
            raise ValueError(f"geglu_route: bias {tuple(bias.shape)} needs a routing with E = {bias.numel()} experts")
        st = lib.sdmoe_geglu_route_bias(yp, ldy, M, F, E, k, act, lab, off, nid, _ptr(removed), op, ldo, gp, ldg,
                                        _ptr(sel_out), _ptr(score_out), _dev(bias, "bias"), _stream())
        _lib.check(st, "sdmoe_geglu_route_bias")
        return out
    st = lib.sdmoe_geglu_route(yp, ldy, M, F, E, k, act, lab, off, nid, _ptr(removed), op, ldo, gp, ldg,
                               _ptr(sel_out), _ptr(score_out), _stream())
    _lib.check(st, "sdmoe_geglu_route")
    return out


def neuron_bits(mask01, device) -> torch.Tensor:
    """A 0/1 list of length F (F % 32 == 0) packed into [F/32] int32 words, bit n % 32 of word n // 32 = neuron n
    (little-endian within a word): the override_bits of geglu_neurons."""
    import numpy as np
    m = np.asarray(mask01).reshape(-1) != 0
    if m.size % 32:
        raise ValueError(f"neuron_bits: {m.size} neurons are not a multiple of 32")
    words = np.packbits(m, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)
    return torch.from_numpy(words.copy()).to(device)


def position_bits(positions, rows_per_img: int, device) -> torch.Tensor:
    """Token positions (each in [0, rows_per_img)) as the [ceil(rows_per_img / 32)] int32 pos_bits of geglu_neurons."""
    import numpy as np
    m = np.zeros(-(-int(rows_per_img) // 32) * 32, dtype=bool)
    idx = np.asarray(list(positions), dtype=np.int64)
    if idx.size == 0 or idx.min() < 0 or idx.max() >= rows_per_img:
        raise ValueError(f"position_bits: positions must be a non-empty subset of [0, {rows_per_img})")
    m[idx] = True
    words = np.packbits(m, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)
    return torch.from_numpy(words.copy()).to(device)


def _geglu_seam(fn, y, act, out, gate_out):
    """The operands of a streaming pass over the GEGLU seam y = proj(x) [M, 2F] (geglu_neurons, geglu_sparsity): loads
    the library and the GELU table, allocates out [M, F] when None and checks the shapes of out and gate_out. Returns
    (lib, M, F, out, (y pointer, ldy), (out pointer, ldo), (gate_out pointer or None, ldg))."""
    lib = _lib.load()
    if act == ACT_GELU:
        ensure_gelu_table(y.device)
    yl = _rows(y, "y")
    M = y.shape[0]
    F = y.shape[1] // 2
    if out is None:
        out = torch.empty((M, F), dtype=torch.float16, device=y.device)
    ol = _rows(out, "out")
    if tuple(out.shape) != (M, F):
        raise ValueError(f"{fn}: out {tuple(out.shape)} is not {(M, F)}")
    gl = (None, 0) if gate_out is None else _rows(gate_out, "gate_out")
    if gate_out is not None and tuple(gate_out.shape) != (M, F):
        raise ValueError(f"{fn}: gate_out {tuple(gate_out.shape)} is not {(M, F)}")
    return lib, M, F, out, yl, ol, gl


def _image_groups(fn, M, rows_per_img, img_group, one=1):
    """M rows as images of rows_per_img rows (0: `one` image) with an optional group table: (rows_per_img as an int,
    images, img_group pointer or None). The table's length is checked where the rows divide into images; where they do
    not, the entry point refuses the call."""
    rpi = int(rows_per_img)
    divides = rpi <= 0 or M % rpi == 0
    nimg = M // rpi if rpi > 0 and divides else one
    if img_group is None:
        return rpi, nimg, None
    if divides and img_group.numel() != nimg:
        raise ValueError(f"{fn}: img_group has {img_group.numel()} entries for {nimg} images")
    return rpi, nimg, _dev(img_group, "img_group", torch.int32)


def _ws_args(device, workspace):
    """(pointer, floats) of the fp32 scratch of a statistics pass: `workspace`, or the device's shared one."""
    ws = _workspace(device) if workspace is None else workspace
    return _dev(ws, "workspace", torch.float32), ws.numel()


def geglu_neurons(y, act=ACT_GELU, *, override_bits=None, override_value=0.0, gate_out=None, rows_per_img=0,
                  img_group=None, ngroups=1, pos_bits=None, colmax=None, out=None, workspace=None):
    """Dense GEGLU over y = proj(x) [M, 2F] with a per-neuron gate override and a per-group column maximum
    (sdmoe_geglu_neurons): out = value * g', g' = fp16(override_value) where override_bits (int32 [F/32], neuron_bits)
    is set, else g = act(gate); gate_out (optional [M, F]) receives g'; colmax (optional fp16 [ngroups, F]) the
    maximum of g -- before the override -- over the rows of the images of each group (image i = rows_per_img rows,
    group img_group[i], int32 device [M / rows_per_img]; None = all group 0), restricted to the positions of pos_bits
    (int32 [ceil(rows_per_img / 32)], position_bits) when given. workspace: fp32 scratch for the per-slab partial
    maxima (default: the device's shared workspace). Returns out."""
    lib, M, F, out, (yp, ldy), (op, ldo), (gp, ldg) = _geglu_seam("geglu_neurons", y, act, out, gate_out)
    obp = None
    if override_bits is not None:
        if override_bits.numel() * 32 != F:
            raise ValueError(f"geglu_neurons: {override_bits.numel()} override words for F={F}")
        obp = _dev(override_bits, "override_bits", torch.int32)
    cp = pbp = None
    if colmax is not None:
        if tuple(colmax.shape) != (int(ngroups), F):
            raise ValueError(f"geglu_neurons: colmax {tuple(colmax.shape)} is not {(int(ngroups), F)}")
        cp = _dev(colmax, "colmax")
    rpi, _, igp = _image_groups("geglu_neurons", M, rows_per_img, img_group if colmax is not None else None)
    if colmax is not None and pos_bits is not None:
        if pos_bits.numel() != -(-(rpi if rpi > 0 else M) // 32):
            raise ValueError(f"geglu_neurons: {pos_bits.numel()} pos_bits words for {rpi if rpi > 0 else M} rows")
        pbp = _dev(pos_bits, "pos_bits", torch.int32)
    st = lib.sdmoe_geglu_neurons(yp, ldy, M, F, act, obp, float(override_value), op, ldo, gp, ldg, rpi, igp,
                                 int(ngroups), pbp, cp, *_ws_args(y.device, workspace), _stream())
    _lib.check(st, "sdmoe_geglu_neurons")
    return out


def geglu_sparsity(y, act=ACT_GELU, *, threshold=0.0, rows_per_img=0, img_group=None, ngroups=1, col_zero=None,
                   col_neg=None, totals=None, out=None, workspace=None, gate_out=None):
    """Dense GEGLU over y = proj(x) [M, 2F] with the gate-sparsity counts of the same pass (sdmoe_geglu_sparsity):
    out = value * g, g = act(gate), bit-identical to geglu_neurons without an override; per group of images (image i =
    rows_per_img rows, group img_group[i], int32 device [M / rows_per_img]; None = all group 0) and neuron, col_zero
    (optional int32 [ngroups, F]) receives the number of rows with |g| <= threshold (fp32 compare; 0.0 counts the exact
    zeros of either sign), col_neg (optional int32 [ngroups, F]) the rows with g < 0, totals (optional int64
    [ngroups, 2]) their sums over the neurons. Either totals or both arrays must be given; every given buffer is
    written in full (none needs zeroing). gate_out (optional [M, F]) receives g. workspace: fp32 scratch for the
    per-slab partial counts (default: the device's shared workspace). Returns out."""
    lib, M, F, out, (yp, ldy), (op, ldo), (gp, ldg) = _geglu_seam("geglu_sparsity", y, act, out, gate_out)
    if totals is None and (col_zero is None or col_neg is None):
        raise ValueError("geglu_sparsity: give totals, or both col_zero and col_neg")
    ptrs = {}
    for name, t, shape, dtype in (("col_zero", col_zero, (int(ngroups), F), torch.int32),
                                  ("col_neg", col_neg, (int(ngroups), F), torch.int32),
                                  ("totals", totals, (int(ngroups), 2), torch.int64)):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"geglu_sparsity: {name} {tuple(t.shape)} is not {shape}")
        ptrs[name] = None if t is None else _dev(t, name, dtype)
    rpi, _, igp = _image_groups("geglu_sparsity", M, rows_per_img, img_group)
    st = lib.sdmoe_geglu_sparsity(yp, ldy, M, F, act, float(threshold), op, ldo, gp, ldg, rpi, igp, int(ngroups),
                                  ptrs["col_zero"], ptrs["col_neg"], ptrs["totals"],
                                  *_ws_args(y.device, workspace), _stream())
    _lib.check(st, "sdmoe_geglu_sparsity")
    return out


NOISE_SLAB_ROWS = 1024  # rows per partial sum of sdmoe_noise_distance (its workspace bound, include/sdmoe.h)


def noise_capture(eps, store):
    """Channels 0..3 of every row of eps (fp16 [rows, >= 4], e.g. the pipeline's padded U-Net output) -> store (fp16
    [rows, >= 4]; a compact [rows, 4] step slice of a [T, rows, 4] noise store), on the current stream
    (sdmoe_noise_capture). Columns past 3 of either are never touched. Returns store."""
    lib = _lib.load()
    ep, lde = _rows(eps, "eps")
    sp, lds = _rows(store, "store")
    if eps.shape[0] != store.shape[0] or eps.shape[1] < 4 or store.shape[1] < 4:
        raise ValueError(f"noise_capture: eps {tuple(eps.shape)} and store {tuple(store.shape)} need the same rows and "
                         f">= 4 channels")
    _lib.check(lib.sdmoe_noise_capture(ep, lde, sp, lds, eps.shape[0], _stream()), "sdmoe_noise_capture")
    return store


def noise_distance(a, b, nimg, *, img_group=None, ngroups=1, out=None, workspace=None):
    """The noise-HPO sums of two stores of per-step U-Net outputs (sdmoe_noise_distance): a, b fp16 [T, nimg * HW, ld]
    (ld >= 4, the row and step strides multiples of 4; only channels 0..3 are read); image i of a step belongs to group
    img_group[i] (int32 device [nimg]; None: one group). Returns the device float64 [T, ngroups, 4] of
    {S (a - b)^2, A = S |a|, B = S |b|, S (a / max(A, 1e-12) - b / max(B, 1e-12))^2} per step and group, accumulated in
    float64 in a fixed order (bit-identical from run to run). workspace: float64 scratch of at least
    4 * T * nimg * ceil(HW / 1024) values (default: allocated per call -- a few KB)."""
    lib = _lib.load()
    for name, t in (("a", a), ("b", b)):
        if t.dim() != 3:
            raise ValueError(f"noise_distance: {name} must be [T, nimg * HW, ld], got {tuple(t.shape)}")
        if not t.is_cuda:
            raise _lib.SdmoeError(f"noise_distance: {name} is not on a GPU device; sdmoe has no CPU path")
        if t.dtype != torch.float16:
            raise TypeError(f"noise_distance: {name}: expected float16, got {t.dtype}")
        if t.stride(2) != 1 and t.shape[2] > 1:
            raise ValueError(f"noise_distance: {name}: inner dimension must be contiguous")
    if a.shape[:2] != b.shape[:2] or a.device != b.device:
        raise ValueError(f"noise_distance: a {tuple(a.shape)} and b {tuple(b.shape)} differ in steps, rows or device")
    T, rows = a.shape[0], a.shape[1]
    nimg = int(nimg)
    if nimg <= 0 or rows % nimg:
        raise ValueError(f"noise_distance: {rows} rows per step are not {nimg} images")
    HW = rows // nimg
    if a.shape[2] < 4 or b.shape[2] < 4:
        raise ValueError("noise_distance: a and b need >= 4 channels")
    igp = None
    if img_group is not None:
        if img_group.numel() != nimg:
            raise ValueError(f"noise_distance: img_group has {img_group.numel()} entries for {nimg} images")
        igp = _dev(img_group, "img_group", torch.int32)
    if out is None:
        out = torch.empty((T, int(ngroups), 4), dtype=torch.float64, device=a.device)
    elif tuple(out.shape) != (T, int(ngroups), 4):
        raise ValueError(f"noise_distance: out {tuple(out.shape)} is not {(T, int(ngroups), 4)}")
    if workspace is None:
        workspace = torch.empty(4 * T * nimg * -(-HW // NOISE_SLAB_ROWS), dtype=torch.float64, device=a.device)
    st = lib.sdmoe_noise_distance(a.data_ptr(), a.stride(1), a.stride(0), b.data_ptr(), b.stride(1), b.stride(0), T,
                                  nimg, HW, igp, int(ngroups), _dev(out, "out", torch.float64),
                                  _dev(workspace, "workspace", torch.float64), workspace.numel(), _stream())
    _lib.check(st, "sdmoe_noise_distance")
    return out


CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)   # transformers OPENAI_CLIP_MEAN / OPENAI_CLIP_STD
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
_RESAMPLE_BITS = 22  # Pillow's 8bpc PRECISION_BITS


def clip_quantise(x, out=None):
    """[B, 3, H, W] fp16 / fp32 in [0, 1] (output_type='pt') -> [B, H, W, 3] uint8, rint(x * 255) half-even, clamped:
    diffusers' numpy_to_pil on the device (sdmoe_clip_quantise)."""
    lib = _lib.load()
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"clip_quantise: expected [B, 3, H, W], got {tuple(x.shape)}")
    if x.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"clip_quantise: expected float16 or float32, got {x.dtype}")
    xp = _dev(x, "x", x.dtype)
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    elif tuple(out.shape) != (B, H, W, 3):
        raise ValueError(f"clip_quantise: out {tuple(out.shape)} is not {(B, H, W, 3)}")
    st = lib.sdmoe_clip_quantise(xp, int(x.dtype == torch.float32), B, H, W, _dev(out, "out", torch.uint8), _stream())
    _lib.check(st, "sdmoe_clip_quantise")
    return out


def _bicubic(x):
    """Pillow's bicubic_filter (a = -0.5)."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _triangle(x):
    """Pillow's bilinear_filter."""
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


RESAMPLE_FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_triangle, 1.0)}  # name -> (filter, support)


def clip_resample_coeffs(in_size: int, out_size: int, first: int = 0, count: int | None = None,
                         filter: str = "bicubic"):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for outputs [first, first + count) of a resize of one axis
    from in_size to out_size with `filter` (RESAMPLE_FILTERS: Image.BICUBIC, the default, or Image.BILINEAR), in
    float64 scalar arithmetic in Pillow's operation order: (bounds, kk, ksize), bounds = [(first tap, taps)], kk =
    rows of ksize 22-bit fixed-point integer weights (zero past the taps)."""
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"clip_resample_coeffs: filter {filter!r} is not one of {sorted(RESAMPLE_FILTERS)}")
    fn, fsupport = RESAMPLE_FILTERS[filter]
    count = out_size - first if count is None else count
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fsupport * fs
    ksize = int(-(-support // 1)) * 2 + 1
    ss = 1.0 / fs
    bounds, kk = [], []
    for i in range(first, first + count):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        row = [int(v * (1 << _RESAMPLE_BITS) - 0.5) if v < 0 else int(v * (1 << _RESAMPLE_BITS) + 0.5) for v in w]
        bounds.append((xmin, n))
        kk.append(row + [0] * (ksize - n))
    return bounds, kk, ksize


def clip_resize_shape(H: int, W: int, size: int):
    """transformers' CLIP resize: the shortest edge to `size`, the long edge to int(size * long / short)."""
    short, long = (H, W) if H <= W else (W, H)
    new_long = int(size * long / short)
    return (size, new_long) if H <= W else (new_long, size)


def centre_crop_offsets(oh: int, ow: int, size: int, half_even: bool = False):
    """(top, left) of a size x size centre crop of an oh x ow image: transformers' (oh - size) // 2, or with half_even
    torchvision's int(round((oh - size) / 2.0)) (Python's round: a difference ending in .5 goes to the even offset)."""
    if half_even:
        return int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))
    return (oh - size) // 2, (ow - size) // 2


class ClipResamplePlan:
    """Device tables of the resize (shortest edge -> `resize`, S by default) + centre crop S x S of H x W images: only
    the crop window's columns and rows, and the input rows [row0, row0 + nrows) the vertical pass reads. filter and
    half_even choose the preset: CLIPImageProcessor's (bicubic, floor crop offsets; the default) or torchvision's
    ImageClassification (bilinear, resize 232 > crop 224, half-even crop offsets)."""

    def __init__(self, H, W, S, device, *, resize=None, filter="bicubic", half_even=False):
        resize = S if resize is None else int(resize)
        if resize < S:
            raise ValueError(f"resize {resize} is smaller than the crop {S}")
        oh, ow = clip_resize_shape(H, W, resize)
        self.H, self.W, self.S, self.resize = H, W, S, resize
        self.top, self.left = centre_crop_offsets(oh, ow, S, half_even)
        bx, kx, self.ksx = clip_resample_coeffs(W, ow, self.left, S, filter)
        by, ky, self.ksy = clip_resample_coeffs(H, oh, self.top, S, filter)
        self.row0 = min(lo for lo, _ in by)
        self.nrows = max(lo + n for lo, n in by) - self.row0
        if min(lo for lo, _ in bx) < 0 or max(lo + n for lo, n in bx) > W or self.row0 < 0 \
                or self.row0 + self.nrows > H:
            raise ValueError("clip resample table outside the image")

        def dev(rows):
            return torch.tensor(rows, dtype=torch.int32).to(device).contiguous()

        self.bx, self.kx, self.by, self.ky = dev(bx), dev(kx), dev(by), dev(ky)


_CLIP_PLANS = {}


def clip_resample_plan(H, W, S, device, *, resize=None, filter="bicubic", half_even=False) -> ClipResamplePlan:
    key = (int(H), int(W), int(S), str(device), None if resize is None else int(resize), filter, bool(half_even))
    plan = _CLIP_PLANS.get(key)
    if plan is None:
        plan = _CLIP_PLANS[key] = ClipResamplePlan(int(H), int(W), int(S), device, resize=resize, filter=filter,
                                                   half_even=half_even)
    return plan


def clip_padded_k(patch: int) -> int:
    """3 * patch^2 padded up to the patch GEMM's K granule (64)."""
    return -(-3 * patch * patch // 64) * 64


def clip_preprocess(u8, size: int, patch: int = 0, *, a_out=None, u8_out=None, mean=CLIP_IMAGE_MEAN,
                    std=CLIP_IMAGE_STD, resize=None, filter="bicubic", half_even=False):
    """CLIPImageProcessor on the device for u8 [B, H, W, 3] uint8: Pillow-exact bicubic resize (shortest edge -> size),
    centre crop size x size (sdmoe_clip_resample_h / _v). a_out: fp16 [B * (size / patch)^2, >= clip_padded_k(patch)]
    row view that receives the normalised, patchified pixels (the patch GEMM's A operand, padding columns zero);
    u8_out: uint8 [B, size, size, 3] that receives the cropped pixels. Returns (a_out, u8_out).
    resize / filter / half_even (ClipResamplePlan) select another preset on the same kernels: torchvision's
    ImageClassification is resize=232, size=224, filter="bilinear", half_even=True."""
    lib = _lib.load()
    if u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError(f"clip_preprocess: expected [B, H, W, 3] uint8, got {tuple(u8.shape)}")
    if a_out is None and u8_out is None:
        raise ValueError("clip_preprocess: nothing to write (a_out and u8_out are both None)")
    up = _dev(u8, "u8", torch.uint8)
    B, H, W, _ = u8.shape
    S = int(size)
    plan = clip_resample_plan(H, W, S, u8.device, resize=resize, filter=filter, half_even=half_even)
    ap, lda, kpad = None, 0, 0
    if a_out is not None:
        if patch <= 0 or S % patch:
            raise ValueError(f"clip_preprocess: patch {patch} does not divide size {S}")
        kpad = clip_padded_k(patch)
        ap, lda = _rows(a_out, "a_out")
        if a_out.shape[0] != B * (S // patch) ** 2 or a_out.shape[1] != kpad:
            raise ValueError(f"clip_preprocess: a_out {tuple(a_out.shape)} is not {(B * (S // patch) ** 2, kpad)}")
    if u8_out is not None and tuple(u8_out.shape) != (B, S, S, 3):
        raise ValueError(f"clip_preprocess: u8_out {tuple(u8_out.shape)} is not {(B, S, S, 3)}")
    uop = None if u8_out is None else _dev(u8_out, "u8_out", torch.uint8)
    tmp = torch.empty((B, plan.nrows, S, 3), dtype=torch.uint8, device=u8.device)
    st = lib.sdmoe_clip_resample_h(up, H * W * 3, B, H, W, plan.row0, plan.nrows, plan.bx.data_ptr(),
                                   plan.kx.data_ptr(), plan.ksx, S, tmp.data_ptr(), _stream())
    _lib.check(st, "sdmoe_clip_resample_h")
    f3 = ctypes.c_float * 3
    st = lib.sdmoe_clip_resample_v(tmp.data_ptr(), B, plan.row0, plan.nrows, plan.by.data_ptr(), plan.ky.data_ptr(),
                                   plan.ksy, S, int(patch) if a_out is not None else 0, f3(*mean), f3(*std), uop, ap,
                                   lda, kpad, _stream())
    _lib.check(st, "sdmoe_clip_resample_v")
    return a_out, u8_out


def clip_scores(T, A, R, out=None):
    """Removal-quality cosines of fp16 feature rows T (text; None), A (original), R (removal) [n, D]
    (sdmoe_clip_scores): device float64 [3 n + 3] = cos(T,A) | cos(T,R) | cos(A,R) | sum cos(A,R), sum cos(A,R)^2,
    count of cos(T,A) > cos(T,R). float64, fixed order: bit-identical from run to run."""
    lib = _lib.load()
    ap, lda = _rows(A, "A")
    rp, ldr = _rows(R, "R")
    tp, ldt = (None, 0) if T is None else _rows(T, "T")
    n, D = A.shape
    if R.shape != A.shape or (T is not None and T.shape != A.shape):
        raise ValueError("clip_scores: T, A and R must have the same [n, D] shape")
    if out is None:
        out = torch.empty(3 * n + 3, dtype=torch.float64, device=A.device)
    elif out.numel() != 3 * n + 3:
        raise ValueError(f"clip_scores: out has {out.numel()} values, expected {3 * n + 3}")
    st = lib.sdmoe_clip_scores(tp, ldt, ap, lda, rp, ldr, n, D, _dev(out, "out", torch.float64), _stream())
    _lib.check(st, "sdmoe_clip_scores")
    return out


IMAGENET_MEAN = (0.485, 0.456, 0.406)   # torchvision ImageClassification preset
IMAGENET_STD = (0.229, 0.224, 0.225)
STEM_K, STEM_KPAD = 147, 192  # 3 x 7 x 7 taps, padded to the GEMM's K granule (64)


def stem_rows(u8, out=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """u8 [B, S, S, 3] uint8 -> fp16 [B * So^2, STEM_KPAD], So = (S - 1) // 2 + 1: the normalised im2col rows of the
    7x7 / stride 2 / padding 3 stem (sdmoe_stem_rows); the stem is then linear(rows, w[64, STEM_KPAD], act=ACT_RELU)."""
    lib = _lib.load()
    if u8.dim() != 4 or u8.shape[3] != 3 or u8.shape[1] != u8.shape[2]:
        raise ValueError(f"stem_rows: expected [B, S, S, 3] uint8, got {tuple(u8.shape)}")
    B, S = u8.shape[0], u8.shape[1]
    So = (S - 1) // 2 + 1
    if out is None:
        out = torch.empty((B * So * So, STEM_KPAD), dtype=torch.float16, device=u8.device)
    op, lda = _rows(out, "out")
    if out.shape[0] != B * So * So or out.shape[1] < STEM_K:
        raise ValueError(f"stem_rows: out {tuple(out.shape)} is not [{B * So * So}, >= {STEM_K}]")
    f3 = ctypes.c_float * 3
    st = lib.sdmoe_stem_rows(_dev(u8, "u8", torch.uint8), B, S, f3(*mean), f3(*std), op, lda, out.shape[1], _stream())
    _lib.check(st, "sdmoe_stem_rows")
    return out


def maxpool3x3s2(x, nimg, H, W, out=None):
    """F.max_pool2d(x, 3, 2, 1) on NHWC x viewed as [nimg*H*W, C] -> [nimg*OH*OW, C] (sdmoe_maxpool3x3s2)."""
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    C = x.shape[1]
    if x.shape[0] != nimg * H * W:
        raise ValueError("maxpool3x3s2: rows != nimg*H*W")
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((nimg * OH * OW, C), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    if tuple(out.shape) != (nimg * OH * OW, C):
        raise ValueError(f"maxpool3x3s2: out {tuple(out.shape)} is not {(nimg * OH * OW, C)}")
    _lib.check(lib.sdmoe_maxpool3x3s2(xp, ldx, nimg, H, W, C, op, ldy, _stream()), "sdmoe_maxpool3x3s2")
    return out


def avgpool_rows(x, nimg, HW, out=None):
    """[nimg*HW, C] -> [nimg, C]: per image and channel fp16(fp32 sum in row order / HW) (sdmoe_avgpool_rows)."""
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    C = x.shape[1]
    if x.shape[0] != nimg * HW:
        raise ValueError("avgpool_rows: rows != nimg*HW")
    if out is None:
        out = torch.empty((nimg, C), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    if tuple(out.shape) != (nimg, C):
        raise ValueError(f"avgpool_rows: out {tuple(out.shape)} is not {(nimg, C)}")
    _lib.check(lib.sdmoe_avgpool_rows(xp, ldx, nimg, HW, C, op, ldy, _stream()), "sdmoe_avgpool_rows")
    return out


def add_relu(a, b, out=None):
    """out = relu(a + b) on contiguous fp16 tensors of one shape, any element count; out may be a or b
    (sdmoe_add_relu)."""
    lib = _lib.load()
    if a.shape != b.shape:
        raise ValueError(f"add_relu: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    if out is None:
        out = torch.empty_like(a)
    elif out.shape != a.shape:
        raise ValueError(f"add_relu: out {tuple(out.shape)} is not {tuple(a.shape)}")
    st = lib.sdmoe_add_relu(_dev(a, "a"), _dev(b, "b"), _dev(out, "out"), a.numel(), _stream())
    _lib.check(st, "sdmoe_add_relu")
    return out


def topk_hits(logits, table, label, k=5):
    """Top-k classes of fp16 logits [n, C] and their match against a label bit table (sdmoe_topk_hits): table uint32
    words [G, ceil(C / 32)] held as an int32 device tensor, label int32 [n]. Returns device int32 tensors (topk [n, k]
    descending, ties to the lower id, NaN first; hit [n]; total [1]); a label outside [0, G) gives hit -1 and total -1."""
    lib = _lib.load()
    lp, ldl = _rows(logits, "logits")
    n, C = logits.shape
    if not 1 <= k <= min(C, 8):
        raise ValueError(f"topk_hits: k={k} is not in [1, min(C={C}, 8)]")
    if table.dim() != 2 or table.shape[1] != (C + 31) // 32:
        raise ValueError(f"topk_hits: table {tuple(table.shape)} is not [G, {(C + 31) // 32}]")
    if label.numel() != n:
        raise ValueError(f"topk_hits: {label.numel()} labels for {n} rows")
    topk = torch.empty((n, k), dtype=torch.int32, device=logits.device)
    hit = torch.empty(n, dtype=torch.int32, device=logits.device)
    total = torch.empty(1, dtype=torch.int32, device=logits.device)
    st = lib.sdmoe_topk_hits(lp, ldl, n, C, k, _dev(table, "table", torch.int32), table.shape[0],
                             _dev(label, "label", torch.int32), topk.data_ptr(), hit.data_ptr(), total.data_ptr(),
                             _stream())
    _lib.check(st, "sdmoe_topk_hits")
    return topk, hit, total


POOL_MAX_D = 2048  # sdmoe_text_pool / sdmoe_concept_route: 256 chunks of 8 columns


def _pool_rows(X, nseq, name):
    """(ptr, row stride, L, D) of fp16 hidden-state rows [nseq * L, D] (a row-strided or offset view is fine)."""
    xp, ldx = _rows(X, name)
    rows, D = X.shape
    if nseq <= 0 or rows % nseq or rows == 0:
        raise ValueError(f"{name}: {rows} rows are not {nseq} whole sequences")
    if not 1 <= D <= POOL_MAX_D:
        raise ValueError(f"{name}: D = {D} is outside 1..{POOL_MAX_D}")
    return xp, ldx, rows // nseq, D


def text_pool(X, nseq, group=1, renorm=False, out=None):
    """Unit mean features of text-encoder rows (sdmoe_text_pool): X fp16 [nseq * L, D] -> float64 [nseq / group, D];
    per sequence f = mean of its L rows / its norm (no epsilon: an all-zero block gives NaN), then the mean of every
    `group` consecutive f, re-normalised if renorm. float64, fixed order: bit-identical from run to run."""
    xp, ldx, L, D = _pool_rows(X, int(nseq), "X")
    group = int(group)
    if group <= 0 or nseq % group:
        raise ValueError(f"text_pool: {nseq} sequences are not whole groups of {group}")
    if out is None:
        out = torch.empty((nseq // group, D), dtype=torch.float64, device=X.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (nseq // group, D):
        raise ValueError(f"out must be float64 [{nseq // group}, {D}], got {out.dtype} {tuple(out.shape)}")
    op = _dev(out, "out", torch.float64)
    st = _lib.load().sdmoe_text_pool(xp, ldx, int(nseq), L, D, group, int(bool(renorm)), op, out.stride(0), _stream())
    _lib.check(st, "sdmoe_text_pool")
    return out


def concept_groups(groups, R, device=None):
    """The group table of concept_route from host records (row0, row1, neg_row, anchor_row or -1, threshold or None /
    -inf), checked against the R bank rows: int32 [G, 6] in sdmoe_concept_group's layout (four ints and the bits of
    the float64 threshold), on `device` if given."""
    import numpy as np
    rec = np.zeros(len(groups), dtype=np.dtype([("rows", "<i4", 4), ("thr", "<f8")]))
    for g, (row0, row1, neg, anchor, thr) in enumerate(groups):
        row0, row1, neg, anchor = int(row0), int(row1), int(neg), -1 if anchor is None else int(anchor)
        if not 0 <= row0 < row1 <= R or not 0 <= neg < R or not -1 <= anchor < R:
            raise ValueError(f"group {g}: rows ({row0}, {row1}, {neg}, {anchor}) do not fit a bank of {R} rows")
        rec[g] = ((row0, row1, neg, anchor), float("-inf") if thr is None else float(thr))
    t = torch.from_numpy(rec.view("<i4").reshape(len(groups), 6).copy())
    return t if device is None else t.to(device)


def concept_route(X, nprompt, bank, row_bit, groups, preset=None, select_out=None, sims_out=None, sims=True):
    """Per-prompt select words from text-encoder rows in one launch (sdmoe_concept_route). X fp16 [nprompt * L, D];
    bank float64 [R, D] (text_pool rows); row_bit int32 [R] (the select bit of each bank row, -1 = none): a host
    sequence (checked here, uploaded) or a device tensor the caller has checked; groups: host records (concept_groups
    checks and uploads them) or its int32 [G, 6] device tensor; preset: optional int32 [nprompt] words OR-ed in first.
    Returns (select int32 [nprompt] -- bit patterns of uint32 words, the operand of wmask_union_sets --, sims float64
    [nprompt, R] or None with sims=False)."""
    nprompt = int(nprompt)
    if bank.dim() != 2 or bank.shape[0] < 1 or bank.dtype != torch.float64:
        raise ValueError(f"bank must be float64 [R >= 1, D], got {bank.dtype} {tuple(bank.shape)}")
    R = bank.shape[0]
    # the host forms are checked before anything touches the device
    if not isinstance(row_bit, torch.Tensor):
        bits = [int(v) for v in row_bit]
        if len(bits) != R or any(v < -1 or v > 31 for v in bits):
            raise ValueError(f"row_bit must hold {R} bits in -1..31, got {bits}")
        row_bit = torch.tensor(bits, dtype=torch.int32)
    elif row_bit.dtype != torch.int32 or tuple(row_bit.shape) != (R,):
        raise ValueError(f"row_bit must be int32 [{R}], got {row_bit.dtype} {tuple(row_bit.shape)}")
    if not isinstance(groups, torch.Tensor):
        groups = concept_groups(list(groups), R)
    elif groups.dtype != torch.int32 or groups.dim() != 2 or groups.shape[1] != 6:
        raise ValueError(f"groups must be int32 [G, 6] (concept_groups), got {groups.dtype} {tuple(groups.shape)}")
    xp, ldx, L, D = _pool_rows(X, nprompt, "X")
    dev = X.device
    if bank.shape[1] != D or (bank.stride(1) != 1 and D > 1) or not bank.is_cuda:
        raise ValueError(f"bank must be a device tensor [R, {D}] with contiguous rows, got {tuple(bank.shape)} on "
                         f"{bank.device}")
    row_bit, groups = row_bit.to(dev), groups.to(dev)
    G = groups.shape[0]
    if preset is not None and (preset.dtype != torch.int32 or tuple(preset.shape) != (nprompt,)):
        raise ValueError(f"preset must be int32 [{nprompt}], got {preset.dtype} {tuple(preset.shape)}")
    if select_out is None:
        select_out = torch.empty(nprompt, dtype=torch.int32, device=dev)
    elif select_out.dtype != torch.int32 or tuple(select_out.shape) != (nprompt,):
        raise ValueError(f"select_out must be int32 [{nprompt}], got {select_out.dtype} {tuple(select_out.shape)}")
    if sims_out is None and sims:
        sims_out = torch.empty((nprompt, R), dtype=torch.float64, device=dev)
    elif sims_out is not None and (sims_out.dtype != torch.float64 or tuple(sims_out.shape) != (nprompt, R)):
        raise ValueError(f"sims_out must be float64 [{nprompt}, {R}], got {sims_out.dtype} {tuple(sims_out.shape)}")
    st = _lib.load().sdmoe_concept_route(
        xp, ldx, nprompt, L, D, bank.data_ptr(), bank.stride(0), R, _dev(row_bit, "row_bit", torch.int32),
        _dev(groups, "groups", torch.int32) if G else None, G,
        None if preset is None else _dev(preset, "preset", torch.int32), _dev(select_out, "select_out", torch.int32),
        None if sims_out is None else _dev(sims_out, "sims_out", torch.float64), _stream())
    _lib.check(st, "sdmoe_concept_route")
    return select_out, sims_out


def expert_mean_topk(score, k: int, rows_per_img: int = 0, row_idx=None, mean_out=None, topk_out=None):
    """GetExperts statistic (get_experts.py:72-80): mean of the fp16 expert scores [M, E] over all tokens, or
    over positions row_idx (int32 device tensor) of every rows_per_img-row image, then the top-k expert ids
    (descending, ties -> lowest id) as int32 [k]."""
    lib = _lib.load()
    sp, lds = _rows(score, "score")
    M, E = score.shape
    if topk_out is None:
        topk_out = torch.empty(int(k), dtype=torch.int32, device=score.device)
    rp, n_idx = (None, 0) if row_idx is None else (_dev(row_idx, "row_idx", torch.int32), row_idx.numel())
    ws = _workspace(score.device)
    st = lib.sdmoe_expert_mean_topk(sp, lds, M, E, int(rows_per_img), rp, n_idx, int(k),
                                    None if mean_out is None else _dev(mean_out, "mean_out"),
                                    _dev(topk_out, "topk_out", torch.int32), ws.data_ptr(), ws.numel(), _stream())
    _lib.check(st, "sdmoe_expert_mean_topk")
    return topk_out


def expert_stats(score, *, sel=None, rows_per_img=0, img_group=None, ngroups=1, colmax=None, count=None,
                 workspace=None):
    """Expert-level statistics of one routed call (sdmoe_expert_stats) over score [M, E] fp16 (a row-strided view is
    fine) and sel (optional int32 [M, ceil(E / 32)], the sel_out of the routing kernels): colmax (optional fp16
    [ngroups, E]) receives the maximum of each score column over the rows of the images of each group (image i =
    rows_per_img rows, group img_group[i], int32 device [M / rows_per_img]; None = all group 0; rows_per_img 0 = one
    image), count (optional int32 [M / rows_per_img, E]) the number of rows of each image whose sel bit is set.
    workspace: fp32 scratch for the per-slab partials (default: the device's shared workspace). Returns
    (colmax, count)."""
    lib = _lib.load()
    sp, lds = _rows(score, "score")
    M, E = score.shape
    if int(rows_per_img) < 0:
        raise ValueError(f"expert_stats: rows_per_img = {int(rows_per_img)}")
    selp = cp = cntp = None
    if sel is not None:
        if tuple(sel.shape) != (M, (E + 31) // 32):
            raise ValueError(f"expert_stats: sel {tuple(sel.shape)} is not {(M, (E + 31) // 32)}")
        selp = _dev(sel, "sel", torch.int32)
    if colmax is not None:
        if tuple(colmax.shape) != (int(ngroups), E):
            raise ValueError(f"expert_stats: colmax {tuple(colmax.shape)} is not {(int(ngroups), E)}")
        cp = _dev(colmax, "colmax")
    rpi, nimg, igp = _image_groups("expert_stats", M, rows_per_img, img_group if colmax is not None else None,
                                   one=min(M, 1))
    if count is not None:
        if (rpi <= 0 or M % rpi == 0) and tuple(count.shape) != (nimg, E):
            raise ValueError(f"expert_stats: count {tuple(count.shape)} is not {(nimg, E)}")
        cntp = _dev(count, "count", torch.int32)
    st = lib.sdmoe_expert_stats(sp, lds, selp, M, E, rpi, igp, int(ngroups), cp, cntp,
                                *_ws_args(score.device, workspace), _stream())
    _lib.check(st, "sdmoe_expert_stats")
    return colmax, count


def colnorm_accum(P, sumsq):
    """Wanda column statistic (wanda_receiver.py:37-57): sumsq[f] += sum_m (P[m,f] / ||P[m,:]||_2)^2."""
    lib = _lib.load()
    pp, ldp = _rows(P, "P")
    M, F = P.shape
    if sumsq.numel() != F:
        raise ValueError(f"colnorm_accum: sumsq has {sumsq.numel()} entries, P has {F} columns")
    ws = _workspace(P.device)
    st = lib.sdmoe_colnorm_accum(pp, ldp, M, F, _dev(sumsq, "sumsq", torch.float32), ws.data_ptr(), ws.numel(),
                                 _stream())
    _lib.check(st, "sdmoe_colnorm_accum")
    return sumsq


def wanda_mask(W, norm_base, norm_adj, kprune: int, out=None):
    """modularity/wanda.py:140-160 on device: bit-packed [C, F/8] mask of (top-kprune of |W|*norm_adj per row)
    AND (|W|*norm_adj > |W|*norm_base); norms fp16 [F]."""
    lib = _lib.load()
    wp, ldw = _rows(W, "W")
    C, F = W.shape
    if out is None:
        out = torch.empty((C, F // 8), dtype=torch.uint8, device=W.device)
    st = lib.sdmoe_wanda_mask(wp, ldw, C, F, _dev(norm_base, "norm_base"), _dev(norm_adj, "norm_adj"), int(kprune),
                              _dev(out, "bits", torch.uint8), _stream())
    _lib.check(st, "sdmoe_wanda_mask")
    return out


def timestep_embedding(t: float, dim: int, device, flip_sin_to_cos=True, freq_shift=0.0, out=None, t_dev=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty((1, dim), dtype=torch.float16, device=device)
    st = lib.sdmoe_timestep_embedding(out.data_ptr(), _ptr(t_dev), float(t), dim, int(flip_sin_to_cos),
                                      float(freq_shift), _stream())
    _lib.check(st, "sdmoe_timestep_embedding")
    return out


def timestep_embedding_rows(t_dev: torch.Tensor, dim: int, out: torch.Tensor, group: int = 1,
                            flip_sin_to_cos=True, freq_shift=0.0):
    """Sinusoids of t_dev (fp32 [n]) into `out` (2-D fp16 view): row r at out[r // group, (r % group)*dim:]."""
    lib = _lib.load()
    op, ldo = _rows(out, "out")
    n = t_dev.numel()
    if out.shape[0] * group < n or out.shape[1] < group * dim:
        raise ValueError("timestep_embedding_rows: output view too small")
    st = lib.sdmoe_timestep_embedding_rows(op, ldo, _dev(t_dev, "t_dev", torch.float32), n, group, dim,
                                           int(bool(flip_sin_to_cos)), float(freq_shift), _stream())
    _lib.check(st, "sdmoe_timestep_embedding_rows")
    return out


def prepare_input(lat: torch.Tensor, out: torch.Tensor, ncopy: int):
    lib = _lib.load()
    B, C, H, W = lat.shape
    op, ldo = _rows(out, "out")
    st = lib.sdmoe_prepare_input(_dev(lat, "lat", torch.float32), op, B, H * W, ldo, ncopy, _stream())
    _lib.check(st, "sdmoe_prepare_input")
    return out


def cfg_ddim_step(eps: torch.Tensor, lat: torch.Tensor, do_cfg: bool, guidance: float, alpha_t: float,
                  alpha_prev: float, next_in: torch.Tensor | None = None):
    lib = _lib.load()
    B, C, H, W = lat.shape
    ep, lde = _rows(eps, "eps")
    np_, ldn = (None, 0) if next_in is None else _rows(next_in, "next_in")
    st = lib.sdmoe_cfg_ddim_step(ep, lde, _dev(lat, "lat", torch.float32), B, H * W, int(bool(do_cfg)),
                                 float(guidance), float(alpha_t), float(alpha_prev), np_, ldn, _stream())
    _lib.check(st, "sdmoe_cfg_ddim_step")
    return lat


def cfg_multistep_step(eps: torch.Tensor, lat: torch.Tensor, do_cfg: bool, guidance: float, hist: torch.Tensor,
                       cur: torch.Tensor, coef, flags, next_in: torch.Tensor | None = None):
    """CFG + one PLMS (PNDM) update in place (pipeline.pndm_schedule gives coef[7] / flags[3] per call)."""
    import ctypes
    lib = _lib.load()
    B, C, H, W = lat.shape
    if tuple(hist.shape) != (4, B, C, H, W) or tuple(cur.shape) != (B, C, H, W):
        raise ValueError("cfg_multistep_step: history [4, B, 4, H, W] and cur [B, 4, H, W] expected")
    ep, lde = _rows(eps, "eps")
    np_, ldn = (None, 0) if next_in is None else _rows(next_in, "next_in")
    cf = (ctypes.c_float * 7)(*[float(v) for v in coef])
    fl = (ctypes.c_int * 3)(*[int(v) for v in flags])
    st = lib.sdmoe_cfg_multistep_step(ep, lde, _dev(lat, "lat", torch.float32), B, H * W, int(bool(do_cfg)),
                                      float(guidance), _dev(hist, "hist", torch.float32),
                                      _dev(cur, "cur", torch.float32), ctypes.cast(cf, ctypes.c_void_p),
                                      ctypes.cast(fl, ctypes.c_void_p), np_, ldn, _stream())
    _lib.check(st, "sdmoe_cfg_multistep_step")
    return lat


def prepare_input_scaled(lat: torch.Tensor, out: torch.Tensor, ncopy: int, lat_scale: float, in_scale: float):
    """lat *= lat_scale in place (latents * scheduler.init_noise_sigma), then out = fp16(lat * in_scale) for ncopy
    copies (the first step's scale_model_input): prepare_input for the sigma schedulers."""
    lib = _lib.load()
    B, C, H, W = lat.shape
    op, ldo = _rows(out, "out")
    st = lib.sdmoe_prepare_input_scaled(_dev(lat, "lat", torch.float32), op, B, H * W, ldo, ncopy, float(lat_scale),
                                        float(in_scale), _stream())
    _lib.check(st, "sdmoe_prepare_input_scaled")
    return out


def cfg_x0_step(eps: torch.Tensor, lat: torch.Tensor, do_cfg: bool, guidance: float, prev_x0: torch.Tensor | None,
                coef, flags, next_in: torch.Tensor | None = None):
    """CFG + one Euler / DPM-Solver++ 2M update in place (pipeline.euler_schedule / dpmpp_2m_schedule give coef[6] =
    [cx, cm, a, b0, b1, in_scale] and flags[2] = [use_prev, store_prev] per step). prev_x0 [B, 4, H, W] fp32 may be None
    when both flags are 0."""
    import ctypes
    lib = _lib.load()
    B, C, H, W = lat.shape
    if prev_x0 is not None and tuple(prev_x0.shape) != (B, C, H, W):
        raise ValueError("cfg_x0_step: prev_x0 [B, 4, H, W] expected")
    ep, lde = _rows(eps, "eps")
    np_, ldn = (None, 0) if next_in is None else _rows(next_in, "next_in")
    cf = (ctypes.c_float * 6)(*[float(v) for v in coef])
    fl = (ctypes.c_int * 2)(*[int(v) for v in flags])
    pp = None if prev_x0 is None else _dev(prev_x0, "prev_x0", torch.float32)
    st = lib.sdmoe_cfg_x0_step(ep, lde, _dev(lat, "lat", torch.float32), B, H * W, int(bool(do_cfg)),
                               float(guidance), pp, ctypes.cast(cf, ctypes.c_void_p),
                               ctypes.cast(fl, ctypes.c_void_p), np_, ldn, _stream())
    _lib.check(st, "sdmoe_cfg_x0_step")
    return lat


def softmax_rows(x, out=None):
    """Row softmax of a 2-D fp16 view (fp32 max / sum), sdmoe_softmax_rows."""
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    R, N = x.shape
    if out is None:
        out = torch.empty((R, N), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    _lib.check(lib.sdmoe_softmax_rows(xp, ldx, op, ldy, R, N, _stream()), "sdmoe_softmax_rows")
    return out


def transpose(x, out=None):
    """[R, C] fp16 view -> contiguous [C, R] (sdmoe_transpose)."""
    lib = _lib.load()
    xp, ldx = _rows(x, "x")
    R, C = x.shape
    if out is None:
        out = torch.empty((C, R), dtype=torch.float16, device=x.device)
    op, ldy = _rows(out, "out")
    _lib.check(lib.sdmoe_transpose(xp, ldx, op, ldy, R, C, _stream()), "sdmoe_transpose")
    return out


def add(a, b, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(a)
    st = lib.sdmoe_add(_dev(a, "a"), _dev(b, "b"), _dev(out, "out"), a.numel(), _stream())
    _lib.check(st, "sdmoe_add")
    return out


def gather_rows(table, idx, *, add=None, period=0, out=None):
    """out[r] = table[idx[r]] (+ add[r % period]) — token + position embedding, pooled-row gather
    (sdmoe_gather_rows). idx: int32 device tensor [R]."""
    lib = _lib.load()
    tp, ldt = _rows(table, "table")
    C = table.shape[1]
    R = idx.numel()
    if out is None:
        out = torch.empty((R, C), dtype=torch.float16, device=table.device)
    op, ldo = _rows(out, "out")
    ap, lda = (None, 0) if add is None else _rows(add, "add")
    if add is not None and period <= 0:
        period = add.shape[0]
    st = lib.sdmoe_gather_rows(tp, ldt, _dev(idx, "idx", torch.int32), R, C, ap, lda, int(period), op, ldo,
                               _stream())
    _lib.check(st, "sdmoe_gather_rows")
    return out


def attention_short(q, k, v, nseq, N, heads, out=None, scale=None, causal=True):
    """Short-sequence (N <= 128) attention per (sequence, head), optional causal mask (sdmoe_attention_short)."""
    lib = _lib.load()
    qp, ldq = _rows(q, "q")
    kp, ldk = _rows(k, "k")
    vp, ldv = _rows(v, "v")
    C = q.shape[1]
    d = C // heads
    if out is None:
        out = torch.empty((nseq * N, C), dtype=torch.float16, device=q.device)
    op, ldo = _rows(out, "out")
    if scale is None:
        scale = d ** -0.5
    st = lib.sdmoe_attention_short(qp, ldq, kp, ldk, vp, ldv, op, ldo, nseq, N, heads, d, float(scale),
                                   int(bool(causal)), _stream())
    _lib.check(st, "sdmoe_attention_short")
    return out
