"""The normalisations on offset and outlier activations, on every arithmetically different path.

The other normalisation tests draw randn * s + m with |m| / s <= 4. Here (norm_cases.py) a group or a row sits up to
64 standard deviations off zero, one channel or one element carries an outlier (among them the element the shifted
sums take their reference from), a group is constant or alternates +-60000, and the images of one call differ
so that one image's statistics or folded weights on another's rows show. Reference: the fp64 one of norm_cases.
Bars: the suite's own through close() -- scaled max error 2e-3 on x * scale + shift, 5e-3 on normalised activations,
1e-2 behind a GEMM or conv, relative L2 2e-3 everywhere. test_norm_cases.py shows on the CPU that the number formats
and the formulation of each path stay within half of its bar on every case it is held to here; a case outside a
path's table (norm_cases.GN_EXCLUDED, GN_FOLD_EXCLUDED, LN_FOLD_ADMITTED) only has to come out finite, and its measured
error is printed.

Paths: gn_small_kernel, gn_partial_kernel<1|2> + gn_finalize_kernel (groupnorm_stats); gn_fused_reg_kernel<4|8|16>,
gn_fused_kernel and gn_small + apply (groupnorm, knob gn_fused 1 / 2 / 0); the GroupNorm inside sdmoe_conv3x3_gn and
its apply + conv fall-back; sdmoe_gn_fold + sdmoe_linear_per_image; layernorm_kernel at its 13 widths and two block
sizes; the LayerNorm folded into the GEMM (sdmoe_linear_ln, sdmoe_linear_geglu_ln)."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from sdmoe import _lib, ops, tune  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402
from test_gpu_kernels import close  # noqa: E402

DEV = "cuda"
GN_CASES = nc.gn_cases()
GN_IDS = [nc.gn_case_id(c) for c in GN_CASES]
GN_INDEX = list(range(len(GN_CASES)))
GN_WIDE = [i for i in GN_INDEX if GN_CASES[i][0] in ("group_offset", "ref_outlier", "mixed_images")]
LN_CASES = nc.ln_cases()
LN_IDS = [c[0] for c in LN_CASES]
SENTINEL = 0x7B2D  # a finite fp16 bit pattern (~58,784) no path produces here
JUNK = 1.0e4


@functools.lru_cache(maxsize=64)
def _gn(i, C, HW):
    """(x, gamma, beta, nimg) on the device; x is columns [64, 64 + C) of a buffer whose other columns hold 1e4"""
    fam, cid, fn, args = GN_CASES[i]
    x, gamma, beta, nimg = fn(C, HW, *args)
    buf = torch.full((x.shape[0], C + 72), JUNK, dtype=torch.float16, device=DEV)
    buf[:, 64:64 + C] = x.to(DEV)
    return buf[:, 64:64 + C], gamma.to(DEV), beta.to(DEV), nimg


def _held(out, ref, tol, what, admitted=True):
    """print the measured figures, then the bar (admitted) or finiteness alone"""
    rel, mx = nc.errors(out, ref)
    print(f"NORM {what}: rel L2 {rel:.3e} scaled max err {mx:.3e}{'' if admitted else ' (not held to the bar)'}")
    assert torch.isfinite(out).all()
    if admitted:
        close(out.double(), ref, tol=tol)


# ---- GroupNorm statistics ------------------------------------------------------------------------------------------

def _stats(i, C, HW, path):
    x, gamma, beta, nimg = _gn(i, C, HW)
    sc, sh = ops.groupnorm_stats(x, nimg, HW, gamma, beta, nc.GN_EPS, nc.GROUPS)
    ref = nc.gn_exact(x, nimg, HW, gamma, beta)
    _held(nc.gn_apply_stats(x, nimg, HW, sc.double(), sh.double()), ref, nc.TOL_STATS,
          f"stats {path} {GN_IDS[i]} C={C} HW={HW}", GN_IDS[i] not in nc.GN_EXCLUDED)


@pytest.mark.parametrize("HW", (64, 1024))
@pytest.mark.parametrize("i", GN_INDEX, ids=GN_IDS)
def test_groupnorm_stats_single_launch(i, HW):
    """gn_small_kernel: shifted sums around a reference from row 0 of the group (gn_ref), fp64 finalize"""
    _stats(i, 320, HW, "small")


@pytest.mark.parametrize("i", GN_INDEX, ids=GN_IDS)
def test_groupnorm_stats_partial_finalize(i):
    """gn_partial_kernel<1> over 64 slices of 17 rows + gn_finalize_kernel (HW = 1088 > 1024)"""
    _stats(i, 320, 1088, "partial<1>")


@pytest.mark.parametrize("i", GN_WIDE, ids=[GN_IDS[i] for i in GN_WIDE])
def test_groupnorm_stats_partial_finalize_wide(i):
    """gn_partial_kernel<2> (C / 8 = 320 chunks > 256 threads: two virtual threads each), C = 2560: groups of
    87040 elements, the most of this file. With the outlier of ref_outlier as the only reference of the shifted sums
    the statistics were 3.1e-3 (d = 1000) and 4.0e-3 (d = 60000) off, scaled max error, against the bar of 2e-3."""
    _stats(i, 2560, 1088, "partial<2>")


# ---- GroupNorm, single launch and two launches ----------------------------------------------------------------------

@pytest.mark.parametrize("C,HW", [(320, 64), (320, 192), (320, 256), (576, 64)])
@pytest.mark.parametrize("i", GN_INDEX, ids=GN_IDS)
def test_groupnorm_every_variant(i, C, HW):
    """ops.groupnorm with and without SiLU under gn_fused = 1 (register-resident: 80-channel chunks, 25 row phases, so
    HW = 64 / 192 / 256 take 3 / 8 / 11 rows per thread: <4>, <8>, <16>; C = 576: 144-channel chunks, nq = 18 > 16),
    2 (gn_fused_kernel) and 0 (gn_small_kernel + apply): each within the bar, the three bit-identical, the output a
    view into a sentinel-filled buffer whose guard columns stay untouched, the input a slice of a buffer of 1e4."""
    x, gamma, beta, nimg = _gn(i, C, HW)
    rows = nimg * HW
    for silu in (False, True):
        ref = nc.gn_exact(x, nimg, HW, gamma, beta, act=silu)
        bufs = []
        for mode in (1, 2, 0):
            buf = torch.full((rows, C + 16), SENTINEL, dtype=torch.int16, device=DEV)
            out = buf.view(torch.float16)[:, 8:8 + C]
            with tune.tuned(gn_fused=mode):
                ops.groupnorm(x, nimg, HW, gamma, beta, nc.GN_EPS, nc.GROUPS, silu, out=out)
            bufs.append(buf)
        assert torch.equal(bufs[0], bufs[2]) and torch.equal(bufs[1], bufs[2])
        assert (bufs[0][:, :8] == SENTINEL).all() and (bufs[0][:, 8 + C:] == SENTINEL).all()
        out = bufs[0].view(torch.float16)[:, 8:8 + C]
        _held(out, ref, nc.TOL_NORM, f"groupnorm {GN_IDS[i]} C={C} HW={HW} silu={int(silu)}",
              GN_IDS[i] not in nc.GN_EXCLUDED)
        if GN_IDS[i] == "constant_group-all-2" and not silu:
            # variance exactly 0: the output is beta, up to the fp32 rounding of shift = beta - 2 * 316 gamma
            # (half an ulp of 700, 3e-5), that of scale (2 * 316 * 2^-24, 4e-5) and the fp16 rounding of the
            # output (|beta| < 0.5: 1.2e-4)
            assert (out.double() - beta.double()).abs().max().item() <= 2e-4
    assert (x._base[:, :64] == JUNK).all() and (x._base[:, 64 + C:] == JUNK).all()  # the input is only read


# ---- GroupNorm (+ SiLU) in front of the 3x3 conv ---------------------------------------------------------------------

@pytest.mark.parametrize("H,W,fused", [(4, 64, True), (16, 16, False)])
@pytest.mark.parametrize("i", GN_INDEX, ids=GN_IDS)
def test_conv3x3_groupnorm(i, H, W, fused):
    """ops.conv3x3(..., gn=(scale, shift, silu)) at Cin = Cout = 320 on 256 pixels per image: 4 x 64, which
    sdmoe_conv3x3_gn normalises itself in the staged halo (it takes 64-wide images only), and 16 x 16, which it
    refuses, so that the apply pass + plain conv run. Reference: fp64 GroupNorm + SiLU + conv."""
    C = 320
    x, gamma, beta, nimg = _gn(i, C, H * W)
    if fused:
        assert ops.conv_gn_fusable(H, W, C, C) and ops.conv_plan(nimg, H, W, C, C, gn=True)["halo"]
    else:
        with pytest.raises(_lib.SdmoeError):
            ops.conv_plan(nimg, H, W, C, C, gn=True)
    w, b = (t.to(DEV) for t in nc.conv_weights(C, C))
    sc, sh = ops.groupnorm_stats(x, nimg, H * W, gamma, beta, nc.GN_EPS, nc.GROUPS)
    out = ops.conv3x3(x, nimg, H, W, ops.conv_weight(w), b, gn=(sc, sh, True))
    ref = nc.conv3x3_exact(nc.gn_exact(x, nimg, H * W, gamma, beta, act=True), nimg, H, W, w, b)
    _held(out, ref, nc.TOL_GEMM, f"conv3x3 gn {'in-kernel' if fused else 'apply+conv'} {GN_IDS[i]}",
          GN_IDS[i] not in nc.GN_EXCLUDED)


# ---- GroupNorm folded into proj_in -----------------------------------------------------------------------------------

@pytest.mark.parametrize("C", (320, 1280))
@pytest.mark.parametrize("i", GN_INDEX, ids=GN_IDS)
def test_gn_fold(i, C):
    """ops.gn_fold + ops.linear_per_image at HW = 256, (C, N) = (320, 320) and (1280, 1280), with and without a
    residual: the full bar on every case the fold's restatement admits, group offsets of 64 std among them, and
    agreement with ops.linear(ops.groupnorm(...))."""
    HW, N = 256, C
    x, gamma, beta, nimg = _gn(i, C, HW)
    admitted = GN_IDS[i] not in nc.GN_FOLD_EXCLUDED
    w, b = (t.to(DEV) for t in nc.linear_weights(N, C))
    sc, sh = ops.groupnorm_stats(x, nimg, HW, gamma, beta, nc.GN_EPS, nc.GROUPS)
    wf, cb = ops.gn_fold(w, b, sc, sh)
    assert (wf[:, :, 3] == 0).all()  # gamma[3] = 0
    out = ops.linear_per_image(x, wf, cb, HW)
    ref = nc.gn_exact(x, nimg, HW, gamma, beta, w=w, bias=b)
    _held(out, ref, nc.TOL_GEMM, f"gn_fold {GN_IDS[i]} C={C}", admitted)
    r = (torch.randn(nimg * HW, N, generator=nc._gen(30, N)) * 2).half().to(DEV)
    _held(ops.linear_per_image(x, wf, cb, HW, residual=r), ref + r.double(), nc.TOL_GEMM,
          f"gn_fold + residual {GN_IDS[i]} C={C}", admitted)
    unf = ops.linear(ops.groupnorm(x, nimg, HW, gamma, beta, nc.GN_EPS, nc.GROUPS), w, b)
    _held(unf, ref, nc.TOL_GEMM, f"groupnorm + linear {GN_IDS[i]} C={C}", GN_IDS[i] not in nc.GN_EXCLUDED)
    _held(out, unf.double(), nc.TOL_GEMM, f"gn_fold vs groupnorm + linear {GN_IDS[i]} C={C}", admitted)


def test_gn_fold_operands_row_tail():
    """sdmoe_gn_fold alone at N = 38 (blocks of four waves, one output row each: the last block is half empty), three
    images with their own statistics, a zero-gamma channel: Wf and the column bias against their definition in fp64,
    at the tolerances of test_gn_fold_proj_in"""
    C, HW, N = 320, 64, 38
    x, gamma, beta, nimg = nc.mixed_images(C, HW)
    w, b = nc.linear_weights(N, C)
    scale, shift = nc.gn_scale_shift(x, nimg, HW, gamma, beta)
    wf, cb = ops.gn_fold(w.to(DEV), b.to(DEV), scale.float().to(DEV), shift.float().to(DEV))
    wref, cref = nc.gn_fold_operands(w, b, scale, shift)
    assert tuple(wf.shape) == (nimg, N, C) and tuple(cb.shape) == (nimg, N)
    close(wf.double().cpu(), wref, rel=1e-3)
    close(cb.double().cpu(), cref, tol=1e-4, rel=1e-5)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------

def _layernorm_guarded(cid, fn, args, M, C):
    """x and out are rows [3, 3 + M) x columns [8, 8 + C) of poisoned buffers: 1e4 around x, a sentinel around out"""
    x, gamma, beta = fn(M, C, *args)
    g = 3
    xb = torch.full((M + 2 * g + 8, C + 16), JUNK, dtype=torch.float16, device=DEV)
    xb[g:g + M, 8:8 + C] = x.to(DEV)
    xv = xb[g:g + M, 8:8 + C]
    buf = torch.full((M + 2 * g + 8, C + 16), SENTINEL, dtype=torch.int16, device=DEV)
    out = buf.view(torch.float16)[g:g + M, 8:8 + C]
    ret = ops.layernorm(xv, gamma.to(DEV), beta.to(DEV), nc.LN_EPS, out=out)
    assert ret.data_ptr() == out.data_ptr()
    ref = nc.ln_exact(xv, gamma.to(DEV), beta.to(DEV))
    _held(out, ref, nc.TOL_NORM, f"layernorm {cid} M={M} C={C}")
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[g:g + M, 8:8 + C] = False
    assert (buf[guard] == SENTINEL).all(), "a store outside the output view"
    return out, ref, beta


@pytest.mark.parametrize("width", nc.LN_WIDTHS)
@pytest.mark.parametrize("case", LN_CASES, ids=LN_IDS)
def test_layernorm_every_width(case, width):
    """layernorm_kernel<C / 64> at M = 77: one-wave blocks of 8 rows, the last with three dead rows (they read row 0)"""
    cid, fn, args = case
    out, ref, beta = _layernorm_guarded(cid, fn, args, 77, 64 * width)
    if cid.startswith("constant_rows"):  # variance 0 in the two-pass statistics: exactly fp16(beta)
        assert torch.equal(out, beta.to(DEV)[None].expand_as(out))


@pytest.mark.parametrize("case", LN_CASES, ids=LN_IDS)
def test_layernorm_wide_blocks(case):
    """M = 32768 + 5 rows at C = 64: the 256-thread blocks of 32 rows, a ragged last block"""
    cid, fn, args = case
    _layernorm_guarded(cid, fn, args, 32768 + 5, 64)


@pytest.mark.parametrize("C,status", [(448, -3), (2112, -2)])
def test_layernorm_refuses_widths_it_has_no_kernel_for(C, status):
    """C / 64 = 7 has no instantiation (unsupported mode); C = 2112 is past the 2048 the registers hold (unsupported
    shape). Nothing is written."""
    x = torch.zeros(16, C, dtype=torch.float16, device=DEV)
    out = torch.full((16, C), SENTINEL, dtype=torch.int16, device=DEV)
    with pytest.raises(_lib.SdmoeError, match=rf"\({status}\)"):
        ops.layernorm(x, torch.ones(C, dtype=torch.float16, device=DEV), torch.zeros(C, dtype=torch.float16, device=DEV),
                      out=out.view(torch.float16))
    assert (out == SENTINEL).all()


# ---- LayerNorm folded into the GEMM ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ln_linear(K):
    w, b = (t.to(DEV) for t in nc.linear_weights(K, K))
    gamma, beta = (t.to(DEV) for t in nc.affine(K))
    return w, b, ops.LNFold(w, gamma, beta, nc.LN_EPS, b)


@pytest.mark.parametrize("M", (1000, 77))
@pytest.mark.parametrize("K", nc.LN_FOLD_K)
@pytest.mark.parametrize("case", LN_CASES, ids=LN_IDS)
def test_linear_ln(case, K, M):
    """sdmoe_linear_ln (one-pass fp32 statistics from fdot2 in the GEMM's main loop), N = K: the full bar on the cases
    LN_FOLD_ADMITTED[K] lists; outside it finite outputs, the measured error printed"""
    cid, fn, args = case
    x, gamma, beta = (t.to(DEV) for t in fn(M, K, *args))
    w, b, fold = _ln_linear(K)
    out = ops.linear_ln(x, fold)
    _held(out, nc.ln_exact(x, gamma, beta, w=w, bias=b), nc.TOL_GEMM, f"linear_ln {cid} K={K} M={M}",
          cid in nc.LN_FOLD_ADMITTED[K])


@functools.lru_cache(maxsize=None)
def _ln_geglu(K):
    F_, E = 4 * K, K // 5
    g = nc._gen(31, K)
    w = (torch.randn(2 * F_, K, generator=g) * K ** -0.5).half().to(DEV)
    b = (torch.randn(2 * F_, generator=g) * 0.3).half().to(DEV)
    routing = ops.Routing(torch.randperm(F_, generator=g) % E, E, 12, DEV)
    gamma, beta = (t.to(DEV) for t in nc.affine(K))
    fold = ops.interleave_ln_fold(ops.LNFold(w, gamma, beta, nc.LN_EPS, b), routing.perm)
    return w, b, routing, fold, F_, E


@pytest.mark.parametrize("M", (1000, 77))
@pytest.mark.parametrize("K", nc.LN_FOLD_K)
@pytest.mark.parametrize("case", LN_CASES, ids=LN_IDS)
def test_linear_geglu_ln(case, K, M):
    """sdmoe_linear_geglu_ln (norm3 folded into the routed projection, F = 4 K, K / 5 experts of 20 neurons, ReLU):
    the product value * act(gate) and the per-expert gate sums, as test_linear_ln"""
    cid, fn, args = case
    x, gamma, beta = (t.to(DEV) for t in fn(M, K, *args))
    w, b, routing, fold, F_, E = _ln_geglu(K)
    score = torch.empty((M, E), dtype=torch.float16, device=DEV)
    P = ops.linear_geglu(x, None, None, ops.ACT_RELU, score=score, esize=routing.esize, ln=fold)
    y = nc.ln_exact(x, gamma, beta, w=w, bias=b)
    perm = routing.perm.to(DEV)
    rows = torch.cat([perm, F_ + perm])
    pref, sref = nc.geglu_exact(y[:, rows], F_, routing.esize)
    admitted = cid in nc.LN_FOLD_ADMITTED[K]
    _held(P, pref, nc.TOL_GEMM, f"geglu_ln P {cid} K={K} M={M}", admitted)
    _held(score, sref, nc.TOL_GEMM, f"geglu_ln score {cid} K={K} M={M}", admitted)
