"""The normalisation numerics cases (norm_cases.py) on the CPU: every case the GPU tests hold a path to the bar on
is one whose format-faithful restatement stays within HALF of that bar against the fp64 reference, every case left
out of a table is one whose restatement does not, and every family does what it is for. No kernel runs here: the
bars and the admitted ranges of test_gpu_norm_numerics.py come from the number formats and the formulations alone.

It also pins the reason for the centred column bias of sdmoe_gn_fold: with the bias taken from the unrounded
weights the restatement leaves the bar at a group offset of 16 standard deviations; with the bias taken from the
rounded weights it stays within half of it up to 64."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402

C, HW, N = 320, 256, 320  # the GroupNorm shape of this file: proj_in of the 16x16 level
GN_CASES = nc.gn_cases()
GN_IDS = [nc.gn_case_id(c) for c in GN_CASES]
LN_CASES = nc.ln_cases()
LN_IDS = [c[0] for c in LN_CASES]


@functools.lru_cache(maxsize=None)
def _gn(i, c=C, hw=HW):
    fam, cid, fn, args = GN_CASES[i]
    return fn(c, hw, *args)


def _show(what, out, ref):
    rel, mx = nc.errors(out, ref)
    print(f"{what}: rel L2 {rel:.2e} scaled max {mx:.2e}")


# ---- GroupNorm ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(GN_CASES)), ids=GN_IDS)
def test_gn_explicit_restatement_is_within_half_the_bar(i):
    """fp32 scale / shift from exact statistics, then one fp16 rounding: the statistics, the normalised activations and
    their SiLU. The one excluded case (a constant 1000) must really be out."""
    x, gamma, beta, nimg = _gn(i)
    ref = nc.gn_exact(x, nimg, HW, gamma, beta)
    sc, sh = nc.gn_scale_shift(x, nimg, HW, gamma, beta)
    stats = nc.gn_apply_stats(x, nimg, HW, sc, sh)
    _show("stats", stats, ref)
    checks = [nc.within(stats, ref, nc.TOL_STATS, 0.5)]
    for act in (False, True):
        out = nc.gn_explicit(x, nimg, HW, gamma, beta, act=act)
        r = nc.gn_exact(x, nimg, HW, gamma, beta, act=act)
        _show(f"explicit silu={act}", out, r)
        checks.append(nc.within(out, r, nc.TOL_NORM, 0.5))
        assert torch.isfinite(out).all()
    if GN_IDS[i] in nc.GN_EXCLUDED:
        assert not any(checks)
    else:
        assert all(checks)


@pytest.mark.parametrize("i", range(len(GN_CASES)), ids=GN_IDS)
def test_gn_fold_restatement_against_its_table(i):
    """Wf = fp16(W scale), the centred fp32 column bias, one fp16 rounding of the output: within half the GEMM bar
    on every case outside GN_FOLD_EXCLUDED, outside half of it on the excluded ones (so the exclusion is the
    formats', not a convenience). The explicit path + linear is shown beside it."""
    x, gamma, beta, nimg = _gn(i)
    w, b = nc.linear_weights(N, C)
    ref = nc.gn_exact(x, nimg, HW, gamma, beta, w=w, bias=b)
    explicit = (nc.gn_explicit(x, nimg, HW, gamma, beta).double() @ w.double().t() + b.double()).half()
    fold = nc.gn_fold_emulate(x, nimg, HW, gamma, beta, w, b)
    _show("explicit + linear", explicit, ref)
    _show("fold", fold, ref)
    assert nc.within(fold, ref, nc.TOL_GEMM, 0.5) == (GN_IDS[i] not in nc.GN_FOLD_EXCLUDED)
    if GN_IDS[i] not in nc.GN_EXCLUDED:
        assert nc.within(explicit, ref, nc.TOL_GEMM, 0.5)


@pytest.mark.parametrize("sigma", nc.SIGMAS)
@pytest.mark.parametrize("rho", nc.RHOS)
def test_gn_fold_bias_from_rounded_weights_is_what_holds_the_bar(rho, sigma):
    """The reason for the fold's centred bias. Not centred (bias + sum W shift, from the UNROUNDED weights), the fp16
    rounding of W scale is multiplied by the activation's mean and nothing cancels it: the restatement leaves the
    full bar at rho >= 16. Centred (bias + sum Wf shift / scale) the rounding multiplies x - mean + beta std / gamma
    and the restatement stays within half the bar at every rho up to 64."""
    x, gamma, beta, nimg = nc.group_offset(C, HW, rho, sigma)
    w, b = nc.linear_weights(N, C)
    ref = nc.gn_exact(x, nimg, HW, gamma, beta, w=w, bias=b)
    old = nc.gn_fold_emulate(x, nimg, HW, gamma, beta, w, b, centred=False)
    new = nc.gn_fold_emulate(x, nimg, HW, gamma, beta, w, b, centred=True)
    _show(f"rho {rho} sigma {sigma} not centred", old, ref)
    _show(f"rho {rho} sigma {sigma} centred", new, ref)
    assert nc.within(new, ref, nc.TOL_GEMM, 0.5)
    if rho >= 16:
        assert not nc.within(old, ref, nc.TOL_GEMM, 1.0)
    else:
        assert nc.within(old, ref, nc.TOL_GEMM, 1.0)


def test_gn_fold_restatement_at_1280():
    """the widest proj_in: K = N = 1280 at rho = 64 and on the three-image mix"""
    w, b = nc.linear_weights(1280, 1280)
    for x, gamma, beta, nimg in (nc.group_offset(1280, HW, 64, 1.0), nc.mixed_images(1280, HW)):
        ref = nc.gn_exact(x, nimg, HW, gamma, beta, w=w, bias=b)
        new = nc.gn_fold_emulate(x, nimg, HW, gamma, beta, w, b)
        _show("K = 1280 centred", new, ref)
        assert nc.within(new, ref, nc.TOL_GEMM, 0.5)


def test_gn_fold_zero_scale_channel():
    """gamma[3] = 0: scale is 0 there, Wf is exactly 0 and the bias keeps the term W shift = W beta"""
    x, gamma, beta, nimg = nc.group_offset(C, HW, 4, 1.0)
    w, b = nc.linear_weights(N, C)
    sc, sh = nc.gn_scale_shift(x, nimg, HW, gamma, beta)
    assert (sc[:, 3] == 0).all() and (sh[:, 3] == beta[3].double()).all()
    wf, cb = nc.gn_fold_operands(w, b, sc, sh)
    assert (wf[:, :, 3] == 0).all() and torch.isfinite(cb).all()
    others = torch.arange(C) != 3
    w0 = w.clone()
    w0[:, 3] = 0
    _, cb0 = nc.gn_fold_operands(w0, b, sc, sh)
    torch.testing.assert_close(cb - cb0, (w[:, 3].double() * beta[3].double())[None].expand(nimg, N), rtol=0, atol=1e-6)
    assert (sc[:, others] != 0).all()


def test_affine_has_negative_and_zero_gamma():
    for c in (320, 576, 1280, 2560):
        gamma, beta = nc.affine(c)
        assert (gamma == 0).sum() == 1 and gamma[3] == 0 and (gamma < 0).sum() >= c // 8 and (gamma > 0.5).sum() > c // 2


def _group_view(x, nimg, hw):
    return x.double().reshape(nimg, hw, nc.GROUPS, -1)


@pytest.mark.parametrize("sigma", nc.SIGMAS)
def test_group_offset_reaches_its_rho(sigma):
    x, _, _, nimg = nc.group_offset(C, HW, 64, sigma)
    mean, var = nc.gn_moments(x, nimg, HW)
    rho = mean.abs() / var.sqrt()
    assert rho.min() >= 60 and rho.max() <= 68
    assert (mean > 0).any() and (mean < 0).any()  # signs differ between the groups
    x0, _, _, _ = nc.group_offset(C, HW, 0, sigma)
    m0, v0 = nc.gn_moments(x0, nimg, HW)
    assert (m0.abs() / v0.sqrt()).max() < 0.1


@pytest.mark.parametrize("d", (16, 256))
def test_channel_offset_sits_where_the_shifted_sums_take_their_reference(d):
    for last in (False, True):
        x, _, _, nimg = nc.channel_offset(C, HW, d, last)
        xg = _group_view(x, nimg, HW)
        col = -1 if last else 0
        assert (xg[..., col] > d - 6).all() and xg[..., 1:-1].abs().max() < 6
        first = xg[:, 0, :, 0]  # row 0, first channel of each group: one of the kernels' reference elements
        assert ((first > d - 6) != last).all()
        mean, var = nc.gn_moments(x, nimg, HW)
        assert (mean.abs() / var.sqrt()).max() < (C // nc.GROUPS) ** 0.5  # benign by construction


@pytest.mark.parametrize("d", (1e3, 6e4))
def test_ref_outlier_puts_the_maximum_at_the_reference(d):
    x, _, _, nimg = nc.ref_outlier(C, HW, d, False)
    xg = _group_view(x, nimg, HW)
    flat = xg.permute(0, 2, 1, 3).reshape(nimg, nc.GROUPS, -1)
    assert (flat.argmax(-1) == 0).all() and (flat[..., 0] == float(torch.tensor(d).half())).all()
    assert flat[..., 1:].abs().max() < 6
    xc, _, _, _ = nc.ref_outlier(C, HW, d, True)
    flatc = _group_view(xc, nimg, HW).permute(0, 2, 1, 3).reshape(nimg, nc.GROUPS, -1)
    r, c = nc.REF_CONTROL
    assert (flatc.argmax(-1) == r * (C // nc.GROUPS) + c).all() and flatc[..., 0].abs().max() < 6


def test_constant_group_has_no_variance_and_normalises_to_beta():
    for level in (1000.0, 2.0):
        x, gamma, beta, nimg = nc.constant_group(C, HW, level, False)
        mean, var = nc.gn_moments(x, nimg, HW)
        assert (var == 0).all() and (mean == level).all()
        ref = nc.gn_exact(x, nimg, HW, gamma, beta)
        assert torch.equal(ref, beta.double()[None].expand(nimg * HW, C))
    x, _, _, nimg = nc.constant_group(C, HW, 1000.0, True)
    assert set(x.unique().tolist()) == {1000.0, 1000.5}
    mean, var = nc.gn_moments(x, nimg, HW)
    assert (mean == 1000.25).all() and (var == 0.0625).all()
    # unshifted one-pass sums in fp32 cannot hold this variance: the sum of squares of a group is 2.6e9, where fp32
    # is spaced by 256, and the variance times n is 160
    n = HW * (C // nc.GROUPS)
    assert n * 1000.25 ** 2 > 2 ** 31 and n * 0.0625 < 256


def test_near_max_is_finite_in_fp32_sums():
    x, gamma, beta, nimg = nc.near_max(C, HW)
    assert (x.abs() == 60000).all()
    mean, var = nc.gn_moments(x, nimg, HW)
    assert (mean == 0).all()
    n = HW * (C // nc.GROUPS)
    assert 1e12 < n * 1.2e5 ** 2 < 3e38  # shifted by a reference of +-60000, the squares are (1.2e5)^2 each


def test_mixed_images_separate_the_images():
    """another image's scale / shift on an image's rows misses the statistics bar by far"""
    x, gamma, beta, nimg = nc.mixed_images(C, HW)
    assert nimg == 3
    ref = nc.gn_exact(x, nimg, HW, gamma, beta)
    sc, sh = nc.gn_scale_shift(x, nimg, HW, gamma, beta)
    assert nc.within(nc.gn_apply_stats(x, nimg, HW, sc, sh), ref, nc.TOL_STATS, 0.5)
    for roll in (1, 2):
        wrong = nc.gn_apply_stats(x, nimg, HW, sc.roll(roll, 0), sh.roll(roll, 0))
        for i in range(nimg):
            rows = slice(i * HW, (i + 1) * HW)
            rel, mx = nc.errors(wrong[rows], ref[rows])
            assert rel > 100 * nc.REL_L2
    w, b = nc.linear_weights(N, C)
    wf, cb = nc.gn_fold_operands(w, b, sc, sh)
    refl = nc.gn_exact(x, nimg, HW, gamma, beta, w=w, bias=b)
    for i in range(nimg):  # image 0's folded operands everywhere: only image 0 comes out right
        rows = slice(i * HW, (i + 1) * HW)
        out = nc.gn_fold_apply(x[rows], 1, HW, wf[:1], cb[:1])
        assert nc.within(out, refl[rows], nc.TOL_GEMM) == (i == 0)


def test_conv3x3_exact_matches_torch():
    g = torch.Generator().manual_seed(3)
    y = torch.randn(2 * 5 * 7, 8, generator=g, dtype=torch.float64)
    w = torch.randn(6, 3, 3, 8, generator=g, dtype=torch.float64)
    b = torch.randn(6, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv2d(y.reshape(2, 5, 7, 8).permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=1)
    torch.testing.assert_close(nc.conv3x3_exact(y, 2, 5, 7, w, b), ref.permute(0, 2, 3, 1).reshape(-1, 6))


# ---- LayerNorm ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", nc.LN_WIDTHS)
def test_ln_explicit_restatement_is_within_half_the_bar(width):
    """two-pass statistics and one fp16 rounding: every case, at every width sdmoe_layernorm instantiates"""
    for cid, fn, args in LN_CASES:
        x, gamma, beta = fn(77, 64 * width, *args)
        ref = nc.ln_exact(x, gamma, beta)
        out = nc.ln_explicit(x, gamma, beta)
        _show(f"{cid} C={64 * width}", out, ref)
        assert nc.within(out, ref, nc.TOL_NORM, 0.5)


def _ln_fold_errors(x, gamma, beta, K):
    w, b = nc.linear_weights(K, K)
    ref = nc.ln_exact(x, gamma, beta, w=w, bias=b)
    out = nc.ln_fold_emulate(x, *nc.ln_fold_operands(w, gamma, beta, b)).half()
    return out, ref


@pytest.mark.parametrize("M", (77, 1000))
@pytest.mark.parametrize("K", nc.LN_FOLD_K)
def test_ln_fold_restatement_against_its_table(K, M):
    """The one-pass fp32 statistics in the GEMM's association, then rstd (acc - mean wsum) + bias_f: within half the
    GEMM bar exactly on the cases LN_FOLD_ADMITTED[K] lists."""
    for cid, fn, args in LN_CASES:
        x, gamma, beta = fn(M, K, *args)
        out, ref = _ln_fold_errors(x, gamma, beta, K)
        _show(f"K={K} M={M} {cid}", out, ref)
        assert torch.isfinite(out).all()
        assert nc.within(out, ref, nc.TOL_GEMM, 0.5) == (cid in nc.LN_FOLD_ADMITTED[K]), cid
        if cid in nc.LN_FOLD_ADMITTED[K]:
            # the routed projection behind the same fold (F = K / 2 here, experts of 20 neurons): the product
            # value * relu(gate) and the per-expert gate sums, each rounded to fp16 once
            w, b = nc.linear_weights(K, K)
            y = nc.ln_fold_emulate(x, *nc.ln_fold_operands(w, gamma, beta, b))
            p, s = nc.geglu_exact(y, K // 2, 20)
            pref, sref = nc.geglu_exact(nc.ln_exact(x, gamma, beta, w=w, bias=b), K // 2, 20)
            _show(f"K={K} M={M} {cid} geglu P", p.half(), pref)
            _show(f"K={K} M={M} {cid} geglu score", s.half(), sref)
            assert nc.within(p.half(), pref, nc.TOL_GEMM, 0.5) and nc.within(s.half(), sref, nc.TOL_GEMM, 0.5), cid


@pytest.mark.parametrize("K", nc.LN_FOLD_K)
def test_ln_fold_first_rho_out_of_half_the_bar(K):
    """where the one-pass variance gives out: the first rho of the ladder at which the restatement leaves half the
    bar, at the larger of the GPU test's two M"""
    first = None
    for rho in nc.RHO_LADDER:
        x, gamma, beta = nc.row_offset(1000, K, rho)
        out, ref = _ln_fold_errors(x, gamma, beta, K)
        _show(f"K={K} rho={rho}", out, ref)
        if first is None and not nc.within(out, ref, nc.TOL_GEMM, 0.5):
            first = rho
    assert first == nc.LN_FOLD_FIRST_RHO_OUT[K]
    assert all(r < first for r in nc.RHOS)


def test_ln_one_pass_sums_are_the_sums():
    x, _, _ = nc.row_offset(77, 640, 16)
    s1, s2 = nc.ln_one_pass_sums(x)
    xd = x.double()
    torch.testing.assert_close(s1[:, 0], xd.sum(-1), rtol=1e-5, atol=0)
    torch.testing.assert_close(s2[:, 0], (xd * xd).sum(-1), rtol=1e-5, atol=0)
    assert (s1.float().double() == s1).all() and (s2.float().double() == s2).all()  # fp32 values


def test_ln_families_do_what_they_are_for():
    M, K = 77, 320
    x, _, _ = nc.row_offset(M, K, 64)
    xd = x.double()
    rho = xd.mean(-1).abs() / xd.std(-1, unbiased=False)
    assert rho.min() >= 55 and (xd.mean(-1) > 0).any() and (xd.mean(-1) < 0).any()
    x, _, _ = nc.massive_channels(M, K)
    xd = x.double()
    assert (xd[:, 7] > 44).all() and (xd[:, K - 3] < -44).all()
    rest = torch.ones(K, dtype=torch.bool)
    rest[[7, K - 3]] = False
    assert xd[:, rest].abs().max() < 6
    x, gamma, beta = nc.constant_rows(M, K)
    xd = x.double()
    assert (xd.var(-1, unbiased=False) == 0).all() and set(xd[:, 0].tolist()) == set(nc.CONSTANTS)
    assert torch.equal(nc.ln_exact(x, gamma, beta), beta.double()[None].expand(M, K))
    x, _, _ = nc.interleaved(M, K)
    xd = x.double()
    std = xd.std(-1, unbiased=False)
    assert (std[2::4] == 0).all() and (xd[2::4] == 2).all()          # constant rows
    assert (std[3::4] > 6).all() and (std[0::4] < 1.3).all()         # N(0, 64) rows and offset rows
    assert (xd[0::4].mean(-1).abs() > 15).all() and (xd[1::4, 7] > 44).all()
