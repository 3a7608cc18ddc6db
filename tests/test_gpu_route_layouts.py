"""The routed GEGLU off the balanced 20-neuron layout, bit for bit against tests/route_ref.py (a numpy restatement that
shares no code with the product; tests/test_route_ref_host.py checks it and every input used here on the CPU):

a. sdmoe_geglu_route / _bias on unbalanced layouts: empty experts, one of 300 neurons, E from 1 to 256 on both sides
   of every 64-expert slot, F any multiple of 8, M with a partly live workgroup, k in {0, 1, middle, E}, removed lists
   with an empty, a tied and every expert, strided operands with guard columns;
b. the same with GELU on gates in the registered table's range (the activated gate is torch's, not a kernel's);
c. the fused score epilogue (expert_sums) at every admitted expert size, on every GEGLU tile, LN-folded too;
d. linear_geglu -> moe_topk_mask / moe_topk_keep at those sizes equal the reference and the unfused kernel;
e. the three top-k kernels on scores drawn from the whole fp16 key space.

Every comparison is exact and covers every row: ties are decided by the rule (lowest expert id), not left out.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sdmoe import _lib, ops, tune  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_ref as R  # noqa: E402

DEV = "cuda"
GUARD = 8          # guard columns on both sides of every strided operand (keeps the 16-B alignment)
FILL = 77.0        # their content, and the content of every output before the call


def _wide(payload=None, shape=None):
    """(wide, view): a [M, GUARD + C + GUARD] fp16 device buffer filled with FILL and its middle column slice, set to
    `payload` (numpy fp16 [M, C]) when given."""
    M, C = payload.shape if payload is not None else shape
    wide = torch.full((M, C + 2 * GUARD), FILL, dtype=torch.float16, device=DEV)
    view = wide[:, GUARD:GUARD + C]
    if payload is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(payload)))
    return wide, view


def _expect_wide(payload):
    return _wide(payload)[0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(words):
    return _dev(words.view(np.int32))


def _removed_bits(rm, E):
    return ops.removed_bits(rm, E, DEV) if len(rm) else None


def _run_unfused(c, y_np, act, gate_act, form, bias=None):
    """Every (removed, k) of a case through ops.geglu_route on guarded column slices, against the reference."""
    E, F, M, labels = c["E"], c["F"], c["M"], c["labels"]
    routing = ops.Routing(torch.from_numpy(labels), E, c["kmid"], DEV)
    assert routing.fusable is False or E == 1
    y_wide, y = _wide(y_np)
    y_before = y_wide.clone()
    nw = (E + 31) // 32
    for rm in c["removed"]:
        for k in c["ks"]:
            ref = R.route(y_np, labels, E, k, gate_act=gate_act, removed=rm, bias=bias, form=form)
            out_wide, out = _wide(shape=(M, F))
            gate_wide, gate = _wide(shape=(M, F))
            sel = torch.full((M, nw), -1, dtype=torch.int32, device=DEV)
            score = torch.full((M, E), FILL, dtype=torch.float16, device=DEV)
            ops.geglu_route(y, routing, act, removed=_removed_bits(rm, E), out=out, gate_out=gate, sel_out=sel,
                            score_out=score, k=k, bias=None if bias is None else _dev(bias))
            torch.cuda.synchronize()
            what = f"E={E} F={F} M={M} k={k} removed={rm if len(rm) < 6 else 'all'} {form}"
            assert torch.equal(score, _dev(ref["score"])), f"score: {what}"
            assert torch.equal(sel, _i32(R.sel_words(ref["sel"]))), f"selection: {what}"
            assert torch.equal(gate_wide, _expect_wide(ref["gate"])), f"gate_out: {what}"
            assert torch.equal(out_wide, _expect_wide(ref["out"])), f"out: {what}"
            assert torch.equal(y_wide, y_before), f"y changed: {what}"


# ---- a. unfused kernel, arbitrary layouts ---------------------------------------------------------------------

@pytest.mark.parametrize("E,F,M,kmid,b", R.LAYOUT_CASES)
def test_unfused_route_on_unbalanced_layouts(E, F, M, kmid, b):
    """ReLU. Quantised gates: expected scores are the exact sums (independent of the summation order). Plain
    randn * 1.5 gates: expected scores are the fp32 sums taken in ascending neuron id, which pins the order."""
    c = R.layout_case(E, F, M, kmid, b)
    _run_unfused(c, np.concatenate([c["value"], c["gate_q"]], 1), ops.ACT_RELU, None, "float64")
    _run_unfused(c, np.concatenate([c["value"], c["gate_plain"]], 1), ops.ACT_RELU, None, "float32")


@pytest.mark.parametrize("E,F,M,kmid,b", R.BIAS_CASES)
def test_unfused_route_with_bias_on_unbalanced_layouts(E, F, M, kmid, b):
    """sdmoe_geglu_route_bias: the bias joins the ROUNDED score in fp32 and the sum is rounded once more; a removed
    expert scores 0 + bias."""
    c = R.layout_case(E, F, M, kmid, b)
    _run_unfused(c, np.concatenate([c["value"], c["gate_q"]], 1), ops.ACT_RELU, None, "float64", bias=c["bias"])


# ---- b. GELU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E,F,M,kmid,b", R.GELU_CASES)
def test_unfused_route_gelu_on_unbalanced_layouts(E, F, M, kmid, b):
    """Gates with 2^-5 <= |x| < 8 or 0: the kernel applies the registered table there, so its activated gate is
    F.gelu of the fp16 tensor bit for bit; that torch result is what enters the reference. Row 0 is all negative:
    a removed expert (score 0) is then selected ahead of every live one and never kept."""
    c = R.gelu_case(E, F, M, kmid, b)
    gact = torch.nn.functional.gelu(_dev(c["gate"])).cpu().numpy()
    _run_unfused(c, np.concatenate([c["value"], c["gate"]], 1), ops.ACT_GELU, gact, "float32")


# ---- c. fused score epilogue -----------------------------------------------------------------------------------

def _unit_rows(M):
    x = torch.zeros(M, 64, dtype=torch.float16)
    x[torch.arange(M), torch.arange(M) % 64] = 1.0
    return x.to(DEV)


def _weights(value, gate):
    """W [2F, 64] whose product with the unit row e_j is exactly [value[j] | gate[j]]."""
    return _dev(np.concatenate([value.T, gate.T], 0))


# 64x160, 128x160, 256x320 2x4 (ReLU) / 256x160 4x2 and 256x320 2x4 with the GELU table (gt320 = 0 / 1), M tails
EPILOGUE_RUNS = [(64, 80, "relu", 0), (70, 80, "relu", 0), (70, 320, "relu", 0), (64, 1280, "relu", 0),
                 (4096, 1280, "relu", 0), (8192, 1280, "relu", 0), (70, 1280, "gelu", 0), (4096, 1280, "gelu", 0),
                 (8192, 1280, "gelu", 0), (8192, 1280, "gelu", 1)]


@pytest.mark.parametrize("M,F,act,gt320", EPILOGUE_RUNS)
@pytest.mark.parametrize("esize", R.ESIZES)
def test_fused_score_epilogue_every_expert_size(esize, M, F, act, gt320):
    """sdmoe_linear_geglu's per-expert gate sums and product for experts of 1 .. 40 contiguous neurons, the GEMM
    driven to exact chosen values (x rows are unit vectors, K = 64, bias 0). F = 80 is the smallest admitted; F = 320
    and 1280 give E > 256 for the small sizes, which the epilogue (unlike the top-k) does not mind."""
    E = F // esize
    labels = np.arange(F) // esize
    value, gate, _ = R.fused_rows(F, esize)
    if act == "relu":
        gact, form, code = R.relu16(gate), "float64", ops.ACT_RELU
    else:
        gate = R.gelu_range_gates(np.random.default_rng(F + esize), (64, F))
        gact, form, code = torch.nn.functional.gelu(_dev(gate)).cpu().numpy(), "float32", ops.ACT_GELU
    exp_score = _dev(R.scores(gact, labels, E, form))
    exp_P = _dev((value.astype(np.float32) * gact.astype(np.float32)).astype(np.float16))
    w = _weights(value, gate)
    w_il, b_il = ops.interleave_geglu(w, torch.zeros(2 * F, dtype=torch.float16, device=DEV), None)
    ld = E + 3
    score_wide = torch.full((M, ld), FILL, dtype=torch.float16, device=DEV)
    with tune.tuned(gt320=gt320):
        P = ops.linear_geglu(_unit_rows(M), w_il, b_il, code, score=score_wide[:, :E], esize=esize)
    rows = torch.arange(M, device=DEV) % 64
    assert torch.equal(P, exp_P[rows])
    assert torch.equal(score_wide[:, :E], exp_score[rows])
    assert bool((score_wide[:, E:] == FILL).all())


@pytest.mark.parametrize("esize,M", [(8, 70), (5, 200)])
def test_fused_score_epilogue_ln_folded(esize, M):
    """The LN-folded GEMM's epilogue at an expert size other than 20: x rows of +-1 with mean 0 and variance 1 and
    eps = 0 make the norm the identity, W holds multiples of 2^-8, so y = x W^T is exact and an fp16 value."""
    F = 320
    E = F // esize
    x64, w = R.ln_case_operands(F)
    y = (x64.astype(np.float64) @ w.astype(np.float64).T).astype(np.float16)
    labels = np.arange(F) // esize
    ref = R.route(y, labels, E, E)
    fold = ops.LNFold(_dev(w), torch.ones(64, dtype=torch.float16, device=DEV),
                      torch.zeros(64, dtype=torch.float16, device=DEV), 0.0)
    fold = ops.interleave_ln_fold(fold, None)
    rows = torch.arange(M) % 64
    score = torch.full((M, E), FILL, dtype=torch.float16, device=DEV)
    P = ops.linear_geglu(_dev(x64)[rows.to(DEV)].contiguous(), None, None, ops.ACT_RELU, score=score, esize=esize,
                         ln=fold)
    assert torch.equal(P, _dev(ref["out"])[rows.to(DEV)])
    assert torch.equal(score, _dev(ref["score"])[rows.to(DEV)])


# ---- d. mask, keep and unfused agree ---------------------------------------------------------------------------

def _chain_removed(E):
    return sorted({1, E // 2 + 3, E - 1})


@pytest.mark.parametrize("topk", (0, 4))
@pytest.mark.parametrize("esize,F,k", R.CHAIN_CASES)
def test_mask_keep_and_unfused_chains_every_expert_size(esize, F, k, topk):
    """linear_geglu -> moe_topk_mask and linear_geglu -> moe_topk_keep on balanced experts scattered over the neurons,
    one and four tokens per wave (knob topk = 0 / 4): the masked product, keep words and selection bits of the
    reference, and -- un-permuted -- the unfused kernel's output on ops.linear's y. Where 64 does not divide F there
    are no keep words: sdmoe_moe_topk_keep must refuse the shape."""
    E, M = F // esize, 70
    labels = R.chain_labels(F, esize)
    value, gate, _ = R.fused_rows(F, esize, labels=labels, k=k)
    y64 = np.concatenate([value, gate], 1)
    routing = ops.Routing(torch.from_numpy(labels), E, k, DEV)
    assert routing.fusable and routing.esize == esize
    assert np.array_equal(routing.perm.numpy(), R.expert_major(labels))
    w = _weights(value, gate)
    zero_b = torch.zeros(2 * F, dtype=torch.float16, device=DEV)
    w_il, b_il = ops.interleave_geglu(w, zero_b, routing.perm)
    x = _unit_rows(M)
    rows = np.arange(M) % 64
    perm = routing.perm.to(DEV)
    nw = (E + 31) // 32
    with tune.tuned(topk=topk):
        score = torch.full((M, E), FILL, dtype=torch.float16, device=DEV)
        P = ops.linear_geglu(x, w_il, b_il, ops.ACT_RELU, score=score, esize=esize)
        raw = R.scores(R.relu16(gate), labels, E, "float64")
        assert torch.equal(score, _dev(raw[rows]))
        y = ops.linear(x, w, zero_b)
        assert torch.equal(y, _dev(y64[rows]))
        for rm in ([], _chain_removed(E)):
            ref = R.route(y64, labels, E, k, removed=rm)
            exp_sel = _i32(R.sel_words(ref["sel"][rows]))
            exp_out = _dev(ref["out"][rows])
            bits = _removed_bits(rm, E)
            # mask chain
            Pm = P.clone()
            sel_m = torch.full((M, nw), -1, dtype=torch.int32, device=DEV)
            ops.moe_topk_mask(Pm, score, routing, removed=bits, sel_out=sel_m)
            out_m = torch.empty_like(Pm)
            out_m[:, perm] = Pm
            assert torch.equal(sel_m, exp_sel), f"mask selection, removed={rm}"
            assert torch.equal(out_m, exp_out), f"masked product, removed={rm}"
            # keep chain
            if F % 64 == 0:
                sel_k = torch.full((M, nw), -1, dtype=torch.int32, device=DEV)
                keep = ops.moe_topk_keep(score, routing, M, removed=bits, sel_out=sel_k)
                assert torch.equal(sel_k, exp_sel), f"keep selection, removed={rm}"
                assert torch.equal(keep, _dev(R.keep_words(ref["keep"][rows], labels).view(np.int64))), f"removed={rm}"
            else:
                with pytest.raises(_lib.SdmoeError, match=r"\(-2\)"):
                    ops.moe_topk_keep(score, routing, M, removed=bits,
                                      keep=torch.empty((F // 64, M), dtype=torch.int64, device=DEV))
            # unfused kernel on the plain projection
            sel_u = torch.full((M, nw), -1, dtype=torch.int32, device=DEV)
            score_u = torch.empty_like(score)
            out_u = ops.geglu_route(y, routing, ops.ACT_RELU, removed=bits, sel_out=sel_u, score_out=score_u)
            assert torch.equal(sel_u, exp_sel) and torch.equal(out_u, out_m)
            assert torch.equal(score_u, _dev(ref["score"][rows]))


@pytest.mark.parametrize("topk", (0, 4))
def test_keep_refuses_experts_above_40_neurons_mask_does_not(topk):
    """esize = 80 (E = 8, F = 640): no keep-word form (SDMOE_EUNSUP) and not fusable; the mask form runs on given
    scores and follows the rule."""
    E, esize, M, k = 8, 80, 37, 3
    F = E * esize
    labels = np.arange(F) // esize
    routing = ops.Routing(torch.from_numpy(labels), E, k, DEV)
    assert not routing.fusable and routing.esize == esize
    c = R.topk_case(E, esize, M, E + 1)
    rm = [2]
    score = _dev(c["score"])[:, :E]
    with tune.tuned(topk=topk):
        with pytest.raises(_lib.SdmoeError, match=r"\(-3\)"):
            ops.moe_topk_keep(score, routing, M, removed=_removed_bits(rm, E))
        P = torch.ones((M, F), dtype=torch.float16, device=DEV)
        sel = torch.full((M, 1), -1, dtype=torch.int32, device=DEV)
        ops.moe_topk_mask(P, score, routing, removed=_removed_bits(rm, E), sel_out=sel)
    ref_sel = R.select(R.final_scores(c["score"][:, :E], rm), k)
    assert torch.equal(sel, _i32(R.sel_words(ref_sel)))
    assert torch.equal(P, _dev(R.keep_of(ref_sel, rm)[:, labels].astype(np.float16)))


# ---- e. top-k on the whole fp16 key space ------------------------------------------------------------------------

@pytest.mark.parametrize("topk", (0, 1, 4))  # 1: the ballot kernel at one token per wave for E <= 64 as well
@pytest.mark.parametrize("E,esize,M,ld", R.TOPK_CASES)
def test_topk_on_every_fp16_score(E, esize, M, ld, topk):
    """moe_topk_keep (quad / group kernels at knob 0 on aligned rows, else the ballot kernel) and moe_topk_mask on
    scores from every finite fp16 bit pattern and +-inf, plus hand-made rows: all equal, +0 / -0 at the boundary,
    ties across experts 15|16, 31|32, 63|64, 127|128, more +inf than places, all-negative rows whose removed experts
    score 0 (selected, never kept), the largest finite values and subnormals. The reference is the selection rule."""
    c = R.topk_case(E, esize, M, ld)
    F, k = E * esize, c["k"]
    labels = np.arange(F) // esize
    routing = ops.Routing(torch.from_numpy(labels), E, k, DEV)
    full = _dev(c["score"])
    before = full.clone()
    score = full[:, :E]
    nw = (E + 31) // 32
    for rm in ([], c["removed"], list(range(E))):
        for kk in sorted({k, 0, 1, E}):
            ref_sel = R.select(R.final_scores(c["score"][:, :E], rm), kk)
            ref_keep = R.keep_of(ref_sel, rm)
            exp_sel = _i32(R.sel_words(ref_sel))
            bits = _removed_bits(rm, E)
            with tune.tuned(topk=topk):
                sel_k = torch.full((M, nw), -1, dtype=torch.int32, device=DEV)
                keep = ops.moe_topk_keep(score, routing, M, removed=bits, sel_out=sel_k, k=kk)
                P = torch.ones((M, F), dtype=torch.float16, device=DEV)
                sel_m = torch.full((M, nw), -1, dtype=torch.int32, device=DEV)
                ops.moe_topk_mask(P, score, routing, removed=bits, sel_out=sel_m, k=kk)
            what = f"k={kk} removed={rm if len(rm) < 6 else 'all'}"
            assert torch.equal(sel_k, exp_sel), f"keep selection {what}"
            assert torch.equal(sel_m, exp_sel), f"mask selection {what}"
            assert torch.equal(keep, _dev(R.keep_words(ref_keep, labels).view(np.int64))), f"keep words {what}"
            assert torch.equal(P, _dev(ref_keep[:, labels].astype(np.float16))), f"masked product {what}"
    assert torch.equal(full, before)
