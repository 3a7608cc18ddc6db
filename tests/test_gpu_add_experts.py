"""AddExperts on the MI355X: the score-bias kernel, the biased routing entry point, the selection on both paths, the
receiver against the reference's own hook (tests/golden/add_experts_*) and through the pipeline.

Bars:
  * sdmoe_score_bias and the geglu_route_bias identities are bitwise (an fp16 + fp16 sum is exact in fp32, so the one
    round-to-nearest-even conversion is torch's fp16 add);
  * the selection is compared with the top-k' of the scores the DEVICE returned (ties toward the lowest expert id):
    no tolerance;
  * the receiver against the reference's hook uses the contract of tests/test_gpu_receiver_golden.py::compare_call
    (check_out / near_tie_rows of test_gpu_route_parity, same arguments); near-tie rows (biased score, k', 8 ulps)
    are at most 5 % of every call's rows.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import add_experts_ref as R  # noqa: E402
from sdmoe import ops  # noqa: E402
from sdmoe.unet import GEGLU, LoRACompatibleLinear  # noqa: E402
from test_gpu_route_parity import check_out, fp16_spacing, near_tie_rows  # noqa: E402,F401

DEV = "cuda"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ sdmoe_score_bias
SPECIAL_S = [0.0, -0.0, 6e-8, -6e-8, 3e-5, 65504.0, -65504.0, 1.0, 1.0 + 2.0 ** -10, 2048.0, 60000.0, -1.0]
SPECIAL_B = [0.0, -0.0, 6e-8, 2.0 ** -11, 65504.0, -65504.0, 1.0, 6000.0, -3e-5, 3.0 * 2.0 ** -11]
# (1 + 2^-11 and 1 + 2^-10 + 2^-11 are exact rounding ties; 65504 + 65504, 60000 + 6000 overflow to +inf; 6e-8 + 6e-8,
#  3e-5 - 3e-5 stay subnormal / cancel to +0; -0 + -0 = -0. No +inf and -inf meet, so no NaN is formed.)


def bias_inputs(M, E, seed):
    g = torch.Generator().manual_seed(seed)
    score = (torch.randn(M, E, generator=g) * 4).half()
    bias = (torch.randn(E, generator=g) * 2).half()
    ns, nb = len(SPECIAL_S), len(SPECIAL_B)
    for j in range(min(E, 2 * nb)):
        bias[j] = SPECIAL_B[j % nb]
    for r in range(min(M, ns)):
        for j in range(min(E, 2 * nb)):
            score[r, j] = SPECIAL_S[(r + j // nb) % ns]
    return score, bias


@pytest.mark.parametrize("E", [5, 64, 72, 256])
@pytest.mark.parametrize("M", [1, 37, 4099])
def test_score_bias_bitwise(M, E):
    score, bias = bias_inputs(M, E, 100 * M + E)
    want = score + bias  # torch's fp16 add on the CPU
    assert torch.isfinite(score).all() and not torch.isnan(want).any()
    if M >= len(SPECIAL_S) and E >= 2 * len(SPECIAL_B):
        assert torch.isinf(want).any() and (want == 1.0).any()
    bd = bias.to(DEV)
    # contiguous rows, out of place and in place
    s = score.to(DEV)
    out = torch.full((M, E), 7.0, dtype=torch.float16, device=DEV)
    ops.score_bias(s, bd, out=out)
    assert torch.equal(bits(out), bits(want)) and torch.equal(bits(s), bits(score))
    assert ops.score_bias(s, bd) is s
    assert torch.equal(bits(s), bits(want))
    # strided rows (ld = E + 24) with poisoned padding, out of place and in place
    ld = E + 24
    for inplace in (False, True):
        sbuf = torch.full((M, ld), 123.0, dtype=torch.float16, device=DEV)
        obuf = torch.full((M, ld), -77.0, dtype=torch.float16, device=DEV)
        sbuf[:, :E] = score.to(DEV)
        got = ops.score_bias(sbuf[:, :E], bd, out=None if inplace else obuf[:, :E])
        assert torch.equal(bits(got), bits(want))
        assert bool((sbuf[:, E:] == 123.0).all()) and bool((obuf[:, E:] == -77.0).all())
        if not inplace:
            assert torch.equal(bits(sbuf[:, :E]), bits(score))
    # a pointer offset by one element: the scalar path
    flat = torch.full((M * E + 2,), 55.0, dtype=torch.float16, device=DEV)
    view = flat[1:1 + M * E].view(M, E)
    view.copy_(score.to(DEV))
    ops.score_bias(view, bd)
    assert torch.equal(bits(view), bits(want))
    assert float(flat[0]) == 55.0 and float(flat[-1]) == 55.0


# ------------------------------------------------------------------------------------------------ shared operands
def operands(M, E, seed, gate_bias=0.0):
    """x [M, C], GEGLU proj (w, b), down (wd, bd) and a routing with scattered balanced 20-neuron experts."""
    C = 5 * E
    F = 4 * C
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g).half().to(DEV)
    w = (torch.randn(2 * F, C, generator=g) * C ** -0.5).half().to(DEV)
    b = (torch.randn(2 * F, generator=g) * 0.3)
    b[F:] += gate_bias
    b = b.half().to(DEV)
    wd = (torch.randn(C, F, generator=g) * F ** -0.5).half().to(DEV)
    bd = (torch.randn(C, generator=g) * 0.1).half().to(DEV)
    k = int(E * 0.2)
    routing = ops.Routing(torch.randperm(F, generator=g) % E, E, k, DEV)
    assert routing.fusable and routing.esize == 20
    return x, w, b, wd, bd, routing, g


def route(y, routing, M, E, F, **kw):
    out = torch.empty((M, F), dtype=torch.float16, device=DEV)
    gate = torch.empty((M, F), dtype=torch.float16, device=DEV)
    sel = torch.zeros((M, (E + 31) // 32), dtype=torch.int32, device=DEV)
    score = torch.empty((M, E), dtype=torch.float16, device=DEV)
    ops.geglu_route(y, routing, ops.ACT_RELU, out=out, gate_out=gate, sel_out=sel, score_out=score, **kw)
    return out, gate, sel, score


@pytest.mark.parametrize("E", [64, 256])
def test_geglu_route_bias_identities(E):
    M = 37
    x, w, b, _, _, routing, g = operands(M, E, 7 + E)
    F = routing.F
    y = ops.linear(x, w, b)
    kk = R.k_selected(routing.k)
    rm = ops.removed_bits([1, E - 2], E, DEV)
    for removed in (None, rm):
        plain = route(y, routing, M, E, F, removed=removed, k=kk)
        zero = route(y, routing, M, E, F, removed=removed, k=kk, bias=torch.zeros(E, dtype=torch.float16, device=DEV))
        for a, z in zip(plain, zero):
            assert torch.equal(a, z)
        # the entry point itself with bias == NULL
        lib = ops._lib.load()
        null = [torch.empty_like(t) for t in plain]
        st = lib.sdmoe_geglu_route_bias(y.data_ptr(), y.stride(0), M, F, E, kk, ops.ACT_RELU, routing.labels.data_ptr(),
                                        routing.e_off.data_ptr(), routing.e_nid.data_ptr(), ops._ptr(removed),
                                        null[0].data_ptr(), F, null[1].data_ptr(), F, null[2].data_ptr(),
                                        null[3].data_ptr(), None, ops._stream())
        assert st == 0
        for a, z in zip(plain, null):
            assert torch.equal(a, z)
        bias = (torch.randn(E, generator=g) * 3).half()
        biased = route(y, routing, M, E, F, removed=removed, k=kk, bias=bias.to(DEV))
        assert torch.equal(bits(biased[3]), bits(plain[3].cpu() + bias))


# ------------------------------------------------------------------------------------------------ selection
def bias_case(kind, E, kk, g):
    bias = torch.zeros(E, dtype=torch.float16)
    ids = torch.randperm(E, generator=g)
    if kind == "moderate":
        bias[ids[:kk + 3]] = (torch.rand(kk + 3, generator=g) * 4 + 0.5).half()
    elif kind == "many_inf":
        bias[ids[:kk + 3]] = 60000.0
    else:
        bias[ids[:1]] = 60000.0
    return bias, sorted(int(e) for e in ids[:1 if kind == "single" else kk + 3])


@pytest.mark.parametrize("kind", ["moderate", "many_inf", "single"])
@pytest.mark.parametrize("M,E", [(37, 64), (37, 256), (16400, 64), (16400, 256)])
def test_selection_exact_against_own_scores(M, E, kind):
    """many_inf: the gate bias 300 makes every raw score ~ 6000, so 60000 on k' + 3 experts sends all of them to +inf
    and the lowest k' ids among them must win in every row. single: one expert at +60000 is in every row's selection
    (this fails if the bias is ignored)."""
    x, w, b, wd, bd, routing, g = operands(M, E, 11 * E + M, gate_bias=300.0 if kind == "many_inf" else 0.0)
    F = routing.F
    kk = R.k_selected(routing.k)
    bias, listed = bias_case(kind, E, kk, g)
    bdev = bias.to(DEV)
    # unfused
    y = ops.linear(x, w, b)
    _, _, sel_u, score_u = route(y, routing, M, E, F, k=kk, bias=bdev)
    on_u = R.unpack_sel(sel_u.cpu().numpy(), E)
    su = score_u.cpu().numpy()
    assert np.array_equal(on_u, R.topk_lowest(su, kk))
    # fused: linear_geglu -> score_bias -> moe_topk_keep(k = k')
    w_il, b_il = ops.interleave_geglu(w, b, routing.perm)
    score = torch.empty((M, E), dtype=torch.float16, device=DEV)
    P = ops.linear_geglu(x, w_il, b_il, ops.ACT_RELU, score=score, esize=routing.esize)
    ops.score_bias(score, bdev)
    sel = torch.zeros((M, (E + 31) // 32), dtype=torch.int32, device=DEV)
    keep = ops.moe_topk_keep(score, routing, M, sel_out=sel, k=kk)
    sf = score.cpu().numpy()
    on = R.unpack_sel(sel.cpu().numpy(), E)
    assert np.array_equal(on, R.topk_lowest(sf, kk))
    assert np.array_equal(R.unpack_keep(keep.cpu().numpy()), R.expand_keep(on, routing.esize))
    assert (on.sum(1) == kk).all()
    if kind == "many_inf":
        assert np.isposinf(sf[:, listed]).all()
        assert on[:, listed[:kk]].all() and not on[:, listed[kk:]].any()
    if kind == "single":
        assert on[:, listed[0]].all() and on_u[:, listed[0]].all()
    # the keep words in the down projection == the mask pass at k' followed by the plain down projection
    Pm = P.clone()
    sel_m = torch.zeros_like(sel)
    ops.moe_topk_mask(Pm, score, routing, sel_out=sel_m, k=kk)
    assert torch.equal(sel_m, sel)
    assert torch.equal(ops.linear_keep(P, keep, wd, bd), ops.linear(Pm, wd, bd))


# ------------------------------------------------------------------------------------------------ receiver vs reference
GOLD = R.golden("add_experts")


def fixture_module(c, l, d):
    """Our GEGLU with the fixture's weights of module l, MoE-fied from a label FILE through helper.modify_ffn."""
    from moefication.helper import modify_ffn
    C = int(c["C"])
    w, b = R.weights(c, l)
    m = GEGLU(LoRACompatibleLinear(w.to(DEV), b.to(DEV)))
    if str(c["act"]) == "relu":
        m.gelu = torch.nn.functional.relu  # sparsity/relufy_model.py:35
    lp = os.path.join(d, "labels")
    torch.save([np.int64(v) for v in c["labels"]], lp)
    modify_ffn(m, lp, float(c["topk"]))
    assert m.k == int(c["k"]) and m.patterns.shape == (int(c["E"]), 4 * C)
    return m, w, b


@pytest.mark.parametrize("name,c", GOLD, ids=[n for n, _ in GOLD])
def test_receiver_against_the_reference_hook(name, c, tmp_path, parity_report):
    """AddExperts, reading its lists and statistics from files at the reference's derived paths, through the fixture's
    four hooked calls. Per call the two contracts of tests/test_gpu_receiver_golden.py::compare_call, same arguments
    and bars, with the routing taken on the BIASED score at k':
      (1) the restated hook (tests/add_experts_ref.py, pinned bit for bit to these fixtures on the CPU by
          tests/test_add_experts_host.py) on the DEVICE's projection y: output and stored gate bit-identical on every
          row that is not an exact k'-th-score tie (ReLU; a tie at score 0 selects no neuron either way), or within
          check_out outside ties and the 2-ulp band (GELU);
      (2) the reference's output: within 2e-2 * max(1, |ref|.max()) on every row clear of exact ties and of the 8-ulp
          near-tie band. (compare_call's bitwise bar on rows whose device y equals the reference's y needs the
          reference's y, which these fixtures do not carry: they stay in the size range of their expert_* siblings.)
    Near-tie rows (reference's biased score, k', 8 ulps) are at most 5 % of every call's rows. The reference's out and
    gate are recorded for the first call; for the others they are the restated hook's on the CPU."""
    from neuron_receivers import AddExperts
    C, E, k, kk, T, L = (int(c[n]) for n in ("C", "E", "k", "kk", "T", "L"))
    relu, act = str(c["act"]) == "relu", str(c["act"])
    lists = {tuple(map(int, key.split(","))): v for key, v in json.loads(str(c["lists"])).items()}
    path = tmp_path / "adj_x" / "x" / "y"
    path.mkdir(parents=True)
    stats = {"time_steps": {str(t): {str(l): {"std": c["std"][t * L + l].tolist()} for l in range(L)} for t in range(T)}}
    (tmp_path / "adj_x" / "predictivity_base_expert.json").write_text(json.dumps(stats))
    for (t, l), ids in lists.items():
        (path / f"timestep_{t}_layer_{l}.json").write_text(json.dumps(ids))
    mods = [fixture_module(c, l, str(tmp_path)) for l in range(L)]
    pat = R.patterns(c)
    rec = AddExperts(0, str(path), T, L)
    totals = dict(rows=0, exact_tie=0, compared=0, golden_tolerance_rows=0, near_tie=0)
    for call, (t, l) in enumerate(c["call_tl"]):
        t, l = int(t), int(l)
        m, w, b = mods[l]
        ids, std = lists[(t, l)], c["std"][call].tolist()
        x = R.tokens(c, call)
        assert (rec.timestep, rec.layer) == (t, l)
        with torch.no_grad():
            out = rec.hook_fn(m, (x.to(DEV),), None)
        o = out.cpu().numpy().reshape(-1, 4 * C)
        g = rec.gates[call].numpy().reshape(-1, 4 * C)
        y_dev = ops.linear(x.to(DEV).reshape(-1, C), m.proj.weight, m.proj.bias).cpu()
        yd = y_dev.numpy()
        # (1) the restated hook on the device's y
        o1, g1, s1, _ = R.route_from_y(y_dev, act, pat, k, ids, std)
        o1, g1, s1 = o1.numpy(), g1.numpy(), s1.float().numpy()
        s = np.sort(s1, axis=1)[:, ::-1]
        tie = s[:, kk - 1] == s[:, kk]
        if relu:
            rows = ~tie | (s[:, kk - 1] == 0)
            assert np.array_equal(o[rows], o1[rows]), f"call {call}: output differs from the restated hook"
            assert np.array_equal(g[rows], g1[rows]), f"call {call}: stored gate differs from the restated hook"
        else:
            rows = ~tie & ~near_tie_rows(s1, kk)
            check_out(o, o1, g, g1, yd[:, :4 * C], rows)
        # (2) the reference's output: recorded for the first call; for the others the restated hook on this host's CPU
        # (whose fp16 sums may differ by an ulp from the CPU the fixture was made on, hence no bitwise bar here)
        if call == 0:
            ro = c["out0"].reshape(-1, 4 * C)
        else:
            ro = R.add_hook(x, w, b, act, pat, k, ids, std)[0].numpy().reshape(-1, 4 * C)
        near = near_tie_rows(c["score"][call], kk, slack_ulps=8)
        assert near.sum() <= 0.05 * near.size, f"call {call}: {int(near.sum())} near-tie rows of {near.size}"
        other = ~tie & ~near
        assert other.any()
        err = np.abs(o[other].astype(np.float32) - ro[other].astype(np.float32)).max()
        assert err <= 2e-2 * max(1.0, np.abs(ro.astype(np.float32)).max()), f"call {call}: {err}"
        totals["rows"] += rows.size
        totals["compared"] += int(rows.sum())
        totals["exact_tie"] += int(tie.sum())
        totals["golden_tolerance_rows"] += int(other.sum())
        totals["near_tie"] += int(near.sum())
    assert (rec.timestep, rec.layer) == (T, 0) and len(rec.gates) == T * L
    assert totals["compared"] >= 0.85 * totals["rows"], totals  # (the bar of the remove_* sequences)
    parity_report(f"receiver_add_experts[{name}]", **totals)


# ------------------------------------------------------------------------------------------------ pipeline
def test_through_the_pipeline():
    """SD-1.4 widths at sample size 16 (fused-eligible FFNs), two prompts, two DDIM steps, relufied, MoE-fied at 0.2."""
    from moefication.helper import moefy_synthetic
    from neuron_receivers import AddExperts, MOEFy
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    from sdmoe.unet import UNet2DConditionModel
    from sdmoe.weights import make_state_dict
    from sparsity.relufy_model import find_and_change_geglu
    cfg = UNetConfig.sd14(16)
    unet = UNet2DConditionModel.from_state_dict(make_state_dict(cfg, 6), cfg, DEV)
    T = 2
    pipe = StableDiffusionPipeline(unet, DEV, num_inference_steps=T)
    moefy_synthetic(pipe, 0.2, 20, seed=2)
    find_and_change_geglu(pipe.unet)
    geglus = [m for n, m in unet.named_modules() if n.endswith("ff.net.0")]
    L = len(geglus)
    prompts = ["a cat", "Starry night by Van Gogh"]
    nexp = [m.patterns.shape[0] for m in geglus]

    def stats(value):
        return {"time_steps": {str(t): {str(l): {"std": [value] * nexp[l]} for l in range(L)} for t in range(T)}}

    def lists(fn):
        return {t: {l: fn(t, l) for l in range(L)} for t in range(T)}

    def run(rec):
        out, _ = rec.observe_activation(pipe, prompts)
        return torch.stack(out)

    # the bar: MOEFy on the same modules with k set to int(0.8 k) by hand
    ks = [m.k for m in geglus]
    try:
        for m in geglus:
            m.k = R.k_selected(m.k)
        base = run(MOEFy(seed=0, store_gates=False))
    finally:
        for m, k in zip(geglus, ks):
            m.k = k
    assert torch.isfinite(base).all()
    # (ii) all lists empty, (i) on the fused path, (vi) the counter
    rec = AddExperts(0, None, T, L, store_gates=False, expert_indices=lists(lambda t, l: []), activation_stats=stats(1.0))
    empty = run(rec)
    assert torch.equal(empty, base)
    assert all(m._out_keep is not None and m._out_perm is not None for m in geglus)
    assert (rec.timestep, rec.layer) == (T, 0)
    import sdmoe.unet as U
    U.FUSED_KEEP = False
    try:
        nokeep = run(AddExperts(0, None, T, L, store_gates=False, expert_indices=lists(lambda t, l: []),
                                activation_stats=stats(1.0)))
        assert all(m._out_keep is None and m._out_perm is not None for m in geglus)
    finally:
        U.FUSED_KEEP = True
    assert torch.equal(nokeep, base)
    # (iii) a zero std under non-empty lists
    some = lists(lambda t, l: [(3 * l + t) % nexp[l], (5 * l + 1) % nexp[l]])
    zero = run(AddExperts(0, None, T, L, store_gates=False, expert_indices=some, activation_stats=stats(0.0)))
    assert torch.equal(zero, base)
    # (iv) a real bias changes the latents; 5 * 12000 = 60000 on one expert per cell: every token selects it
    real = run(AddExperts(0, None, T, L, store_gates=False, expert_indices=some, activation_stats=stats(0.5)))
    assert torch.isfinite(real).all() and not torch.equal(real, base)
    one = lists(lambda t, l: [(7 * l + t) % nexp[l]])
    rec = AddExperts(0, None, T, L, store_gates=False, expert_indices=one, activation_stats=stats(12000.0),
                     count_selected=True)
    run(rec)
    assert (rec.timestep, rec.layer) == (T, 0)
    for t in range(T):
        for l in range(L):
            e = one[t][l][0]
            assert rec.selection_rate(t, l) == {e: 1.0}
            cnt = rec.selection_count[t][l]
            assert cnt.dtype == np.int64 and cnt.shape == (nexp[l],)
            assert cnt.sum() == rec.selection_tokens[t][l] * R.k_selected(geglus[l].k)
    # test(): the inherited BaseNeuronReceiver.test -- every stored gate >= 0 under the relufied U-Net, the hooked run differs
    rec = AddExperts(0, None, T, L, store_gates=False, expert_indices=some, activation_stats=stats(0.5))
    nochange, changed = rec.test(pipe, prompts[0], relu_condition=True)
    assert not torch.equal(nochange, changed) and rec.gates == [] and rec.store_gates is False
    # (v) store_gates=True (the unfused path, sdmoe_geglu_route_bias) against the fused path: the same selection_count
    # on rows that are not near ties. Lists of k' + 4 experts whose biases step by 20 (std 4, 8, ...): the k'-th and
    # (k'+1)-th listed experts then differ by 20 plus a score difference of a few units, against a near-tie band of at
    # most 8 ulps = 4 at these magnitudes, so near-tie rows are rare; at most 5 % per call is asserted. The two runs
    # see inputs that differ by the down projections' summation order, so only rows clear of the band in BOTH runs are
    # compared. The per-call scores and selection bits are taken where the receiver hands them to ops.expert_stats.
    kks = [R.k_selected(m.k) for m in geglus]
    many = lists(lambda t, l: [(11 * j + l + t) % nexp[l] for j in range(kks[l] + 4)])
    steps = {"time_steps": {str(t): {str(l): {"std": [0.0] * nexp[l]} for l in range(L)} for t in range(T)}}
    for t in range(T):
        for l in range(L):
            assert len(set(many[t][l])) == kks[l] + 4
            for j, e in enumerate(many[t][l]):
                steps["time_steps"][str(t)][str(l)]["std"][e] = 4.0 * (j + 1)
    real_stats = ops.expert_stats
    runs = []
    for store in (False, True):
        seen = []

        def spy(score, **kw):
            seen.append((score.clone(), kw["sel"].clone()))
            return real_stats(score, **kw)

        rec = AddExperts(0, None, T, L, store_gates=store, expert_indices=many, activation_stats=steps,
                         count_selected=True)
        ops.expert_stats = spy
        try:
            run(rec)
        finally:
            ops.expert_stats = real_stats
        assert len(seen) == T * L and len(rec.gates) == (T * L if store else 0)
        assert all((m._out_perm is None) == store for m in geglus)  # unfused under store_gates, fused without
        runs.append((rec, seen))
    for call in range(T * L):
        t, l = call // L, call % L
        E, kk = nexp[l], kks[l]
        ons, nears = [], []
        for rec, seen in runs:
            score, sel = (a.cpu().numpy() for a in seen[call])
            on = R.unpack_sel(sel, E)
            assert np.array_equal(on, R.topk_lowest(score, kk))
            assert np.array_equal(rec.selection_count[t][l], on.sum(0).astype(np.int64))
            near = near_tie_rows(score, kk, slack_ulps=8)
            assert near.sum() <= 0.05 * near.size, (t, l, int(near.sum()), near.size)
            ons.append(on)
            nears.append(near)
        clear = ~nears[0] & ~nears[1]
        assert np.array_equal(ons[0][clear].sum(0), ons[1][clear].sum(0)), (t, l)
