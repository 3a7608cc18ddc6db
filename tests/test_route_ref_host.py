"""CPU checks of tests/route_ref.py and of the inputs tests/test_gpu_route_layouts.py feeds the kernels.

* route_ref equals oracle/hooks_ref.routed_geglu (scores, selection, gate, output) on the reference's fp16 golden
  vectors and on random balanced layouts, outside the rows tied at the k-th score (where the hook's torch order is
  not the rule);
* hand-made examples pin the rule itself: ties toward the lowest expert id, -0 == +0, a removed expert scores 0 and is
  selected but never kept, one rounding of the score and of the biased score;
* on every quantised input of the GPU tests the exact (float64) sum and the step-by-step fp32 sum agree, so the
  expected scores do not depend on the summation order;
* every GPU case still carries the edge it exists for (a tie at the k-th place, a tie pair across each lane / word /
  slot boundary, empty and large experts, an all-negative row with a removed expert).
"""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import route_ref as R  # noqa: E402
from oracle import hooks_ref as H  # noqa: E402

GOLD = os.path.join(HERE, "golden")
h = np.float16


def _goldens():
    out = []
    for f in sorted(glob.glob(os.path.join(GOLD, "moefy_*.npz")) + glob.glob(os.path.join(GOLD, "remove_*.npz"))):
        with np.load(f, allow_pickle=False) as z:
            if str(z["dtype"]) == "float16":
                out.append(os.path.basename(f))
    return out


def _gate_act(y, F, act):
    # torch's CPU fp16 GELU is not correctly rounded and its vectorised and strided paths differ by an ulp on a few
    # inputs: the activated gate is an INPUT of the reference, taken from the same strided view the hook activates
    return None if act == "relu" else Fn.gelu(torch.from_numpy(y).chunk(2, dim=-1)[1]).numpy()


def _against_hook(y, labels, E, k, act, removed):
    F = labels.size
    P = H.patterns_from_labels(labels, torch.float16)
    if P.shape[0] < E:  # (trailing empty experts)
        P = torch.cat([P, torch.zeros(E - P.shape[0], F, dtype=P.dtype)])
    o, g, sel, sc = H.routed_geglu(torch.from_numpy(y), P, k, act, removed, True)
    clear = ~H.tie_rows(sc, k).numpy()
    assert clear.any()
    for form in ("float32", "float64"):
        r = R.route(y, labels, E, k, gate_act=_gate_act(y, F, act), removed=removed or (), form=form)
        assert np.array_equal(r["score"], sc.numpy()), form
        assert np.array_equal(r["sel"][clear], sel.numpy()[clear]), form
        assert np.array_equal(r["gate"][clear], g.numpy()[clear]), form
        assert np.array_equal(r["out"][clear], o.numpy()[clear]), form


@pytest.mark.parametrize("name", _goldens())
def test_reference_equals_hook_on_goldens(name):
    with np.load(os.path.join(GOLD, name), allow_pickle=False) as z:
        c = {k_: z[k_] for k_ in z.files}
    C, E, k, act = int(c["C"]), int(c["E"]), int(c["k"]), str(c["act"])
    y = c["y"].reshape(-1, 8 * C)
    # the golden's own recorded results (moefy) pin the hook restatement; the reference is compared with both
    if str(c["kind"]) == "moefy":
        _against_hook(y, c["labels"], E, k, act, None)
        r = R.route(y, c["labels"], E, k, gate_act=_gate_act(y, 4 * C, act), form="float32")
        clear = ~c["tie"].astype(bool)
        assert np.array_equal(r["score"], c["score"])
        assert np.array_equal(r["out"][clear], c["out"].reshape(-1, 4 * C)[clear])
        assert np.array_equal(r["gate"][clear], c["gate"].reshape(-1, 4 * C)[clear])
        return
    lists = json.loads(str(c["lists"]))
    for i, (t, l) in enumerate(c["call_tl"]):
        ids = lists[f"{t},{l}"] if t < 20 else []
        _against_hook(y, c["labels"], E, k, act, ids)
        r = R.route(y, c["labels"], E, k, gate_act=_gate_act(y, 4 * C, act), removed=ids, form="float32")
        P = H.patterns_from_labels(c["labels"], torch.float16)
        clear = ~H.tie_rows(H.routed_geglu(torch.from_numpy(y), P, k, act, ids, True)[3], k).numpy()
        assert np.array_equal(r["out"][clear], c["out"][i].reshape(-1, 4 * C)[clear])


@pytest.mark.parametrize("E,esize,k,act,nrem", [(64, 20, 12, "relu", 0), (64, 20, 12, "gelu", 5), (16, 20, 3, "relu", 2),
                                               (128, 20, 25, "gelu", 9), (40, 8, 7, "relu", 3), (256, 5, 51, "relu", 20)])
def test_reference_equals_hook_on_random_balanced(E, esize, k, act, nrem):
    g = torch.Generator().manual_seed(E + esize + k)
    F = E * esize
    y = (torch.randn(24, 2 * F, generator=g) * 1.5).half().numpy()
    labels = (torch.randperm(F, generator=g) % E).numpy()
    removed = torch.randperm(E, generator=g)[:nrem].tolist()
    _against_hook(y, labels, E, k, act, removed)


def test_selection_rule_is_pinned():
    s = np.array([[1, 2, 2, 2, 0.5, 3]], dtype=h)
    assert R.select(s, 3).tolist() == [[False, True, True, False, False, True]]  # ties -> lowest ids
    assert R.select(s, 0).sum() == 0 and R.select(s, 6).all()
    z = np.array([[-1, -0.0, 0.0, -0.0, 0.0, -2]], dtype=h)
    assert R.select(z, 2).tolist() == [[False, True, True, False, False, False]]  # -0 == +0, still by id
    assert R.select(z, 3).tolist() == [[False, True, True, True, False, False]]
    inf = np.array([[np.inf, -np.inf, 65504, np.inf, -65504, 6e-8]], dtype=h)
    assert R.select(inf, 3).tolist() == [[True, False, True, True, False, False]]
    assert R.select(inf, 5).tolist() == [[True, False, True, True, True, True]]
    with pytest.raises(AssertionError):
        R.select(np.array([[np.nan, 1]], dtype=h), 1)


def test_removed_expert_rule_is_pinned():
    # experts {0: n0 n3, 1: n1, 2: n2 n4, 3: none}; every live score negative under the given activated gate
    labels = np.array([0, 1, 2, 0, 2])
    value = np.array([[2, 3, 4, 5, 6]], dtype=h)
    gact = np.array([[-1, -0.5, -0.25, -1, -0.25]], dtype=h)
    y = np.concatenate([value, gact], 1)
    r = R.route(y, labels, 4, 2, gate_act=gact, removed=[1])
    assert r["score"].tolist() == [[-2.0, 0.0, -0.5, 0.0]]  # removed -> 0, empty -> +0
    assert not np.signbit(r["score"][0, [1, 3]]).any()
    assert r["sel"].tolist() == [[False, True, False, True]]  # the removed expert takes a place from a live one
    assert r["keep"].tolist() == [[False, False, False, True]]  # ... and is never kept
    assert not r["out"].any() and not r["gate"].any()
    r3 = R.route(y, labels, 4, 3, gate_act=gact, removed=[1])
    assert r3["sel"].tolist() == [[False, True, True, True]]
    assert r3["out"].tolist() == [[0, 0, -1.0, 0, -1.5]] and r3["gate"].tolist() == [[0, 0, -0.25, 0, -0.25]]
    # ReLU of the same gates: every score 0, the first k ids win, the removed one among them
    rr = R.route(y, labels, 4, 2, removed=[0])
    assert rr["sel"].tolist() == [[True, True, False, False]] and rr["keep"].tolist() == [[False, True, False, False]]
    # keep words follow the expert-major order n0 n3 | n1 | n2 n4
    lab64 = np.arange(64) % 4
    kw = R.keep_words(np.array([[True, False, False, True]]), lab64)
    assert kw.shape == (1, 1) and int(kw[0, 0]) == (1 << 16) - 1 | ((1 << 16) - 1) << 48
    assert R.sel_words(np.array([[True] + [False] * 31 + [True]])).tolist() == [[1, 1]]


def test_rounding_points_are_pinned():
    # one rounding of the sum: 2048 + 1 + 1 is 2050 in fp16 (an fp16 running sum would stay at 2048)
    g = np.array([[2048, 1, 1, 0.5]], dtype=h)
    lab = np.array([0, 0, 0, 1])
    for form in ("float32", "float64"):
        assert R.scores(g, lab, 2, form).tolist() == [[2050.0, 0.5]]
    # fp32 step by step in ascending neuron id: 2^-13 is lost behind 4096 in fp32 (twice), kept by the exact sum
    g = np.array([[4096, 2.0 ** -13, 2.0 ** -13, -4096]], dtype=h)
    lab = np.zeros(4, dtype=int)
    assert R.scores(g, lab, 1, "float32").tolist() == [[0.0]]
    assert R.scores(g, lab, 1, "float64").tolist() == [[2.0 ** -12]]
    # the exact sum goes to fp16 directly: 2049 + 2^-24 lies above the midpoint of 2048 and 2050, while its fp32
    # rounding (2049) is the midpoint itself and ties to even
    g = np.array([[2048, 1, 2.0 ** -24]], dtype=h)
    assert R.scores(g, np.zeros(3, dtype=int), 1, "float64").tolist() == [[2050.0]]
    assert R.scores(g, np.zeros(3, dtype=int), 1, "float32").tolist() == [[2048.0]]
    # bias: fp32 add of the ROUNDED score, rounded once more
    raw = np.array([[2050.0, 1.0]], dtype=h)
    b = np.array([1.0, 2.0 ** -11], dtype=h)
    assert R.final_scores(raw, (), b).tolist() == [[2052.0, 1.0]]  # 2051 ties to even; 1 + 2^-11 ties to even
    assert R.final_scores(raw, [0], b).tolist() == [[1.0, 1.0]]     # removed -> 0, then the bias
    # the product rounds once from the exact fp32 product
    y = np.array([[1.0009765625, 3.0, 1.0009765625, 2.0]], dtype=h)
    r = R.route(y, np.array([0, 0]), 1, 1)
    assert r["out"].tolist() == [[float(h(np.float32(1.0009765625) ** 2)), 6.0]]


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------

def _assert_quantised(g, labels, E):
    g64 = g.astype(np.float64)
    assert np.array_equal(g64 / R.Q, np.round(g64 / R.Q)) and np.abs(g64).max() <= R.GMAX
    sizes = np.bincount(labels, minlength=E)
    assert sizes.max() <= 400
    # |partial sum| <= 400 * 8 = 3200 < 2^12 in units of 2^-8: 20 bits
    assert sizes.max() * np.abs(g64).max() / R.Q < 2 ** 20
    ga = R.relu16(g)
    s64, s32 = R.scores(ga, labels, E, "float64"), R.scores(ga, labels, E, "float32")
    assert np.array_equal(s64.view(np.uint16), s32.view(np.uint16))
    return s64


def _kth_tie_rows(score, k):
    s = np.sort(np.where(score == 0, 0, score.astype(np.float32)), axis=1)[:, ::-1]
    return (s[:, k - 1] == s[:, k]) if 0 < k < score.shape[1] else np.zeros(score.shape[0], bool)


def _straddles(score, sel, b):
    """Rows where experts b-1 | b tie and the selection ends between them."""
    return (score[:, b - 1] == score[:, b]) & sel[:, b - 1] & ~sel[:, b]


@pytest.mark.parametrize("E,F,M,kmid,b", R.LAYOUT_CASES + [c for c in R.BIAS_CASES if c not in R.LAYOUT_CASES])
def test_layout_cases_keep_their_edges(E, F, M, kmid, b):
    c = R.layout_case(E, F, M, kmid, b)
    labels = c["labels"]
    sizes = np.bincount(labels, minlength=E)
    assert labels.shape == (F,) and F % 8 == 0
    s = _assert_quantised(c["gate_q"], labels, E)
    assert {0, 1, E} <= set(c["ks"]) and (E <= 2 or 1 < kmid < E)
    if E >= 3:
        assert all(sizes[e] == 0 for e in c["empties"]) and c["empties"]
        assert len(set(sizes.tolist())) > 1  # not balanced
        assert [c["empties"][0]] in c["removed"]
    if F >= 320:
        assert sizes.max() > 64 and sizes[c["big"]] == sizes.max()
    assert list(range(E)) in c["removed"] and [] in c["removed"]
    if E > 1:
        assert _kth_tie_rows(s, kmid if c["boundary"] else 1).any()
    if c["boundary"]:
        assert _straddles(s, R.select(s, kmid), b)[0]
        assert any(b - 1 in r for r in c["removed"][:-1])  # a tied expert is removed in one of the lists
        assert sizes[b - 1] > 0 and sizes[b] > 0


def test_layout_cases_cover_every_boundary_and_size():
    cases = [R.layout_case(*c) for c in R.LAYOUT_CASES]
    assert {c["boundary"] for c in cases} >= set(R.BOUNDARIES)
    assert {c["E"] for c in cases} == {1, 3, 33, 64, 65, 100, 128, 129, 200, 256}
    assert {c["F"] for c in cases} == {8, 64, 320, 1288} and {c["M"] for c in cases} == {1, 5, 7}
    assert any(np.bincount(c["labels"], minlength=c["E"]).max() == 300 for c in cases)


@pytest.mark.parametrize("E,F,M,kmid,b", R.GELU_CASES)
def test_gelu_cases_keep_their_edges(E, F, M, kmid, b):
    c = R.gelu_case(E, F, M, kmid, b)
    g = c["gate"]
    a = np.abs(g.astype(np.float32))
    assert (((a >= 2.0 ** -5) & (a < 8)) | (a == 0)).all()
    ga = Fn.gelu(torch.from_numpy(g)).numpy()
    s = R.scores(ga, c["labels"], E, "float32")
    sizes = np.bincount(c["labels"], minlength=E)
    live = sizes > 0
    assert (s[0, live] < 0).all(), "row 0: every live expert scores below 0"
    rm = next(r for r in c["removed"] if c["removed_live"] in r)
    assert sizes[c["removed_live"]] > 0
    y = np.concatenate([c["value"], g], 1)
    # the removed live expert scores 0 like the empty ones: with a place for each of them it is selected ahead of
    # every live expert, never kept, and nothing of the row survives
    nzero = int((~live).sum()) + 1
    r = R.route(y, c["labels"], E, nzero, gate_act=ga, removed=rm, form="float32")
    assert r["sel"][0, c["removed_live"]] and not r["keep"][0, c["removed_live"]] and not r["out"][0].any()
    assert nzero <= kmid and (r["sel"][0] == (r["score"][0] == 0)).all()
    if c["boundary"]:
        assert _straddles(s, R.select(s, kmid), c["boundary"])[1] and _kth_tie_rows(s, kmid)[1]


@pytest.mark.parametrize("esize", R.ESIZES)
def test_score_epilogue_inputs_are_order_independent(esize):
    for F in (80, 320, 1280):
        _, gate, _ = R.fused_rows(F, esize)
        _assert_quantised(gate, np.arange(F) // esize, F // esize)


def test_ln_case_inputs_are_exact():
    x, w = R.ln_case_operands(320)
    assert set(np.unique(x).tolist()) == {-1.0, 1.0} and (x.astype(np.float64).sum(1) == 0).all()
    y64 = x.astype(np.float64) @ w.astype(np.float64).T
    assert np.array_equal(y64.astype(h).astype(np.float64), y64) and np.abs(y64).max() <= R.GMAX  # y exact in fp16
    _assert_quantised(y64[:, 320:].astype(h), np.arange(320) // 8, 40)


@pytest.mark.parametrize("esize,F,k", R.CHAIN_CASES)
def test_chain_cases_keep_their_edges(esize, F, k):
    E = F // esize
    assert F % 80 == 0 and E <= 256 and 40 % esize == 0 and 0 < k < E
    labels = R.chain_labels(F, esize)
    assert (np.bincount(labels, minlength=E) == esize).all()
    _, gate, tied = R.fused_rows(F, esize, labels=labels, k=k)
    s = _assert_quantised(gate, labels, E)
    sel = R.select(s, k)
    assert _kth_tie_rows(s, k)[0] and (s[0] == s[0, 0]).all()
    assert (s[1] == 0).all() and (gate[1] < 0).all()
    assert _kth_tie_rows(s, k)[8:].any(), "the coarse random rows tie at the k-th place as well"
    assert set(tied) == {b for b in R.BOUNDARIES if b < E}
    for b, row in tied.items():
        assert _straddles(s, sel, b)[row]


def test_chain_cases_cover_sizes_and_partial_slots():
    assert {c[0] for c in R.CHAIN_CASES} == set(R.ESIZES)
    Es = {F // es for es, F, _ in R.CHAIN_CASES}
    assert any(64 < E < 128 for E in Es) and any(128 < E < 256 for E in Es) and {64, 128, 256} <= Es
    assert any(F % 64 for _, F, _ in R.CHAIN_CASES) and any(F % 64 == 0 for _, F, _ in R.CHAIN_CASES)


@pytest.mark.parametrize("E,esize,M,ld", R.TOPK_CASES)
def test_topk_cases_keep_their_edges(E, esize, M, ld):
    c = R.topk_case(E, esize, M, ld)
    sc, k, rm, rows = c["score"], c["k"], c["removed"], c["rows"]
    assert sc.shape == (M, ld) and not np.isnan(sc.astype(np.float32)).any()
    s = R.final_scores(sc[:, :E], rm)
    sel = R.select(s, k)
    keep = R.keep_of(sel, rm)
    bits = sc[len(rows):, :E].view(np.uint16)
    assert np.isinf(sc).any() and ((bits & 0x7c00) == 0).any() and (bits >> 15).any()  # inf, subnormals, negatives
    assert (s[rows["all_equal"]] [[e for e in range(E) if e not in rm]] == h(1.5)).all()
    zr = s[rows["zeros_mixed"]]
    kth = np.sort(np.where(zr == 0, 0, zr.astype(np.float32)))[::-1][k - 1]
    tied0 = sc[rows["zeros_mixed"], :E][(zr == 0)]
    assert kth == 0 and np.signbit(tied0).any() and (~np.signbit(tied0)).any()
    assert (zr == 0).sum() > k - (zr > 0).sum() > 0  # more zeros than the places left for them
    for b in R.BOUNDARIES:
        if b < E and b - 1 not in rm and b not in rm:
            assert _straddles(s, sel, b)[rows[f"tie_{b}"]]
    assert {b for b in R.BOUNDARIES if b < E} <= {int(n[4:]) for n in rows if n.startswith("tie_")}
    assert np.isposinf(s[rows["many_inf"]]).sum() > k
    for name in ("all_negative", "all_negative_extremes"):
        r = rows[name]
        live = [e for e in range(E) if e not in rm]
        assert (sc[r, live] < 0).all()
        assert sel[r, rm].all() and not keep[r, rm].any() and sel[r].sum() == k and keep[r].sum() == k - len(rm)
    assert (sc[rows["all_negative_extremes"], :E] == h(-65504)).any()
    assert (sc[rows["largest_finite"], :E] == h(65504)).any()


def test_topk_cases_cover_the_kernels():
    cs = R.TOPK_CASES
    assert {c[0] for c in cs} == {16, 48, 64, 128, 256} and {c[2] for c in cs} == {70, 513}
    assert any(es == 10 and E <= 64 for E, es, _, _ in cs)
    for E in (64, 128, 256):  # aligned rows (quad FULL / group kernels) and unaligned ones (ballot kernel)
        assert any(c[0] == E and c[1] == 20 and c[3] % 8 == 0 for c in cs)
        assert any(c[0] == E and c[1] == 20 and c[3] % 8 for c in cs)
