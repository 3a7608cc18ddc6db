"""Plain numpy restatement of the routed GEGLU (MOEFy / RemoveExperts hooks) for ANY expert layout: unequal,
empty, scattered experts, any E and k. It shares no code with the product or with oracle/hooks_ref.py (which it is
checked against in tests/test_route_ref_host.py); the GPU tests in tests/test_gpu_route_layouts.py compare the HIP
kernels with it bit for bit.

From a projection output y [M, 2F] fp16 (value | gate), labels [F], E, k:
  gate    relu(gate) in fp16 (exact), or the caller's activated gate (GELU: torch's F.gelu of the fp16 tensor)
  score   per expert, the activated gates of its neurons summed in ascending neuron id, rounded ONCE to fp16
            form "float64": the exact sum (an fp16 is a multiple of 2^-24 below 2^16, so a float64 holds the exact
                            sum of up to 2^12 of them), rounded once
            form "float32": acc = fp32(acc + g) neuron by neuron, as the kernels sum
          a removed expert scores exactly +0; an empty expert scores +0; a bias is then added in fp32 and the
          result rounded once to fp16
  sel     the first k experts of a stable descending order of the fp16 scores with -0 == +0: ties at the k-th
          score go to the lowest expert id
  keep    sel and not removed
  out     fp16(value * gate) where the neuron's expert is kept, else 0; gate_out masked likewise
  words   the keep bits of the neurons in expert-major order (stable sort by label), 64 per word: [F/64, M]
"""
import numpy as np


def relu16(g):
    g = np.asarray(g, dtype=np.float16)
    return np.where(g > 0, g, np.float16(0)).astype(np.float16)


def expert_lists(labels, E):
    """Neuron ids of every expert, ascending."""
    labels = np.asarray(labels).astype(np.int64)
    assert labels.ndim == 1 and (labels.size == 0 or (labels.min() >= 0 and labels.max() < E))
    return [np.flatnonzero(labels == e) for e in range(E)]


def scores(gact, labels, E, form="float64"):
    """fp16 [M, E]: each expert's activated gates summed in ascending neuron id, one rounding to fp16."""
    gact = np.asarray(gact, dtype=np.float16)
    M = gact.shape[0]
    out = np.zeros((M, E), dtype=np.float16)
    for e, ids in enumerate(expert_lists(labels, E)):
        if form == "float64":
            assert ids.size <= 4096
            out[:, e] = gact[:, ids].astype(np.float64).sum(axis=1).astype(np.float16)
        elif form == "float32":
            acc = np.zeros(M, dtype=np.float32)
            for n in ids:
                acc = (acc + gact[:, n].astype(np.float32)).astype(np.float32)
            out[:, e] = acc.astype(np.float16)
        else:
            raise ValueError(form)
    return out


def final_scores(raw, removed=(), bias=None):
    """Removed experts score +0, then the bias is added in fp32 and the sum rounded once to fp16."""
    s = np.array(raw, dtype=np.float16, copy=True)
    if len(removed):
        s[:, sorted(set(int(e) for e in removed))] = np.float16(0)
    if bias is not None:
        s = (s.astype(np.float32) + np.asarray(bias, dtype=np.float16).astype(np.float32)[None, :]).astype(np.float16)
    return s


def select(score16, k):
    """bool [M, E]: the first k of a stable descending order of the fp16 scores, -0 == +0 (no NaN)."""
    s = np.asarray(score16, dtype=np.float16).astype(np.float32)
    assert not np.isnan(s).any(), "the selection rule defines no order for NaN"
    M, E = s.shape
    assert 0 <= k <= E
    s = np.where(s == 0, np.float32(0), s)  # -0 -> +0
    sel = np.zeros((M, E), dtype=bool)
    for m in range(M):
        # descending, equal scores in ascending expert id: sort by (-score, id)
        order = sorted(range(E), key=lambda e: (-s[m, e], e))
        sel[m, order[:k]] = True
    return sel


def keep_of(sel, removed=()):
    keep = np.array(sel, dtype=bool, copy=True)
    if len(removed):
        keep[:, sorted(set(int(e) for e in removed))] = False
    return keep


def expert_major(labels):
    """perm[j] = original id of the neuron at expert-major position j (stable by label)."""
    return np.argsort(np.asarray(labels).astype(np.int64), kind="stable")


def keep_words(keep_e, labels):
    """uint64 [F/64, M]: bit j of word (s, m) = expert-major neuron 64 s + j of row m kept."""
    labels = np.asarray(labels).astype(np.int64)
    F = labels.size
    assert F % 64 == 0
    kn = keep_e[:, labels[expert_major(labels)]]  # [M, F] in expert-major order
    M = kn.shape[0]
    w = np.zeros((F // 64, M), dtype=np.uint64)
    for j in range(64):
        w |= kn[:, j::64].T.astype(np.uint64) << np.uint64(j)
    return w


def sel_words(sel):
    """uint32 [M, ceil(E/32)]: bit e % 32 of word e // 32."""
    M, E = sel.shape
    w = np.zeros((M, (E + 31) // 32), dtype=np.uint32)
    for e in range(E):
        w[:, e >> 5] |= sel[:, e].astype(np.uint32) << np.uint32(e & 31)
    return w


def route(y, labels, E, k, *, gate_act=None, removed=(), bias=None, form="float64"):
    """The whole routed GEGLU. gate_act None: ReLU of y's gate half; else the activated fp16 gate [M, F].
    Returns dict(score, sel, keep, gate, out): score fp16 [M, E] (removed -> 0, bias added), sel / keep bool [M, E],
    gate / out fp16 [M, F]."""
    y = np.asarray(y, dtype=np.float16)
    labels = np.asarray(labels).astype(np.int64)
    F = labels.size
    assert y.ndim == 2 and y.shape[1] == 2 * F
    value = y[:, :F]
    g = relu16(y[:, F:]) if gate_act is None else np.asarray(gate_act, dtype=np.float16)
    assert g.shape == value.shape
    sc = final_scores(scores(g, labels, E, form), removed, bias)
    sel = select(sc, k)
    keep = keep_of(sel, removed)
    kn = keep[:, labels] if F else np.zeros((y.shape[0], 0), bool)
    prod = (value.astype(np.float32) * g.astype(np.float32)).astype(np.float16)  # 22-bit product: exact in fp32
    zero = np.float16(0)
    return dict(score=sc, sel=sel, keep=keep, gate=np.where(kn, g, zero).astype(np.float16),
                out=np.where(kn, prod, zero).astype(np.float16))


# ---------------------------------------------------------------------------------------------------------------
# Inputs of tests/test_gpu_route_layouts.py, generated from seeds (numpy only). tests/test_route_ref_host.py asserts,
# without a GPU, that each of them still carries the edge it exists for.

Q = 2.0 ** -8          # quantised gates: multiples of 2^-8 with |g| <= 8 (exact in fp16); any partial sum of up to
GMAX = 8.0             # 400 of them needs at most 20 bits, so fp32 and float64 sums agree whatever the order
BOUNDARIES = (16, 32, 64, 128)  # lane (15|16), selection word (31|32) and 64-expert slot (63|64, 127|128) edges


def quant_gates(rng, shape, amax=GMAX):
    n = int(round(amax / Q))
    return (rng.integers(-n, n + 1, size=shape).astype(np.float64) * Q).astype(np.float16)


def special_experts(E):
    return sorted({b - 1 for b in BOUNDARIES if b < E} | {b for b in BOUNDARIES if b < E})


def unbalanced_labels(rng, E, F):
    """Scattered labels with sizes from 0 upward, one large expert (300 neurons where F allows, else F // 2), at
    least one empty expert (E >= 3) and the experts on both sides of every boundary non-empty.
    Returns (labels, big, empties)."""
    if E == 1:
        return np.zeros(F, dtype=np.int64), 0, []
    special = special_experts(E)
    big = 1
    empties = []
    if E >= 3:
        empties.append(next(e for e in (E - 1, E - 2, E - 3, E - 4) if e not in special and e != big))
    if E > 8:
        empties.append(5)
    sizes = np.zeros(E, dtype=np.int64)
    sizes[big] = min(300, F // 2)
    for e in special:
        sizes[e] = 1
    rest = F - int(sizes.sum())
    assert rest >= 0
    open_ = np.array([e for e in range(E) if e not in empties and e != big])
    np.add.at(sizes, open_[rng.integers(0, open_.size, size=rest)], 1)
    labels = np.repeat(np.arange(E), sizes)
    assert labels.size == F
    return labels[rng.permutation(F)], big, empties


def tie_score_plan(E, k, b, usable):
    """Per-expert target scores of a row tied at the k-th place across experts b-1 | b: k-1 experts (the highest
    usable ids) above, experts b-1 and b equal, everything else below."""
    assert 1 <= k and b - 1 in usable and b in usable
    high = [e for e in sorted(usable, reverse=True) if e not in (b - 1, b)][:k - 1]
    assert len(high) == k - 1
    plan = {e: 0.25 for e in usable}
    for i, e in enumerate(high):
        plan[e] = 2.0 + (i % 7) * 0.25
    plan[b - 1] = plan[b] = 1.0
    return plan


def gate_row_from_plan(rng, labels, E, plan, fill="neg"):
    """A gate row whose expert sums are exactly `plan` under ReLU (fill 'neg': all other gates negative) or under any
    activation with act(0) = 0 (fill 'zero'): the expert's lowest neuron carries the whole score."""
    F = labels.size
    if fill == "neg":
        row = -np.abs(quant_gates(rng, F)).astype(np.float64) - Q
        row = np.maximum(row, -GMAX)
    else:
        row = np.zeros(F)
    for e, v in plan.items():
        ids = np.flatnonzero(labels == e)
        if ids.size:
            row[ids[0]] = v
    return row.astype(np.float16)


# (E, F, M, middle k, b): every E, F and M the unfused kernel is run at; the middle k is where the hand-made row
# ties, b the boundary that tie straddles (0: E too small for one)
LAYOUT_CASES = [(1, 8, 1, 1, 0), (1, 320, 5, 1, 0), (3, 8, 7, 2, 0), (3, 64, 5, 2, 0), (33, 64, 1, 9, 32),
                (33, 320, 7, 5, 16), (64, 1288, 5, 12, 32), (65, 320, 7, 13, 64), (65, 1288, 1, 30, 16),
                (100, 1288, 7, 20, 64), (128, 320, 5, 25, 64), (129, 1288, 7, 26, 128), (200, 1288, 5, 40, 128),
                (256, 320, 1, 51, 64), (256, 1288, 7, 100, 128)]
BIAS_CASES = [(33, 320, 7, 5, 16), (100, 1288, 5, 20, 64), (200, 1288, 7, 40, 128)]
GELU_CASES = [(3, 64, 5, 2, 0), (33, 320, 7, 5, 32), (65, 1288, 5, 13, 64), (129, 1288, 7, 26, 128),
              (256, 1288, 7, 51, 16)]


def layout_case(E, F, M, kmid, b, seed=0):
    """Unfused-kernel case: unbalanced labels, quantised gates whose row 0 is tied at the kmid-th place across the
    case's boundary (E > 16), plain randn * 1.5 gates for the summation-order check, the k and removed lists."""
    rng = np.random.default_rng(1000 * E + F + 7 * M + seed)
    labels, big, empties = unbalanced_labels(rng, E, F)
    value = (rng.standard_normal((M, F)) * 1.5).astype(np.float16)
    gq = quant_gates(rng, (M, F))
    assert b == 0 or (b in BOUNDARIES and b < E)
    usable = [e for e in range(E) if (labels == e).any()]
    if b:
        gq[0] = gate_row_from_plan(rng, labels, E, tie_score_plan(E, kmid, b, usable))
    elif E > 1:
        gq[0] = -np.abs(gq[0]) - np.float16(Q)  # every score 0: tied at every k < E
    gp =(rng.standard_normal((M, F)) * 1.5).astype(np.float16)
    ks = sorted({0, 1, kmid, E})
    removed = [[]]
    if empties:
        removed.append([empties[0]])
    if b:
        removed.append(sorted({b - 1, big, int(rng.integers(0, E))}))
    removed.append(list(range(E)))
    bias = quant_gates(rng, E, 4.0)
    return dict(E=E, F=F, M=M, kmid=kmid, labels=labels, big=big, empties=empties, boundary=b, value=value,
                gate_q=gq, gate_plain=gp, ks=ks, removed=removed, bias=bias)


def gelu_range_gates(rng, shape):
    """fp16 gates with 2^-5 <= |x| < 8, or 0: the range where the kernels apply the registered GELU table."""
    mag = rng.integers(0x2800, 0x4800, size=shape).astype(np.uint16)  # 2^-5 .. just under 8
    sign = (rng.integers(0, 2, size=shape).astype(np.uint16)) << np.uint16(15)
    g = (mag | sign).view(np.float16)
    return np.where(rng.random(shape) < 0.05, np.float16(0), g).astype(np.float16)


def gelu_case(E, F, M, kmid, b, seed=0):
    """GELU case: gates in the table's range; row 0 all negative (with a non-empty removed expert, which then scores
    0 above every live expert), row 1 tied at the kmid-th place across the boundary (E > 16)."""
    rng = np.random.default_rng(2000 * E + F + 7 * M + seed)
    labels, big, empties = unbalanced_labels(rng, E, F)
    value = (rng.standard_normal((M, F)) * 1.5).astype(np.float16)
    gate = gelu_range_gates(rng, (M, F))
    # gelu(x) of x in [-3, -0.125] is a negative fp16 normal: every live expert's sum is then negative
    gate[0] = -(rng.integers(32, 769, size=F).astype(np.float64) * Q).astype(np.float16)
    assert b == 0 or (b in BOUNDARIES and b < E)
    usable = [e for e in range(E) if (labels == e).any()]
    if b and M > 1:
        gate[1] = gate_row_from_plan(rng, labels, E, tie_score_plan(E, kmid, b, usable), fill="zero")
    live = [e for e in usable if e != big]
    rem_live = live[len(live) // 2]
    removed = [[], [rem_live] + empties[:1], list(range(E))]
    return dict(E=E, F=F, M=M, kmid=kmid, labels=labels, big=big, empties=empties, boundary=b, value=value,
                gate=gate, ks=sorted({0, 1, kmid, E}), removed=removed, removed_live=rem_live)


# ---- fused path (sdmoe_linear_geglu's score epilogue, sdmoe_moe_topk_mask / _keep): 64 chosen rows of exact fp16
# value / gate values; GEMM row m produces row m % 64
ESIZES = (1, 2, 4, 5, 8, 10, 20, 40)


def fused_rows(F, esize, seed=0, labels=None, k=0):
    """value, gate fp16 [64, F] (gates quantised; rows 8.. on a coarse grid of quarters so that expert sums tie
    often), with hand-made rows: 0 all gates equal, 1 all gates negative, 2.. one tie row per boundary below E."""
    rng = np.random.default_rng(31 * F + esize + seed)
    E = F // esize
    if labels is None:
        labels = np.arange(F) // esize
    value = (rng.standard_normal((64, F)) * 1.5).astype(np.float16)
    gate = quant_gates(rng, (64, F))
    gate[8:] = (rng.integers(-4, 9, size=(56, F)) * 0.25).astype(np.float16)
    gate[0] = np.float16(0.5)
    gate[1] = -np.abs(gate[1]) - np.float16(Q)
    tied = {}
    if 1 <= k < E:
        for i, b in enumerate(bb for bb in BOUNDARIES if bb < E and k - 1 <= E - 2):
            gate[2 + i] = gate_row_from_plan(rng, labels, E, tie_score_plan(E, k, b, list(range(E))))
            tied[b] = 2 + i
    return value, gate, tied


def ln_case_operands(F, seed=0):
    """LN-folded GEMM with an exact result: x [64, 64] rows of +-1 that sum to 0 (mean 0, variance 1: with gamma 1,
    beta 0, eps 0 the norm is the identity) and W [2F, 64] multiples of 2^-8 up to 1/8, so that y = x W^T is a
    multiple of 2^-8 with |y| <= 8: exact in fp32 in any order, and an fp16 value."""
    rng = np.random.default_rng(900 + F + seed)
    x = np.ones((64, 64), dtype=np.float16)
    for r in range(64):
        x[r, rng.permutation(64)[:32]] = -1
    w = (rng.integers(-32, 33, size=(2 * F, 64)).astype(np.float64) * Q).astype(np.float16)
    return x, w


# chains (esize, F, k): F % 64 == 0 is needed by the keep words, so keep runs where 320 | F; elsewhere the mask
# chain alone runs and keep must refuse the shape. E = 80 and 160 fill the SLOTS = 2 / 4 forms only partly.
CHAIN_CASES = [(1, 80, 20), (1, 240, 60), (2, 320, 40), (2, 160, 16), (4, 320, 20), (4, 640, 70), (5, 320, 13),
               (5, 400, 20), (5, 1280, 130), (8, 320, 10), (8, 1280, 70), (10, 320, 6), (10, 640, 20),
               (10, 1280, 65), (20, 320, 4), (20, 1280, 17), (20, 2560, 30), (40, 320, 2), (40, 2560, 17),
               (40, 5120, 33)]


def chain_labels(F, esize, seed=0):
    """Balanced experts scattered over the neurons."""
    rng = np.random.default_rng(77 * F + esize + seed)
    return rng.permutation(F) % (F // esize)


# ---- top-k on the whole fp16 key space: (E, esize, M, ld)
TOPK_CASES = [(16, 20, 70, 16), (16, 20, 513, 24), (48, 20, 70, 48), (48, 20, 513, 51), (64, 20, 513, 64),
              (64, 20, 70, 72), (64, 20, 70, 67), (64, 10, 70, 64), (64, 10, 513, 65), (128, 20, 513, 128),
              (128, 20, 70, 130), (256, 20, 70, 256), (256, 20, 513, 264), (256, 20, 70, 259)]


def topk_case(E, esize, M, ld, seed=0):
    """Scores [M, ld] over every finite fp16 bit pattern and +-inf (no NaN); the first rows are hand-made. Returns
    dict(score [M, ld], k, removed, rows: name -> row index)."""
    rng = np.random.default_rng(5000 * E + 3 * M + ld + esize + seed)
    bits = rng.integers(0, 65536, size=(M, ld)).astype(np.uint16)
    nan = ((bits & 0x7c00) == 0x7c00) & ((bits & 0x03ff) != 0)
    bits[nan] &= np.uint16(0xfc00)  # NaN -> the infinity of its sign
    score = bits.view(np.float16).copy()
    k = max(2, E // 5)
    removed = sorted({1, E // 2 + 3, E - 1})
    rows = {}
    r = 0
    h = np.float16

    def put(name, row):
        nonlocal r
        score[r, :E] = row
        rows[name] = r
        r += 1
    put("all_equal", np.full(E, 1.5, dtype=h))
    z = np.full(E, -2.0, dtype=h)            # k-1 positives above, then +0 / -0 alternating at the boundary
    z[E - (k - 1):] = h(3.0)
    z[2:8:2] = h(0.0)
    z[3:8:2] = h(-0.0)
    z[1] = h(7.0)                            # (removed: scores 0 like the zeros around it)
    put("zeros_mixed", z)
    for b in (bb for bb in BOUNDARIES if bb < E):
        usable = [e for e in range(E) if e not in removed]
        if b - 1 in usable and b in usable:
            plan = tie_score_plan(E, k, b, usable)
            row = np.array([plan.get(e, -1.0) for e in range(E)], dtype=h)
            put(f"tie_{b}", row)
    inf = (rng.standard_normal(E) * 100).astype(h)
    inf[0] = h(-np.inf)
    live = np.array([e for e in range(1, E) if e not in removed])
    inf[live[rng.permutation(live.size)[:k + 2]]] = h(np.inf)   # more +inf than places
    put("many_inf", inf)
    neg = -np.abs(rng.standard_normal(E) * 50).astype(h) - h(Q)
    put("all_negative", neg)                 # removed experts score 0: selected first, never kept
    neg2 = neg.copy()
    neg2[::3] = h(-65504.0)
    neg2[2::7] = h(-6e-8)                    # the smallest subnormal
    put("all_negative_extremes", neg2)
    big = (rng.standard_normal(E) * 1000).astype(h)
    big[::4] = h(65504.0)
    big[1::4] = h(6e-8)
    put("largest_finite", big)
    assert r <= M
    return dict(E=E, esize=esize, M=M, ld=ld, score=score, k=k, removed=removed, rows=rows)
