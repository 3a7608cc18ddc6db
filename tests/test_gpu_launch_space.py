"""The launch space of the GEMM / conv kernel that the U-Net's own shapes never visit: forced split-K counts on every
launch family (sdmoe_tune knob 9), both split-K tile orders (knob 14), both residual epilogues (knob 8), forced tiles
under a split (knob 1), non-square convs on every shifted and halo tile, and a weight with ldw > K.

Two things keep a pass from being vacuous:
  * every case first asks sdmoe_gemm_plan / sdmoe_conv_plan, under the same knobs and with the same workspace size,
    what the library will launch, and asserts that this is the split (tile, halo family) the case means to test;
  * every launch runs on a private split-K workspace sized exactly ksplit * M * N floats, filled with NaN, between two
    guard bands: afterwards the guards are bit-unchanged, every slab element was written (finite) and nothing behind
    the slabs was touched. A reduce that reads a slab row no workgroup wrote therefore sums a NaN instead of the right
    value a previous call happened to leave in the shared 32 M-float workspace.

Tolerance: test_gpu_kernels.close (max-abs <= 1e-2 * max(1, max |ref|) and rel-L2 <= 2e-3) against a torch fp32
reference of the same op; conv references are computed once per geometry on the host and shared.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sdmoe import _lib, ops  # noqa: E402
from sdmoe.tune import tuned  # noqa: E402
from test_gpu_kernels import DEV, close, conv_ref, rnd  # noqa: E402

SENTINEL = 12345.0


class _Workspace:
    def __init__(self, device, floats, guard):
        assert guard % 4 == 0 and floats >= 0  # the slab stores are 16 B: the middle stays 16-B aligned
        self.guard, self.floats = guard, floats
        self.buf = torch.full((guard + floats + guard,), float("nan"), dtype=torch.float32, device=device)
        self.buf[:guard] = SENTINEL
        self.buf[guard + floats:] = SENTINEL
        self.view = self.buf[guard:guard + floats]
        self._guards = self._guard_bits().clone()

    def _guard_bits(self):
        bits = self.buf.view(torch.int32)
        return torch.cat([bits[:self.guard], bits[self.guard + self.floats:]])

    def check(self, written):
        """Guards bit-unchanged; the first `written` floats all finite (every slab element stored); the rest NaN."""
        torch.cuda.synchronize()
        assert 0 <= written <= self.floats
        assert torch.equal(self._guard_bits(), self._guards), "a store landed outside the workspace"
        head, tail = self.view[:written], self.view[written:]
        nbad = int((~torch.isfinite(head)).sum())
        assert nbad == 0, f"{nbad} of {written} slab floats were never written"
        ntouched = int((~torch.isnan(tail)).sum())
        assert ntouched == 0, f"{ntouched} floats behind the {written} slab floats were written"


@contextlib.contextmanager
def private_workspace(device, floats, guard=1024):
    """Install a NaN-filled fp32 workspace of exactly `floats` elements (between two `guard`-float sentinel bands) as
    the split-K workspace ops hands to the library on `device`; ops passes its numel() as workspace_floats."""
    ws = _Workspace(device, floats, guard)
    missing = object()
    prev = ops._WS.get(device, missing)
    ops._WS[device] = ws.view
    try:
        yield ws
    finally:
        if prev is missing:
            del ops._WS[device]
        else:
            ops._WS[device] = prev


def device():
    return torch.device("cuda", torch.cuda.current_device())


def expected_splits(nk, ks):
    """Splits of nk K units at a forced count ks (knob 9): ks clamped to nk, ceil(nk / ks) units per split, and as
    many splits as that takes -- no empty trailing split."""
    kchunk = -(-nk // min(ks, nk))
    return -(-nk // kchunk)


def test_expected_splits_examples():
    assert [expected_splits(11, ks) for ks in (2, 3, 4, 5, 7, 32)] == [2, 3, 4, 4, 6, 11]
    assert [expected_splits(9, ks) for ks in (1, 2, 4, 9)] == [1, 2, 3, 9]
    assert [expected_splits(4, ks) for ks in (1, 3, 4)] == [1, 2, 4]


def run_gemm(mode, M, N, K, ksplit, call, *, residual=False, act=ops.ACT_NONE, tile=None, floats=None):
    """call() on a private workspace of `floats` (default ksplit * M * N) after asserting that the library, under the
    knobs in force and with that workspace, plans `ksplit` splits (and `tile` = (tile, waves) where given)."""
    floats = ksplit * M * N if floats is None else floats
    plan = ops.gemm_plan(mode, M, N, K, residual=residual, act=act, workspace_floats=floats)
    assert plan["ksplit"] == ksplit, (plan, ksplit)
    if tile is not None:
        assert (plan["tile"], plan["waves"]) == tile, (plan, tile)
    with private_workspace(device(), floats) as ws:
        out = call()
        ws.check(ksplit * M * N if ksplit > 1 else 0)
    return out


def run_conv(nimg, H, W, Cin, Cout, ksplit, call, *, halo, tile=None, Cin2=0, stride=1, upsample=False, residual=False,
             gn=False, act=ops.ACT_NONE):
    """The conv counterpart of run_gemm: asserts the halo / shifted family too."""
    OH, OW = (2 * H, 2 * W) if upsample else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    M = nimg * OH * OW
    floats = ksplit * M * Cout
    plan = ops.conv_plan(nimg, H, W, Cin, Cout, Cin2=Cin2, stride=stride, upsample=upsample, residual=residual, gn=gn,
                         act=act, workspace_floats=floats)
    assert plan["halo"] == halo and plan["ksplit"] == ksplit, (plan, halo, ksplit)
    if tile is not None:
        assert plan["tile"] == tile, (plan, tile)
    with private_workspace(device(), floats) as ws:
        out = call()
        ws.check(ksplit * M * Cout if ksplit > 1 else 0)
    return out


def rel_l2(out, ref):
    return ((out.float() - ref.float()).norm() / ref.float().norm()).item()


# ---- A. tile-family GEMM under forced splits ------------------------------------------------------------------------

def _linear_operands(M, N, K, seed):
    return (rnd(M, K, seed=seed), rnd(N, K, scale=K ** -0.5, seed=seed + 1), rnd(N, scale=0.1, seed=seed + 2),
            rnd(M, N, seed=seed + 3))


@pytest.mark.parametrize("M,N,K,ks", [(77, 320, 704, ks) for ks in (2, 3, 4, 5, 7, 32)] + [(1, 8, 128, 2)] +
                         [(130, 968, 320, 2), (130, 968, 320, 5)])
def test_linear_forced_splits(M, N, K, ks):
    """sdmoe_linear at forced split counts: an uneven last split (nk = 11 at 2, 3, 4), no empty trailing split (5 -> 4,
    7 -> 6), ks clamped to nk (32 -> 11), the smallest split there is (one row, 8 columns, two K-steps) and M and N
    tails on the 128-wide tiles under a split."""
    x, w, b, r = _linear_operands(M, N, K, 200)
    ksplit = expected_splits(K // 64, ks)
    if (M, N, K) == (77, 320, 704):
        assert ksplit == {2: 2, 3: 3, 4: 4, 5: 4, 7: 6, 32: 11}[ks]
    with tuned(ksplit=ks):
        out = run_gemm("plain", M, N, K, ksplit, lambda: ops.linear(x, w, b, residual=r), residual=True)
    close(out, x.float() @ w.float().t() + b.float() + r.float())


TILES = {1: ((128, 160), (2, 2)), 2: ((64, 160), (2, 2)), 3: ((256, 320), (2, 4)), 4: ((256, 160), (4, 2)),
         5: ((256, 320), (4, 2)), 6: ((128, 320), (2, 4)), 7: ((128, 160), (4, 2)), 8: ((64, 320), (2, 4))}


@pytest.mark.parametrize("tile", sorted(TILES))
def test_linear_forced_tiles_under_a_split(tile):
    """Every wave arrangement's slab store: (300, 1280, 640) at 3 splits (4 + 4 + 2 K-steps) on each forced tile, with
    an M tail in every one of them."""
    M, N, K = 300, 1280, 640
    x, w, b, _ = _linear_operands(M, N, K, 210)
    with tuned(ksplit=3, tile=tile):
        out = run_gemm("plain", M, N, K, 3, lambda: ops.linear(x, w, b), tile=TILES[tile])
    close(out, x.float() @ w.float().t() + b.float())


def _quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


EPILOGUES = ["bias", "silu", "gelu", "relu", "quick_gelu", "coladd", "res16", "res32", "act_res", "strided"]
ACT_FN = {"silu": (ops.ACT_SILU, F.silu), "gelu": (ops.ACT_GELU, F.gelu), "relu": (ops.ACT_RELU, F.relu),
          "quick_gelu": (ops.ACT_QUICK_GELU, _quick_gelu)}


@pytest.mark.parametrize("epi", EPILOGUES)
def test_linear_epilogues_through_the_reduce(epi):
    """Every epilogue the split-K reduce (epilogue8) runs, at (77, 320, 704) on 4 splits: bias, each activation, the
    per-batch column add, the residual on both paths (knob 8 = 1: output rounded to fp16, then added; 0: added in
    fp32), activation + residual, and row-strided x / residual / out views with sentinel columns around out."""
    M, N, K = 77, 320, 704
    x, w, b, r = _linear_operands(M, N, K, 220)
    acc = x.float() @ w.float().t() + b.float()
    knobs, kw, act, res = {"ksplit": 4}, {}, ops.ACT_NONE, False
    if epi == "bias":
        ref = acc
    elif epi in ACT_FN:
        act, fn = ACT_FN[epi]
        ref = fn(acc)
    elif epi == "coladd":
        col = rnd(M // 7, N, seed=225)
        kw = dict(coladd=col, coladd_bstride=N, rows_per_batch=7)
        ref = acc + col.float().repeat_interleave(7, 0)
    elif epi in ("res16", "res32"):
        knobs["res16"] = 1 if epi == "res16" else 0
        kw, res, ref = dict(residual=r), True, acc + r.float()
    elif epi == "act_res":
        act, kw, res, ref = ops.ACT_SILU, dict(residual=r), True, F.silu(acc) + r.float()
    else:
        xbig = rnd(M, K + 128, seed=226)
        rbig = rnd(M, N + 16, seed=227)
        dst = torch.full((M, N + 24), 3.0, dtype=torch.float16, device=DEV)
        x, r = xbig[:, 64:64 + K], rbig[:, 8:8 + N]
        kw, res = dict(residual=r, out=dst[:, 8:8 + N]), True
        ref = x.float() @ w.float().t() + b.float() + r.float()
    with tuned(**knobs):
        out = run_gemm("plain", M, N, K, 4, lambda: ops.linear(x, w, b, act=act, **kw), residual=res, act=act)
    close(out, ref)
    if epi == "strided":
        assert (dst[:, :8] == 3.0).all() and (dst[:, 8 + N:] == 3.0).all()


def test_linear_fp32_residual_unsplit():
    """Knob 8 = 0 without a split: the kernel's own fp32 residual epilogue (the non-res16 staging path)."""
    M, N, K = 256, 320, 320
    x, w, b, r = _linear_operands(M, N, K, 230)
    outs = {}
    for res16 in (0, 1):
        with tuned(ksplit=1, res16=res16):
            outs[res16] = run_gemm("plain", M, N, K, 1, lambda: ops.linear(x, w, b, residual=r), residual=True)
        close(outs[res16], x.float() @ w.float().t() + b.float() + r.float())


@pytest.mark.parametrize("extra,ksplit", [("3mn+4", 3), ("mn", 1), ("zero", 1)])
def test_linear_workspace_lowers_the_split(extra, ksplit):
    """Knob 9 = 8 at (77, 320, 704) on a workspace too small for 8 slabs: plan and launch agree on the lowered split
    (3 slabs + 4 spare floats: 3 splits, the spare floats untouched; one slab or no workspace at all: unsplit, nothing
    written)."""
    M, N, K = 77, 320, 704
    x, w, b, r = _linear_operands(M, N, K, 240)
    floats = {"3mn+4": 3 * M * N + 4, "mn": M * N, "zero": 0}[extra]
    with tuned(ksplit=8):
        assert ops.gemm_plan("plain", M, N, K, residual=True)["ksplit"] == 6  # (with room: 8 wanted -> 2 per split)
        out = run_gemm("plain", M, N, K, ksplit, lambda: ops.linear(x, w, b, residual=r), residual=True, floats=floats)
    close(out, x.float() @ w.float().t() + b.float() + r.float())


@pytest.mark.parametrize("ks,workspace", [(4, True), (1, True), (4, False)])
def test_linear_weight_row_stride_above_k(ks, workspace):
    """ldw > K (sdmoe_linear's contract; ops.linear insists on a contiguous weight): W is the column slice
    [:, 64 : 64 + K] of a [N, K + 128] matrix whose other columns are NaN, split and unsplit, and under a forced split
    with a null workspace (which must run unsplit)."""
    M, N, K = 77, 320, 704
    x, w, b, _ = _linear_operands(M, N, K, 250)
    wbig = torch.full((N, K + 128), float("nan"), dtype=torch.float16, device=DEV)
    wbig[:, 64:64 + K] = w
    wv = wbig[:, 64:64 + K]
    out = torch.empty((M, N), dtype=torch.float16, device=DEV)
    ksplit = expected_splits(K // 64, ks) if workspace else 1
    lib = _lib.load()

    def call():
        ws = ops._workspace(device())
        wsp, wsn = (ws.data_ptr(), ws.numel()) if workspace else (None, 0)
        st = lib.sdmoe_linear(x.data_ptr(), x.stride(0), wv.data_ptr(), wv.stride(0), b.data_ptr(), None, 0, 0, None, 0,
                              out.data_ptr(), out.stride(0), M, N, K, ops.ACT_NONE, wsp, wsn, ops._stream())
        _lib.check(st, "sdmoe_linear")
        return out
    with tuned(ksplit=ks):
        if workspace:
            run_gemm("plain", M, N, K, ksplit, call)
        else:
            assert ops.gemm_plan("plain", M, N, K, workspace_floats=0)["ksplit"] == 1
            with private_workspace(device(), 4 * M * N) as ws:  # (installed, not handed over: it stays NaN)
                call()
                ws.check(0)
    close(out, x.float() @ w.float().t() + b.float())


# ---- B. masked and per-image GEMMs under forced splits ------------------------------------------------------------

def _masks(M, N, K, seed):
    """Random keep words int64 [K/64, M] and packed Wanda bits uint8 [N, K/8] with their unpacked 0/1 matrices."""
    g = torch.Generator().manual_seed(seed)
    keep = (torch.randint(-2 ** 31, 2 ** 31, (K // 64, M), generator=g, dtype=torch.int64) << 32) | \
        torch.randint(0, 2 ** 32, (K // 64, M), generator=g, dtype=torch.int64)
    j = torch.arange(64, dtype=torch.int64)
    keep01 = ((keep.t()[:, :, None] >> j) & 1).reshape(M, K).to(torch.float16)  # bit j of word (s, m): neuron 64 s + j
    removed = (torch.rand(N, K, generator=g) < 0.3).to(torch.uint8)
    bits = torch.from_numpy(np.packbits(removed.numpy(), axis=-1, bitorder="little"))
    return keep.to(DEV), keep01.to(DEV), bits.to(DEV), removed.to(DEV)


@pytest.mark.parametrize("ks", [1, 3, 5])
@pytest.mark.parametrize("kind", ["keep", "wmask", "keepw", "linear_keep"])
def test_masked_linear_forced_splits(kind, ks):
    """sdmoe_linear_masked / sdmoe_linear_keep at (200, 320, 704) on 1, 3 and 4 splits (uneven, M tail): within the
    tolerance of the fp32 product of the unpacked masks, and bit-identical to sdmoe_linear on the operands masked first
    (include/sdmoe.h: the masked modes take the plain GEMM's split)."""
    M, N, K = 200, 320, 704
    x, w, b, r = _linear_operands(M, N, K, 300)
    keep, keep01, bits, removed = _masks(M, N, K, 304)
    ksplit = expected_splits(K // 64, ks)
    use_keep, use_w = kind in ("keep", "keepw", "linear_keep"), kind in ("wmask", "keepw")
    res = kind == "linear_keep"
    bias, rr = (b, r) if res else (None, None)
    xm = x * keep01 if use_keep else x
    with tuned(ksplit=ks):
        wm = ops.mask_weight(w, bits) if use_w else w
        if kind == "linear_keep":
            fn = lambda: ops.linear_keep(x, keep, w, bias, residual=rr)  # noqa: E731
        else:
            fn = lambda: ops.linear_masked(x, w, bias, keep=keep if use_keep else None,  # noqa: E731
                                           wmask=ops.wmask_kmajor(bits) if use_w else None, residual=rr)
        out = run_gemm("keep" if kind == "linear_keep" else kind, M, N, K, ksplit, fn, residual=res)
        plain = run_gemm("plain", M, N, K, ksplit, lambda: ops.linear(xm, wm, bias, residual=rr), residual=res)
    ref = xm.float() @ (w.float() * (1 - removed.float()) if use_w else w.float()).t()
    if res:
        ref = ref + b.float() + r.float()
    close(out, ref)
    assert torch.equal(out, plain)


@pytest.mark.parametrize("ks", [1, 4])
@pytest.mark.parametrize("res", [False, True])
def test_linear_per_image_forced_splits(res, ks):
    """sdmoe_linear_per_image (two images of 256 rows, their own weights and fp32 column add) unsplit and on 4 splits."""
    nimg, rpb, N, K = 2, 256, 320, 704
    M = nimg * rpb
    x = rnd(M, K, seed=310)
    wf = rnd(nimg, N, K, scale=K ** -0.5, seed=311)
    colf = rnd(nimg, N, seed=312).float()
    r = rnd(M, N, seed=313) if res else None
    ksplit = expected_splits(K // 64, ks)
    with tuned(ksplit=ks):
        out = run_gemm("plain", M, N, K, ksplit, lambda: ops.linear_per_image(x, wf, colf, rpb, residual=r), residual=res)
    ref = torch.cat([x[i * rpb:(i + 1) * rpb].float() @ wf[i].float().t() + colf[i] for i in range(nimg)])
    close(out, ref + (r.float() if res else 0))


# ---- C. shifted-tile convs, non-square, under forced splits ---------------------------------------------------------

# family -> (Cin, Cin2, Cout, nimg, H, W, stride, upsample, forced split counts); Cout % 320 != 0: never a halo tile
SHIFTED = {"stride1": (128, 0, 64, 2, 5, 7, 1, False, (1, 2, 4, 5, 18)),
           "stride2": (64, 0, 160, 3, 7, 10, 2, False, (1, 2, 4, 9)),
           "upsample": (64, 0, 128, 2, 3, 5, 1, True, (1, 2, 3)),
           "shortcut": (64, 128, 160, 2, 5, 6, 1, False, (1, 2, 3, 11))}


@functools.lru_cache(maxsize=None)
def _conv_problem(Cin, Cin2, Cout, nimg, H, W, stride, upsample, full):
    """Operands and the fp32 reference (computed on the host, once) of one conv geometry. full: bias + per-image column
    add + SiLU + residual (no residual with the folded shortcut: sdmoe_conv3x3_sc has none); else bias (+ the
    per-image column add with the shortcut). Also the reference with H and W exchanged."""
    seed = 400 + 7 * H + W + Cin
    OH, OW = (2 * H, 2 * W) if upsample else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    x = rnd(nimg * H * W, Cin, seed=seed)
    w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=seed + 1), rnd(Cout, scale=0.1, seed=seed + 2)
    col = rnd(nimg, Cout, seed=seed + 3)
    r = rnd(nimg * OH * OW, Cout, seed=seed + 4) if full and not Cin2 else None
    wc, kw, extra = ops.conv_weight(w), {}, 0
    if Cin2:
        x2, w2 = rnd(nimg * H * W, Cin2, seed=seed + 5), rnd(Cout, Cin2, scale=Cin2 ** -0.5, seed=seed + 6)
        wc, kw = ops.conv_weight_with_shortcut(wc, w2), dict(shortcut=x2)
        extra = x2.float() @ w2.float().t()
    if full or Cin2:
        kw.update(coladd=col, coladd_bstride=Cout)
        extra = extra + col.float().repeat_interleave(OH * OW, 0)
    if full:
        kw.update(act=ops.ACT_SILU)
    if r is not None:
        kw.update(residual=r)

    def reference(h, w_):
        v = conv_ref(x.cpu(), nimg, h, w_, w.cpu(), b.cpu(), stride, upsample).to(DEV) + extra
        if full:
            v = F.silu(v)
        return v + (r.float() if r is not None else 0)
    return x, wc, b, kw, reference(H, W), reference(W, H)


def _shifted_cases():
    for fam, (Cin, Cin2, Cout, nimg, H, W, stride, up, kss) in SHIFTED.items():
        for h, w in ((H, W), (W, H)):
            for ks in kss:
                yield pytest.param(fam, h, w, ks, False, id=f"{fam}-{h}x{w}-ks{ks}")
            yield pytest.param(fam, h, w, kss[2], True, id=f"{fam}-{h}x{w}-ks{kss[2]}-full")


@pytest.mark.parametrize("fam,H,W,ks,full", list(_shifted_cases()))
def test_shifted_conv_nonsquare_forced_splits(fam, H, W, ks, full):
    """The shifted-tile convs (stride 1, stride 2 with an odd height, fused 2x upsample, folded shortcut) on H != W
    images -- each geometry and its transpose -- at forced split counts from one to one K-step per split, in both
    split-K tile orders (knob 14: bit-identical, the order changes no sum); vs torch fp32. The reference with H and W
    exchanged is far outside the tolerance, so an H / W mix-up in the kernel's index math cannot pass."""
    Cin, Cin2, Cout, nimg, _, _, stride, up, _ = SHIFTED[fam]
    x, wc, b, kw, ref, ref_swapped = _conv_problem(Cin, Cin2, Cout, nimg, H, W, stride, up, full)
    ksplit = expected_splits((9 * Cin + Cin2) // 64, ks)
    act = kw.get("act", ops.ACT_NONE)
    outs = []
    for mfast in (1, 0):
        with tuned(ksplit=ks, mfast=mfast):
            outs.append(run_conv(nimg, H, W, Cin, Cout, ksplit,
                                 lambda: ops.conv3x3(x, nimg, H, W, wc, b, stride=stride, upsample=up, **kw),
                                 halo=False, Cin2=Cin2, stride=stride, upsample=up, residual="residual" in kw, act=act))
    close(outs[0], ref)
    assert torch.equal(outs[0], outs[1])
    assert rel_l2(ref_swapped, ref) > 0.3 and rel_l2(outs[0], ref_swapped) > 0.3


# ---- D. halo convs, non-square --------------------------------------------------------------------------------------

HALO_CIN, HALO_COUT, HALO_NIMG, HALO_CIN2 = 128, 320, 2, 128  # four 32-channel slices
HALO_KS = (0, 1, 3, 4)  # 0: the library's own split (>= 2 slices per split: 2)
# (W, H) -> {knob 16 setting: tile rows} wherever that setting takes a halo tile for the shape (plan_halo,
# csrc/gemm.hip); test_halo_knob16_table_is_complete checks that every setting left out plans shifted tiles
HALO_PLAIN = {(64, 2): {1: 128}, (64, 4): {1: 128, 2: 256, 3: 256}, (64, 6): {1: 128},
              (32, 4): {1: 128, 2: 128, 3: 128}, (32, 8): {1: 128, 2: 128, 3: 256}, (32, 12): {1: 128, 2: 128, 3: 128},
              (16, 8): {1: 128, 2: 128, 3: 128}, (16, 24): {1: 128, 2: 128, 3: 128}}
HALO_UP = {(32, 2): 256, (16, 4): 128, (8, 4): 128}  # input (W, H) -> tile rows; output widths 64, 32, 16
HALO_SC = {(64, 4): 128, (32, 12): 128}
HALO_GN = {(64, 4): 128, (64, 12): 128}


def _halo_splits(ks):
    return 2 if ks == 0 else expected_splits(HALO_CIN // 32, ks)


@functools.lru_cache(maxsize=None)
def _halo_problem(H, W, upsample, Cin2):
    """Operands, host fp32 reference and the shifted-tile output (knob 16 = 0, unsplit) of one halo geometry, with the
    time-embedding column add (per image) and, without a folded shortcut, the residual."""
    Cin, Cout, nimg = HALO_CIN, HALO_COUT, HALO_NIMG
    seed = 500 + 5 * H + W + Cin2
    OH, OW = (2 * H, 2 * W) if upsample else (H, W)
    x = rnd(nimg * H * W, Cin, seed=seed)
    w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=seed + 1), rnd(Cout, scale=0.1, seed=seed + 2)
    temb = rnd(nimg, Cout, seed=seed + 3)
    kw = dict(coladd=temb, coladd_bstride=Cout)
    ref = conv_ref(x.cpu(), nimg, H, W, w.cpu(), b.cpu(), 1, upsample).to(DEV) + temb.float().repeat_interleave(OH * OW, 0)
    wc = ops.conv_weight(w)
    if Cin2:
        x2, w2 = rnd(nimg * H * W, Cin2, seed=seed + 5), rnd(Cout, Cin2, scale=Cin2 ** -0.5, seed=seed + 6)
        wc = ops.conv_weight_with_shortcut(wc, w2)
        kw.update(shortcut=x2)
        ref = ref + x2.float() @ w2.float().t()
    else:
        r = rnd(nimg * OH * OW, Cout, seed=seed + 4)
        kw.update(residual=r)
        ref = ref + r.float()
    with tuned(halo=0, ksplit=1):
        shifted = run_conv(nimg, H, W, Cin, Cout, 1, lambda: ops.conv3x3(x, nimg, H, W, wc, b, upsample=upsample, **kw),
                           halo=False, Cin2=Cin2, upsample=upsample, residual=not Cin2)
    close(shifted, ref)
    return x, wc, b, kw, ref, shifted


def _run_halo(H, W, ks, rows, *, knob16=1, upsample=False, Cin2=0):
    x, wc, b, kw, ref, shifted = _halo_problem(H, W, upsample, Cin2)
    ksplit = _halo_splits(ks)
    outs = []
    for mfast in ((1, 0) if ksplit > 1 else (1,)):
        with tuned(ksplit=ks, halo=knob16, mfast=mfast):
            outs.append(run_conv(HALO_NIMG, H, W, HALO_CIN, HALO_COUT, ksplit,
                                 lambda: ops.conv3x3(x, HALO_NIMG, H, W, wc, b, upsample=upsample, **kw),
                                 halo=True, tile=(rows, 320), Cin2=Cin2, upsample=upsample, residual=not Cin2))
    close(outs[0], ref)
    close(outs[0], shifted.float())
    for o in outs[1:]:
        assert torch.equal(outs[0], o)


@pytest.mark.parametrize("ks", HALO_KS)
@pytest.mark.parametrize("W,H,knob16", [(W, H, k) for (W, H), ks_ in HALO_PLAIN.items() for k in sorted(ks_)])
def test_halo_conv_nonsquare(W, H, knob16, ks):
    """The 64-, 32- and 16-wide halo tiles on H != W images at whole-image fractions the square shapes never give (a
    single 128-row tile per image, 384-row images on 128-row tiles), under every knob 16 setting that takes a halo tile
    for the shape, unsplit and on 2 and 4 splits of the four 32-channel slices, with the time-embedding column add and
    residual; vs torch fp32 and vs the shifted-tile path; both tile orders of a split bit-identical."""
    _run_halo(H, W, ks, HALO_PLAIN[(W, H)][knob16], knob16=knob16)


def test_halo_knob16_table_is_complete():
    """HALO_PLAIN lists every (geometry, knob 16) pair that takes a halo tile: the pairs left out plan shifted tiles."""
    for (W, H), settings in HALO_PLAIN.items():
        for knob16 in (1, 2, 3):
            with tuned(halo=knob16):
                plan = ops.conv_plan(HALO_NIMG, H, W, HALO_CIN, HALO_COUT, residual=True)
            assert plan["halo"] == (knob16 in settings), (W, H, knob16, plan)
            if plan["halo"]:
                assert plan["tile"] == (settings[knob16], 320), (W, H, knob16, plan)


@pytest.mark.parametrize("ks", HALO_KS)
@pytest.mark.parametrize("W,H", sorted(HALO_UP))
def test_halo_upsample_conv_nonsquare(W, H, ks):
    """The three upsample halo tiles (output widths 64, 32, 16) on H != W inputs."""
    _run_halo(H, W, ks, HALO_UP[(W, H)], upsample=True)


@pytest.mark.parametrize("ks", HALO_KS)
@pytest.mark.parametrize("W,H", sorted(HALO_SC))
def test_halo_shortcut_conv_nonsquare(W, H, ks):
    """The folded 1x1 shortcut's K-steps behind the halo slices (4 steps of 32 channels, split with them) on H != W."""
    _run_halo(H, W, ks, HALO_SC[(W, H)], Cin2=HALO_CIN2)


@pytest.mark.parametrize("ks", HALO_KS)
@pytest.mark.parametrize("W,H", sorted(HALO_GN))
def test_halo_groupnorm_conv_nonsquare(W, H, ks):
    """sdmoe_conv3x3_gn on 64-wide non-square images: bit-identical to sdmoe_groupnorm_apply + the plain halo conv
    under the same split and tile order, and within the tolerance of torch fp32."""
    Cin, Cout, nimg = HALO_CIN, HALO_COUT, HALO_NIMG
    x = rnd(nimg * H * W, Cin, seed=600 + H) * 2 + 0.5
    gamma, beta = rnd(Cin, scale=0.1, seed=601) + 1, rnd(Cin, scale=0.1, seed=602)
    sc, sh = ops.groupnorm_stats(x, nimg, H * W, gamma, beta, 1e-5, 32)
    w, b = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=603), rnd(Cout, scale=0.1, seed=604)
    temb, r = rnd(nimg, Cout, seed=605), rnd(nimg * H * W, Cout, seed=606)
    wc, kw = ops.conv_weight(w), dict(coladd=temb, coladd_bstride=Cout, residual=r)
    assert ops.conv_gn_fusable(H, W, Cin, Cout)
    ksplit = _halo_splits(ks)
    tile = (HALO_GN[(W, H)], 320)
    for mfast in ((1, 0) if ksplit > 1 else (1,)):
        with tuned(ksplit=ks, mfast=mfast):
            fused = run_conv(nimg, H, W, Cin, Cout, ksplit,
                             lambda: ops.conv3x3(x, nimg, H, W, wc, b, gn=(sc, sh, True), **kw),
                             halo=True, tile=tile, residual=True, gn=True)
            xn = ops.groupnorm_apply(x, nimg, H * W, sc, sh, True)
            plain = run_conv(nimg, H, W, Cin, Cout, ksplit, lambda: ops.conv3x3(xn, nimg, H, W, wc, b, **kw),
                             halo=True, tile=tile, residual=True)
        assert torch.equal(fused, plain)
        if mfast:
            first = fused
        else:
            assert torch.equal(fused, first)
    xr = F.silu(F.group_norm(x.float().view(nimg, H * W, Cin).permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5))
    ref = conv_ref(xr.permute(0, 2, 1).reshape(-1, Cin).cpu(), nimg, H, W, w.cpu(), b.cpu()).to(DEV)
    close(first, ref + temb.float().repeat_interleave(H * W, 0) + r.float())
