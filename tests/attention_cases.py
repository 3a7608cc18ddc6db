"""Inputs and references for the attention numerics tests (test_attention_cases.py on the CPU,
test_gpu_attention_numerics.py on the device). A plain module: no fixtures, nothing collected from it.

  exact(...)    softmax(q k^T scale) v per (image, head) in fp64: the reference every bar is taken against.
  emulate(...)  the same in fp64 arithmetic, rounded to fp16 where every attention kernel must round (the prescaled
                Q~, the probabilities P, the output). Its distance from exact() is what the number formats alone cost;
                the CPU test holds every case below to half the GPU bar by it, so the bar never comes from the
                kernels.
  rescale_rows(...)  which rows would move their running maximum at which 64-key tile under the kernels' deferred
                rule (threshold 8 log2 units): the CPU test uses it to show that a case drives the branch it is
                meant to drive.
  the case builders: each returns (q, k, v, nimg, Nq, Nk, heads), CPU fp16 tensors from a seeded generator,
                q [nimg*Nq, heads*d], k and v [nimg*Nk, heads*d].
"""
import math

import torch

LOG2E = 1.4426950408889634
KB = 64             # keys per tile, both kernels
RESCALE_THR = 8.0   # log2 units, both kernels
NIMG = 2

# what the GPU tests run: every forced variant at the three head dims with dedicated code paths (40: ones column in K
# and V, 64: plain, 80: ones column in V only), the shape-chosen kernel at the other two
VARIANTS = (0, 1, 2, 4, 8, 9)
DIMS_ALL_VARIANTS = (40, 64, 80)
DIMS_DEFAULT_ONLY = (32, 160)
ALL_DIMS = DIMS_ALL_VARIANTS + DIMS_DEFAULT_ONLY


def _split(x, nimg, N, heads):
    d = x.shape[1] // heads
    return x.reshape(nimg, N, heads, d).permute(0, 2, 1, 3)


def _merge(o):
    nimg, heads, N, d = o.shape
    return o.permute(0, 2, 1, 3).reshape(nimg * N, heads * d)


def exact(q, k, v, nimg, Nq, Nk, heads, scale=None):
    """fp64 softmax(q k^T scale) v, [nimg*Nq, heads*d] on the inputs' device."""
    d = q.shape[1] // heads
    scale = d ** -0.5 if scale is None else scale
    qh, kh, vh = (_split(t.double(), nimg, n, heads) for t, n in ((q, Nq), (k, Nk), (v, Nk)))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return _merge(p @ vh)


def _prescaled_q(q, heads, scale):
    d = q.shape[1] // heads
    scale = d ** -0.5 if scale is None else scale
    # the kernels' factor is the fp32 product scale * log2(e); Q~ = fp16(fp32(q) * factor)
    factor = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    return (q.float() * factor).half()


def emulate(q, k, v, nimg, Nq, Nk, heads, scale=None):
    """Format-faithful restatement, fp64 arithmetic between the roundings: Q~ = fp16(fp32(q) scale log2 e),
    s = Q~ k, P = fp16(exp2(s - rowmax)), l = sum of the rounded P, out = fp16(P v / l). Returns fp16."""
    qh = _split(_prescaled_q(q, heads, scale).double(), nimg, Nq, heads)
    kh, vh = _split(k.double(), nimg, Nk, heads), _split(v.double(), nimg, Nk, heads)
    s = qh @ kh.transpose(-1, -2)
    p = torch.exp2(s - s.amax(dim=-1, keepdim=True)).half().double()
    return _merge((p @ vh) / p.sum(dim=-1, keepdim=True)).half()


def errors(out, ref):
    """(relative L2, max |err| / max(1, max |ref|)): the two figures close() bounds by 2e-3 and 1e-2."""
    out, ref = out.double(), ref.double()
    diff = out - ref
    return (diff.norm() / ref.norm()).item(), diff.abs().max().item() / max(1.0, ref.abs().max().item())


def rescale_rows(q, k, nimg, Nq, Nk, heads, scale=None, group=16):
    """(own, fired), bool [nimg, heads, Nq, tiles]. own: row r's own shifted tile maximum exceeds RESCALE_THR at tile
    t >= 1; fired: some row of r's `group` of consecutive queries (one wave's share) does, so r runs the rescale.
    The running maximum m follows the kernels' rule: m = max of tile 0, then m += max(tile max - m, 0) for every row
    of a group that fires."""
    qh = _split(_prescaled_q(q, heads, scale).double(), nimg, Nq, heads)
    s = qh @ _split(k.double(), nimg, Nk, heads).transpose(-1, -2)
    nt = (Nk + KB - 1) // KB
    tmax = torch.stack([s[..., t * KB:(t + 1) * KB].amax(dim=-1) for t in range(nt)], dim=-1)  # [.., Nq, nt]
    pad = (-Nq) % group
    m = tmax[..., 0].clone()
    own = torch.zeros_like(tmax, dtype=torch.bool)
    fired = torch.zeros_like(own)
    for t in range(1, nt):
        x = tmax[..., t] - m
        own[..., t] = x > RESCALE_THR
        per_group = torch.nn.functional.pad(own[..., t], (0, pad)).reshape(*x.shape[:-1], -1, group).any(-1)
        fire = per_group.repeat_interleave(group, dim=-1)[..., :Nq]
        fired[..., t] = fire
        m = torch.where(fire, m + x.clamp(min=0), m)
    return own, fired


# ---------------------------------------------------------------------------------------------------------------
# case builders

def _gen(*key):
    seed = 0
    for x in key:
        seed = (seed * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(seed)


def _values(g, rows, heads, d):
    """V with a per-column offset of +-2: an error in a row sum then scales the whole output row instead of
    averaging out over zero-mean values."""
    C = heads * d
    off = 2.0 * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    return torch.randn(rows, C, generator=g) + off


def logit_scale(d, sigma, Nq, Nk, heads=3):
    """q, k ~ N(0, 1) sqrt(sigma): logits q k^T / sqrt(d) of standard deviation sigma.

    sigma = 12 with Nk = 200 is the family's hardest case for the formats alone (the Q~ rounding of 2^-11 on logits
    near 50 moves the weights of the few keys that compete for a row by percents). It is kept at 12, on the seed
    _gen() derives from the arguments, not on a picked one: with V offset by +-2 the output peaks near 6 and the
    emulation's scaled max error is 1.3e-3 to 1.7e-3 on these seeds, and stayed <= 3.2e-3 (limit 5e-3; relative L2
    <= 3.6e-4, limit 1e-3) on eight other seeds at each of the five head dims."""
    g = _gen(1, d, int(sigma * 10), Nq, Nk)
    C = heads * d
    q = torch.randn(NIMG * Nq, C, generator=g) * math.sqrt(sigma)
    k = torch.randn(NIMG * Nk, C, generator=g) * math.sqrt(sigma)
    v = _values(g, NIMG * Nk, heads, d)
    return q.half(), k.half(), v.half(), NIMG, Nq, Nk, heads


def _direction(g, heads, d):
    """one unit vector per head, +-1/sqrt(d) entries"""
    return ((torch.randint(0, 2, (heads * d,), generator=g) * 2 - 1).float() / math.sqrt(d))


def _noise_orth(g, rows, heads, d, u):
    """N(0,1) noise with its component along each head's u removed"""
    n = torch.randn(rows, heads, d, generator=g)
    uh = u.reshape(heads, d)
    n = n - (n * uh).sum(-1, keepdim=True) * uh
    return n.reshape(rows, heads * d)


RAMP_NK = 520
QUIET_ALONG_U = -1.0  # the quiet rows of mixed(): their logits fall by 1.5 log2 units per tile, maximum in tile 0


def _ramp(d, slope, Nq, Nk, heads, aligned, tag):
    g = _gen(2, d, int(slope * 10) + 1000, Nq, Nk, tag)
    u = _direction(g, heads, d)
    # log2-unit logit of an aligned query (6 u) on key j: 6 a_j scale log2(e) = slope j / 64
    a = slope * torch.arange(Nk, dtype=torch.float32) / (KB * 6.0 * d ** -0.5 * LOG2E)
    k = a.repeat(NIMG)[:, None] * u + 0.3 * torch.randn(NIMG * Nk, heads * d, generator=g)
    along = torch.where(aligned.repeat(NIMG), 6.0, QUIET_ALONG_U)[:, None]
    q = along * u + 0.3 * _noise_orth(g, NIMG * Nq, heads, d, u)
    # the aligned rows keep a small spread of slopes (1.7 % rms: at +9 a row then still clears the threshold of 8)
    q = q + (aligned.repeat(NIMG)[:, None] * 0.1 * torch.randn(NIMG * Nq, 1, generator=g)) * u
    v = _values(g, NIMG * Nk, heads, d)
    return q.half(), k.half(), v.half(), NIMG, Nq, Nk, heads


def ramps(d, slope, Nq=192, Nk=RAMP_NK, heads=2):
    """Keys a_j u + 0.3 noise, queries 6 u + 0.3 noise: the log2-unit logit moves by `slope` per 64-key tile.
    +5: the excess over the running maximum builds up under the threshold and trips the rescale every second tile;
    +9: every tile; -9: the maximum sits in tile 0 and the later tiles underflow. |k| stays below 20."""
    return _ramp(d, slope, Nq, Nk, heads, torch.ones(Nq, dtype=torch.bool), 0)


def mixed(d, reverse, Nq=192, Nk=RAMP_NK, heads=2):
    """The +9 ramp with only every 16th query aligned with u (one triggering row per 16-query MFMA fragment; the
    others lean against u, keep their maximum in tile 0 and must come through a rescale they did not ask for with
    alpha = 1). reverse: every row but each 16th aligned."""
    sel = (torch.arange(Nq) % 16) == 5
    return _ramp(d, 9.0, Nq, Nk, heads, ~sel if reverse else sel, 1 + int(reverse))


STAIR_NK = 400
STAIR_STEP = 12.0  # log2 units per pair of tiles: clears the threshold of 8 with margin for the 0.3 noise


def staircase(d, Nq=192, Nk=STAIR_NK, heads=2):
    """The running maximum moves, then the NEXT tile sits at the same level: tiles 0-1, 2-3 and 4-6 (the last one
    ragged, 16 keys) at log2-unit logits 0, 12 and 24 for every query. Tile 4 moves m and is weighed with the new
    shift as computed in that tile; tiles 5 and 6 are weighed with the shift as it was stored (at d = 40 the
    32x32x16 kernel stores -m as an fp16 element of Q~). The three share the softmax about 4 : 4 : 1 and V carries an
    offset of +-2 whose sign alternates from tile to tile, so a shift that differs between them by half an fp16 ulp
    of m (2^-7 at m = 24: 0.5 % in weight) moves the output by several times the bar, where in the ramps the last
    tile outweighs the one before it 32 to 1 and hides it."""
    g = _gen(6, d, Nq, Nk)
    u = _direction(g, heads, d)
    j = torch.arange(Nk)
    level = STAIR_STEP * torch.clamp(j // (2 * KB), max=2).float()
    a = level / (6.0 * d ** -0.5 * LOG2E)
    k = a.repeat(NIMG)[:, None] * u + 0.3 * torch.randn(NIMG * Nk, heads * d, generator=g)
    q = 6.0 * u + 0.3 * _noise_orth(g, NIMG * Nq, heads, d, u)
    col = (torch.randint(0, 2, (heads * d,), generator=g) * 2 - 1).float()
    tile_sign = (1 - 2 * ((j // KB) % 2)).float().repeat(NIMG)
    v = torch.randn(NIMG * Nk, heads * d, generator=g) + 2.0 * tile_sign[:, None] * col
    return q.half(), k.half(), v.half(), NIMG, Nq, Nk, heads


def last_key_spike(d, Nk, at_tile_start, Nq=130, heads=4):
    """N(0,1) inputs with k[key] = 4 q[query] on one head for every 7th query (a different head each, per image), as
    test_attention_peaked_softmax plants its spike; key = Nk - 1, the last valid key beside the first masked one, or
    the first key of the ragged tile."""
    g = _gen(3, d, Nk, int(at_tile_start), Nq)
    C = heads * d
    q = torch.randn(NIMG * Nq, C, generator=g)
    k = torch.randn(NIMG * Nk, C, generator=g)
    v = _values(g, NIMG * Nk, heads, d)
    key = KB * ((Nk - 1) // KB) if at_tile_start else Nk - 1
    for b in range(NIMG):
        for h in range(heads):
            query = 7 * (b * heads + h + 1)
            k[b * Nk + key, h * d:(h + 1) * d] = 4 * q[b * Nq + query, h * d:(h + 1) * d]
    return q.half(), k.half(), v.half(), NIMG, Nq, Nk, heads


def spiked_rows(Nq=130, heads=4):
    """(image, head, query) of the rows last_key_spike() spikes"""
    return [(b, h, 7 * (b * heads + h + 1)) for b in range(NIMG) for h in range(heads)]


def key_offset(d, Nq, Nk, heads=3):
    """logit_scale at sigma = 4 with a constant vector c, |c_i| = 8, added to every key: the same softmax, but every
    logit of a row moves by q c / sqrt(d) (std 16), so the running maximum m is +-23 log2 units on a typical row and up to +-120 on the
    most extreme ones (logits of +-80) while the logit differences stay those of sigma = 4."""
    q, k, v, nimg, Nq, Nk, heads = logit_scale(d, 4.0, Nq, Nk, heads)
    g = _gen(4, d, Nq, Nk)
    c = 8.0 * (torch.randint(0, 2, (heads * d,), generator=g) * 2 - 1)
    return q, (k.float() + c).half(), v, nimg, Nq, Nk, heads


def guarded(d, Nq, heads=3):
    """self-attention inputs for the guarded-output test (logit std 4, ragged Nq = Nk)"""
    g = _gen(5, d, Nq)
    C = heads * d
    q = torch.randn(NIMG * Nq, C, generator=g) * 2.0
    k = torch.randn(NIMG * Nq, C, generator=g) * 2.0
    v = _values(g, NIMG * Nq, heads, d)
    return q.half(), k.half(), v.half(), NIMG, Nq, Nq, heads


# ---------------------------------------------------------------------------------------------------------------
# the case list both test files walk: (family, id, builder, args). d is the first argument of every builder.

SWEEP_SHAPES = ((200, 200), (130, 77))
SPIKE_NK = (77, 129, 50)
GUARD_NQ = (130, 300)
GUARD_DIMS = (40, 80)


def families():
    """{family: [(id, builder, args-after-d)]}"""
    spikes = []
    for Nk in SPIKE_NK:
        for start in (False, True):
            if start and KB * ((Nk - 1) // KB) == Nk - 1:
                continue  # Nk = 129: key 128 is both
            spikes.append((f"Nk{Nk}-{'tilestart' if start else 'last'}", last_key_spike, (Nk, start)))
    return {
        "logit_scale": [(f"std{s}-{Nq}x{Nk}", logit_scale, (float(s), Nq, Nk))
                        for s in (4, 12) for Nq, Nk in SWEEP_SHAPES],
        "ramps": [(f"slope{s:+d}", ramps, (float(s),)) for s in (5, 9, -9)],
        "staircase": [("step12", staircase, ())],
        "mixed": [("one-in-16", mixed, (False,)), ("all-but-one-in-16", mixed, (True,))],
        "last_key_spike": spikes,
        "key_offset": [(f"{Nq}x{Nk}", key_offset, (Nq, Nk)) for Nq, Nk in SWEEP_SHAPES],
    }


def cases(dims=ALL_DIMS):
    """[(family, id, d, builder, args)] for every family but guarded (its dims and shapes are its own)"""
    out = [(fam, cid, d, fn, args) for fam, lst in families().items() for cid, fn, args in lst for d in dims]
    return out


def guarded_cases():
    return [("guarded", f"Nq{Nq}", d, guarded, (Nq,)) for Nq in GUARD_NQ for d in GUARD_DIMS]
