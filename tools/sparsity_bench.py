"""Time sdmoe_geglu_sparsity (product + per-neuron zero / negative counts + totals in one streaming pass) against
sdmoe_geglu_neurons with colmax (product + per-neuron column maximum), the existing pass of the same shape: both read
2 F and write F halves per row plus negligible partials.

Same process, same inputs, the two kernels alternated round by round; device events around `iters` back-to-back calls
after a warm-up; the inputs rotate through enough distinct buffers (> 1 GiB) that no call finds its Y in the 256 MiB
Infinity Cache. Bytes are counted from the shape (6 M F); the HBM fraction is against the 8 TB/s peak. Prints one line
per activation with both medians and their ratio.

usage: python tools/sparsity_bench.py [--rounds 21] [--iters 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-models-moe_amd"))

import torch  # noqa: E402

from sdmoe import ops  # noqa: E402

M, F, NIMG = 65536, 1280, 16
HBM_PEAK = 8.0e12


def timed(fn, bufs, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(bufs[i % len(bufs)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparsity_bench needs a GPU: a CPU run measures nothing")
    dev = "cuda"
    rpi = M // NIMG
    lines = [f"# sdmoe_geglu_sparsity(col_zero, col_neg, totals) vs sdmoe_geglu_neurons(colmax), M={M} F={F} "
             f"{NIMG} images, {torch.cuda.get_device_name(0)}, median of {a.rounds} rounds x {a.iters} calls, "
             f"us per call"]
    nbuf = max(2, -(-(1 << 30) // (M * 2 * F * 2)))
    g = torch.Generator(device=dev).manual_seed(M + F)
    bufs = [(torch.randn((M, 2 * F), generator=g, device=dev) * 1.5).half() for _ in range(nbuf)]
    out = torch.empty((M, F), dtype=torch.float16, device=dev)
    colmax = torch.empty((1, F), dtype=torch.float16, device=dev)
    cz = torch.empty((1, F), dtype=torch.int32, device=dev)
    cn = torch.empty((1, F), dtype=torch.int32, device=dev)
    tt = torch.empty((1, 2), dtype=torch.int64, device=dev)
    for name in ("relu", "gelu"):
        act = ops.ACT_BY_NAME[name]

        def new(y):
            ops.geglu_sparsity(y, act, rows_per_img=rpi, col_zero=cz, col_neg=cn, totals=tt, out=out)

        def old(y):
            ops.geglu_neurons(y, act, rows_per_img=rpi, colmax=colmax, out=out)

        old(bufs[0])
        want = out.clone()
        new(bufs[0])
        assert torch.equal(out, want), "the two products disagree"
        for fn in (new, old):
            timed(fn, bufs, a.iters)  # warm-up
        tn, to = [], []
        for _ in range(a.rounds):
            tn.append(timed(new, bufs, a.iters))
            to.append(timed(old, bufs, a.iters))
        mn, mo = statistics.median(tn), statistics.median(to)
        byts = 6 * M * F
        lines.append(f"act={name:4s}  sparsity {mn:7.1f} us (min {min(tn):.1f}, max {max(tn):.1f}; "
                     f"{byts / mn / 1e6:.2f} TB/s, {byts / (mn * 1e-6) / HBM_PEAK:.0%} of peak)   "
                     f"neurons {mo:7.1f} us (min {min(to):.1f}, max {max(to):.1f}; {byts / mo / 1e6:.2f} TB/s, "
                     f"{byts / (mo * 1e-6) / HBM_PEAK:.0%} of peak)   sparsity/neurons {mn / mo:.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
