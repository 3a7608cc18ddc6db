"""Time sdmoe_geglu_neurons (product + per-neuron column maximum in one streaming pass) against the only way to get the
same numbers without it: sdmoe_geglu_route(E = 0, gate_out) followed by torch.amax over the stored gate.

Same process, same inputs, the two forms alternated round by round; device events around `iters` back-to-back calls
after a warm-up; the inputs rotate through enough distinct buffers (> 1 GiB) that no call finds its Y in the 256 MiB
Infinity Cache. Bytes are counted from the shapes: the new pass moves 6 M F (read Y, write out), the old route 10 M F
(read Y, write out and gate, read the gate again). Prints one line per shape and the ratio old / new of the medians.

usage: python tools/neuron_bench.py [--act gelu|relu] [--rounds 7] [--iters 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-models-moe_amd"))

import torch  # noqa: E402

from sdmoe import ops  # noqa: E402

SHAPES = [(8192, 1280), (65536, 1280), (4096, 5120)]


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
    ap.add_argument("--act", default="gelu", choices=["gelu", "relu"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neuron_bench needs a GPU: a CPU run measures nothing")
    act = ops.ACT_BY_NAME[a.act]
    dev = "cuda"
    lines = [f"# sdmoe_geglu_neurons(colmax) vs geglu_route(gate_out) + torch.amax, act={a.act}, "
             f"{torch.cuda.get_device_name(0)}, median of {a.rounds} rounds x {a.iters} calls, us per call"]
    for M, F in SHAPES:
        nbuf = max(2, -(-(1 << 30) // (M * 2 * F * 2)))
        g = torch.Generator(device=dev).manual_seed(M + F)
        bufs = [(torch.randn((M, 2 * F), generator=g, device=dev) * 1.5).half() for _ in range(nbuf)]
        out = torch.empty((M, F), dtype=torch.float16, device=dev)
        gate = torch.empty((M, F), dtype=torch.float16, device=dev)
        colmax = torch.empty((1, F), dtype=torch.float16, device=dev)

        def new(y):
            ops.geglu_neurons(y, act, colmax=colmax, out=out)

        def old(y):
            ops.geglu_route(y, None, act, out=out, gate_out=gate)
            torch.amax(gate, 0, out=colmax[0])

        old(bufs[0])
        want = colmax.clone()
        new(bufs[0])
        assert torch.equal(colmax, want), "the two forms disagree"
        for fn in (new, old):
            timed(fn, bufs, a.iters)  # warm-up
        tn, to = [], []
        for _ in range(a.rounds):
            tn.append(timed(new, bufs, a.iters))
            to.append(timed(old, bufs, a.iters))
        mn, mo = statistics.median(tn), statistics.median(to)
        lines.append(f"M={M:6d} F={F:5d}  new {mn:8.1f} us (min {min(tn):.1f}, max {max(tn):.1f}; "
                     f"{6 * M * F / mn / 1e6:.2f} TB/s of 6MF)   old {mo:8.1f} us (min {min(to):.1f}, max {max(to):.1f}; "
                     f"{10 * M * F / mo / 1e6:.2f} TB/s of 10MF)   old/new {mo / mn:.2f}")
        del bufs
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
