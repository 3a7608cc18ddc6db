"""Times the denoising loop's scheduler-step kernels against each other on the same device buffers, in one process,
interleaved round by round, at B = 8 with CFG and 64x64 and 128x128 latents:

  x0 first      ops.cfg_x0_step, flags (0, 0): an Euler step (no prev_x0 traffic)
  x0 second     ops.cfg_x0_step, flags (1, 1): a DPM-Solver++ 2M second-order step (reads and writes prev_x0)
  ddim          ops.cfg_ddim_step
  plms          ops.cfg_multistep_step, a steady-state PLMS call (the fourth-order combination: three history slots read,
                one stored)
  prep scaled   ops.prepare_input_scaled, two CFG copies
  prep          ops.prepare_input, two CFG copies

Each figure is device events around `--launches` back-to-back launches of one kernel, divided by the count; a round
times every kernel once, in turn; the medians, minima and maxima over the rounds after warm-up rounds are reported, with
the spread (max - min) / median of each kernel. Bytes per call are counted from the shapes. "host enqueue" is the host
clock around the same loop before the synchronise: where it equals the device figure, the window measured how fast the
Python binding issues launches, not the kernel. The result goes to stdout
and, with --out, to a file.

usage: python tools/sigma_step_bench.py [--B 8] [--rounds 15] [--launches 200] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "diffusion-models-moe_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from sdmoe import ops  # noqa: E402
from sdmoe.pipeline import ddim_schedule, dpmpp_2m_schedule, euler_schedule, pndm_schedule  # noqa: E402
from sdmoe.unet import IN_PAD, OUT_PAD  # noqa: E402


def cases(B, H, g=7.5):
    """(reset, [(name, bytes per call, fn)]) on buffers shaped as the pipeline's (padded U-Net input and output rows);
    reset() restores the latents, which every timed window of repeated steps moves away from N(0, 1)."""
    HW = H * H
    gen = torch.Generator().manual_seed(0)
    lat0 = torch.randn(B, 4, H, H, generator=gen).cuda()
    lat = lat0.clone()
    prev = torch.randn(B, 4, H, H, generator=gen).cuda()
    hist = torch.randn(4, B, 4, H, H, generator=gen).cuda()
    cur = torch.randn(B, 4, H, H, generator=gen).cuda()
    eps = torch.randn(2 * B * HW, OUT_PAD, generator=gen).half().cuda()
    x_in = torch.zeros((2 * B * HW, IN_PAD), dtype=torch.float16, device="cuda")
    e_coef = euler_schedule(50, "leading").plan[25][1]
    d_coef = dpmpp_2m_schedule(50, "v_prediction").plan[25][1]
    _, a_t, a_prev = ddim_schedule(50)
    _, p_coef, p_flags = pndm_schedule(50)[10]
    assert sum(c != 0 for c in p_coef[1:5]) == 3 and p_flags[0] >= 0
    n = B * 4 * HW
    eps_b, nx_b = 2 * n * 2, 2 * n * 2  # both CFG copies, fp16, channels 0..3
    return (lambda: lat.copy_(lat0)), [
        ("x0 first", eps_b + 2 * n * 4 + nx_b,
         lambda: ops.cfg_x0_step(eps, lat, True, g, None, e_coef, (0, 0), next_in=x_in)),
        ("x0 second", eps_b + 4 * n * 4 + nx_b,
         lambda: ops.cfg_x0_step(eps, lat, True, g, prev, d_coef, (1, 1), next_in=x_in)),
        ("ddim", eps_b + 2 * n * 4 + nx_b,
         lambda: ops.cfg_ddim_step(eps, lat, True, g, a_t[25], a_prev[25], next_in=x_in)),
        ("plms", eps_b + 6 * n * 4 + nx_b,
         lambda: ops.cfg_multistep_step(eps, lat, True, g, hist, cur, p_coef, p_flags, next_in=x_in)),
        ("prep scaled", 2 * n * 4 + nx_b, lambda: ops.prepare_input_scaled(lat, x_in, 2, 1.0, 0.25)),
        ("prep", n * 4 + nx_b, lambda: ops.prepare_input(lat, x_in, 2)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sigma_step_bench needs a GPU")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = [f"# scheduler-step kernels, B={a.B} with CFG, {torch.cuda.get_device_name(0)}, one process, kernels "
             f"interleaved round by round; device events around {a.launches} back-to-back launches; median of "
             f"{a.rounds} rounds after {a.warmup} warm-up rounds; us per call"]
    for H in (64, 128):
        reset, cs = cases(a.B, H)
        times = {name: [] for name, _, _ in cs}
        host = {name: [] for name, _, _ in cs}
        for r in range(a.warmup + a.rounds):
            for name, _, fn in cs:
                reset()
                torch.cuda.synchronize()
                ev0.record()
                t0 = time.perf_counter()
                for _ in range(a.launches):
                    fn()
                t1 = time.perf_counter()
                ev1.record()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[name].append(ev0.elapsed_time(ev1) / a.launches * 1e3)
                    host[name].append((t1 - t0) / a.launches * 1e6)
        lines.append(f"latents {H}x{H}")
        med = {}
        for name, nbytes, _ in cs:
            v = times[name]
            med[name] = m = statistics.median(v)
            lines.append(f"  {name:12s} {m:8.2f} us (min {min(v):.2f}, max {max(v):.2f}, spread "
                         f"{(max(v) - min(v)) / m * 100:.1f} %)   {nbytes / 1e6:7.2f} MB per call from shapes = "
                         f"{nbytes / m / 1e6:.2f} TB/s; host enqueue {statistics.median(host[name]):.2f} us")
        spread = max(max(times[k]) - min(times[k]) for k in ("x0 second", "plms"))
        lines.append(f"  x0 second - plms = {med['x0 second'] - med['plms']:+.2f} us (run-to-run spread of the two: "
                     f"{spread:.2f} us); x0 first - ddim = {med['x0 first'] - med['ddim']:+.2f} us; prep scaled - prep "
                     f"= {med['prep scaled'] - med['prep']:+.2f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
