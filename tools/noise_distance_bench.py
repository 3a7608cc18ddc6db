"""Times the noise-HPO objective two ways on the same device data, in one process, alternating round by round:

  device   ops.noise_distance on the two [T, nimg * HW, 4] fp16 device stores (3 launches) + the one device->host copy
           of its [T, G, 4] float64 result (sdmoe.discovery.noise_distances)
  host     the reference driver's route (modularity/remove_experts_noise_hpo.py:74-84): per step, both [nimg, 4, H, W]
           fp16 outputs copied to the host with .cpu() (2 T blocking copies), torch.norm of their difference, and the
           norm of the difference of their F.normalize(p = 1)'d flattenings, all on fp16 CPU tensors

Each timing is a host clock around work that ends synchronised (the .cpu() copies block; the device form ends in its
own copy). Warm-up rounds first; medians with min / max over the rounds. The result goes to stdout and, with --out, to
a file.

usage: python tools/noise_distance_bench.py [--T 51] [--nimg 16] [--HW 4096] [--rounds 9] [--out FILE]
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

from sdmoe import discovery, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=51)
    ap.add_argument("--nimg", type=int, default=16)
    ap.add_argument("--HW", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_distance_bench needs a GPU")
    T, nimg, HW = a.T, a.nimg, a.HW
    H = int(round(HW ** 0.5))
    B = max(1, nimg // 2)
    g = torch.Generator().manual_seed(0)
    base = torch.randn(T, nimg * HW, 4, generator=g).half().cuda()
    adj = (base.float() + 0.05 * torch.randn(T, nimg * HW, 4, generator=g).cuda()).half()
    table = torch.tensor([i % B for i in range(nimg)], dtype=torch.int32, device="cuda")
    # the layout the reference's hook sees: one [nimg, 4, H, W] tensor per step
    base_nchw = [base[t].view(nimg, H, HW // H, 4).permute(0, 3, 1, 2).contiguous() for t in range(T)]
    adj_nchw = [adj[t].view(nimg, H, HW // H, 4).permute(0, 3, 1, 2).contiguous() for t in range(T)]
    torch.cuda.synchronize()

    def device_route():
        return discovery.noise_distances(ops.noise_distance(base, adj, nimg, img_group=table, ngroups=B))

    def host_route():
        l2, l1n = [], []
        for t in range(T):
            u, v = base_nchw[t].cpu(), adj_nchw[t].cpu()
            l2.append(torch.norm(u - v).item())
            u1 = torch.nn.functional.normalize(u.view(-1), dim=0, p=1)
            u2 = torch.nn.functional.normalize(v.view(-1), dim=0, p=1)
            l1n.append(torch.norm(u1 - u2).item())
        return l2, l1n

    times = {"device": [], "host": []}
    for r in range(a.warmup + a.rounds):
        for name, fn in (("device", device_route), ("host", host_route)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[name].append(dt)
    # kernel time alone: device events around 20 back-to-back calls
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = torch.empty((T, B, 4), dtype=torch.float64, device="cuda")
    ws = torch.empty(4 * T * nimg * -(-HW // ops.NOISE_SLAB_ROWS), dtype=torch.float64, device="cuda")
    kern = []
    for r in range(a.rounds):
        ev0.record()
        for _ in range(20):
            ops.noise_distance(base, adj, nimg, img_group=table, ngroups=B, out=out, workspace=ws)
        ev1.record()
        torch.cuda.synchronize()
        kern.append(ev0.elapsed_time(ev1) / 20 * 1e3)
    nbytes = 2 * 2 * T * nimg * HW * 4 * 2  # two passes over two fp16 stores
    lines = [f"# noise objective, T={T} nimg={nimg} HW={HW} ({B} prompts), {torch.cuda.get_device_name(0)}, one process, "
             f"routes alternated, median of {a.rounds} rounds after {a.warmup} warm-up rounds"]
    for name, what in (("device", "sdmoe_noise_distance (3 launches, float64) + 1 copy of 4*T*B doubles"),
                       ("host", f"{2 * T} .cpu() copies + torch norms on fp16 CPU tensors (the reference's route)")):
        v = [x * 1e3 for x in times[name]]
        lines.append(f"{name:6s} {statistics.median(v):10.3f} ms (min {min(v):.3f}, max {max(v):.3f})   {what}")
    lines.append(f"host/device {statistics.median(times['host']) / statistics.median(times['device']):.1f}")
    lines.append(f"kernels only (device events, 20 back-to-back calls): {statistics.median(kern):.1f} us per call "
                 f"(min {min(kern):.1f}, max {max(kern):.1f}); {nbytes / 1e6:.1f} MB read per call from shapes = "
                 f"{nbytes / statistics.median(kern) / 1e6:.2f} TB/s (the stores fit the Infinity Cache)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
