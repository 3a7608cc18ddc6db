"""Time a pipeline call under the two expert-level discovery receivers against the receiver each one extends:
FrequencyMeasure against MOEFy (the same routed output, plus the per-expert selection counts) and ExpertPredictivity
against GetExperts (the same dense output and scores, a column maximum instead of a mean + top-k).

One process, one pipeline: the benchmark's SD-1.4 shape (UNetConfig.sd14(64), synthetic weights, E = 4C / 20 experts,
k = int(E * topk), one prompt under guidance), `--inference-steps` denoising steps per call. After a warm-up call of
each receiver the four are alternated round by round; a call is timed on the host between two device synchronisations,
so it includes the one device->host copy each discovery receiver makes when observe_activation returns. Prints the
median, minimum and maximum per receiver and the two ratios of the medians.

usage: python tools/expert_discovery_bench.py [--inference-steps 10] [--rounds 7] [--topk 0.2] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-models-moe_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inference-steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--topk", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expert_discovery_bench needs a GPU: a CPU run measures nothing")
    from moefication.helper import moefy_synthetic
    from neuron_receivers import ExpertPredictivity, FrequencyMeasure, GetExperts, MOEFy
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    dev = "cuda:0"
    T = a.inference_steps
    pipe = StableDiffusionPipeline.synthetic(UNetConfig.sd14(64), seed=0, device=dev, num_inference_steps=T)
    _, names, nexp = moefy_synthetic(pipe, a.topk, 20, seed=0)
    L = len(names)
    recs = {
        "MOEFy": MOEFy(seed=0, store_gates=False),
        "FrequencyMeasure": FrequencyMeasure(0, T, L, nexp, names),
        "GetExperts": GetExperts(0, T, L, nexp, names, store_gates=False),
        "ExpertPredictivity": ExpertPredictivity(0, T, L, store_gates=False),
    }
    prompt = "a photo of an astronaut riding a horse"

    def call(rec):
        if hasattr(rec, "reset"):
            rec.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec.observe_activation(pipe, prompt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for rec in recs.values():
        call(rec)  # warm-up: weight layouts, the GELU table, allocator pools
    times = {n: [] for n in recs}
    for _ in range(a.rounds):
        for n, rec in recs.items():
            times[n].append(call(rec))
    med = {n: statistics.median(v) for n, v in times.items()}
    lines = [f"# one pipeline call of {T} steps, SD-1.4 64x64 latents, topk {a.topk}, {torch.cuda.get_device_name(0)}, "
             f"median of {a.rounds} alternated rounds after one warm-up call each, ms per call"]
    for n, v in times.items():
        lines.append(f"{n:20s} {med[n]:8.2f} ms  (min {min(v):.2f}, max {max(v):.2f})")
    lines.append(f"FrequencyMeasure / MOEFy        {med['FrequencyMeasure'] / med['MOEFy']:.3f}")
    lines.append(f"ExpertPredictivity / GetExperts {med['ExpertPredictivity'] / med['GetExperts']:.3f}")
    fm = recs["FrequencyMeasure"]
    k = [int(m.k) for n_, m in pipe.unet.named_modules() if n_.endswith("ff.net.0")]
    worst = max(abs(fm.label_counter[t][l].sum() - k[l]) for t in range(T) for l in range(L))
    lines.append(f"# check: every FrequencyMeasure row sums to its layer's k (largest deviation {worst:.1e})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
