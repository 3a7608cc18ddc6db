"""A/B of per-prompt concept sets (sdmoe_linear_masked_sets, WandaRemovePerPrompt) on one box, in one session.

usage: python tools/per_prompt_ab.py kernel [--prev LIB] [--iters 50]
       python tools/per_prompt_ab.py pipeline [--steps 50] [--size 64] [--prompts 8] [--moe]

kernel: sdmoe_linear_masked_sets (uniform table, and a mixed table over 4 sets) against the PREVIOUS build's
  sdmoe_linear_masked with one mask (--prev, default sdmoe/libsdmoe_hip_prev.so: tools/build_prev.sh), at the four FFN
  down projections of SD-1.4 at 8 prompts (16 images), with bias + residual, without and with the top-k keep bits. The
  previous kernel is timed twice, first and last: their difference is the A/A spread the comparison allows. Launches
  back to back between two HIP events (warm L2: a relative tool, as tools/micro_ab.py).
pipeline: images/s of three paths over the same prompts and sets (SD-1.4 widths, synthetic weights, 3 concepts, the
  prompts spread over 4 distinct sets: {}, {c0}, {c1, c2}, {c0, c1, c2}):
    batched   one WandaRemovePerPrompt call (MultiConceptRemoverWanda.remove_concepts_batch);
    loop      one prompt per call, the removal run of remove_concepts only: removers[c] for one concept, for more the
              union rebuilt on the host (reset_union_remover + handle_multiple_concepts) and the union remover's run;
    ceiling   ONE union of all concepts for every prompt, batched, on the existing in-GEMM path (bake_budget_bytes = 0).
  Each path is run once to warm its caches (device masks, baked weights), then timed.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "diffusion-models-moe_amd"), ROOT]

import torch  # noqa: E402

from sdmoe import _lib, ops  # noqa: E402

DEV = "cuda"
N_IMG = 16
SHAPES = [(4096, 320, 1280), (1024, 640, 2560), (256, 1280, 5120), (64, 1280, 5120)]  # rows per image, N, K


def timed(f, iters):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def kernel(a):
    prev = ctypes.CDLL(a.prev)
    prev.sdmoe_linear_masked.argtypes = _lib.SIGNATURES["sdmoe_linear_masked"]
    prev.sdmoe_linear_masked.restype = ctypes.c_int
    prev.sdmoe_version.restype = ctypes.c_char_p
    lib = _lib.load()
    print(f"previous build: {a.prev} ({prev.sdmoe_version().decode()}); this build: {lib.sdmoe_version().decode()}")
    print(f"{'shape':34s} {'prev':>9s} {'prev again':>11s} {'sets unif.':>11s} {'sets mixed':>11s}   plan (sets)")
    g = torch.Generator(device=DEV).manual_seed(0)
    for rpi, N, K in SHAPES:
        M = rpi * N_IMG
        x = torch.randn(M, K, generator=g, device=DEV).half()
        w = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).half()
        b = (torch.randn(N, generator=g, device=DEV) * 0.1).half()
        r = torch.randn(M, N, generator=g, device=DEV).half()
        y = torch.empty(M, N, dtype=torch.float16, device=DEV)
        wmasks = torch.stack([ops.wmask_kmajor((torch.rand(N, K // 8, generator=g, device=DEV) * 256).to(torch.uint8)
                                               & (torch.rand(N, K // 8, generator=g, device=DEV) * 256).to(torch.uint8)
                                               & (torch.rand(N, K // 8, generator=g, device=DEV) * 256).to(torch.uint8))
                              for _ in range(4)])  # density 1/8 each
        keep_bits = torch.randint(-2 ** 62, 2 ** 62, (K // 64, M), generator=g, dtype=torch.int64, device=DEV)
        ws = ops._workspace(x.device)
        uniform = torch.zeros(N_IMG, dtype=torch.int32, device=DEV)
        mixed = torch.tensor([i % 4 for i in range(N_IMG // 2)] * 2, dtype=torch.int32, device=DEV)
        for keep in (None, keep_bits):
            def old():
                st = prev.sdmoe_linear_masked(x.data_ptr(), x.stride(0), ops._ptr(keep), w.data_ptr(), w.stride(0),
                                              wmasks[0].data_ptr(), b.data_ptr(), r.data_ptr(), r.stride(0),
                                              y.data_ptr(), y.stride(0), M, N, K, ws.data_ptr(), ws.numel(),
                                              ops._stream())
                _lib.check(st, "previous sdmoe_linear_masked")

            def new(table):  # (the raw entry point, as for the previous build: no wrapper time in either column)
                def f():
                    st = lib.sdmoe_linear_masked_sets(x.data_ptr(), x.stride(0), ops._ptr(keep), w.data_ptr(),
                                                      w.stride(0), wmasks.data_ptr(), wmasks.stride(0),
                                                      table.data_ptr(), wmasks.shape[0], rpi, b.data_ptr(),
                                                      r.data_ptr(), r.stride(0), y.data_ptr(), y.stride(0), M, N, K,
                                                      ws.data_ptr(), ws.numel(), ops._stream())
                    _lib.check(st, "sdmoe_linear_masked_sets")
                return f
            t_old = timed(old, a.iters)
            t_uni = timed(new(uniform), a.iters)
            t_mix = timed(new(mixed), a.iters)
            t_old2 = timed(old, a.iters)
            plan = ops.gemm_plan_sets(M, N, K, rpi, keep=keep is not None, residual=True)
            name = f"M={M} N={N} K={K}{' +keep' if keep is not None else ''}"
            print(f"{name:34s} {t_old:7.2f}us {t_old2:9.2f}us {t_uni:9.2f}us {t_mix:9.2f}us   "
                  f"{plan['tile'][0]}x{plan['tile'][1]} split {plan['ksplit']}", flush=True)


def pipeline(a):
    from neuron_receivers import MultiConceptRemoverWanda, WandaRemoveNeuronsFast
    from sdmoe.config import UNetConfig
    from sdmoe.pipeline import StableDiffusionPipeline
    cfg = UNetConfig.sd14(a.size)
    pipe = StableDiffusionPipeline.synthetic(cfg, seed=0, device=DEV, num_inference_steps=a.steps)
    if a.moe:
        from moefication.helper import moefy_synthetic
        from sparsity.relufy_model import find_and_change_geglu
        find_and_change_geglu(pipe.unet)
        moefy_synthetic(pipe, 0.2, 20, seed=0)
    downs = [m for n, m in pipe.unet.named_modules() if n.endswith("ff.net.2")]
    T, L = a.steps, len(downs)
    concepts = ["c0", "c1", "c2"]
    g = torch.Generator(device=DEV).manual_seed(1)
    removers = {}
    for c in concepts:  # one random mask per layer (density 1/32), shared by every timestep: the timings do not read it
        per_layer = []
        for d in downs:
            N, K = d.weight.shape
            byts = torch.full((N, K // 8), 255, dtype=torch.uint8, device=DEV)
            for _ in range(5):
                byts &= (torch.rand(N, K // 8, generator=g, device=DEV) * 256).to(torch.uint8)
            per_layer.append(byts.cpu().numpy())
        removers[c] = WandaRemoveNeuronsFast.from_packed(0, {t: {l: per_layer[l] for l in range(L)} for t in range(T)},
                                                         T, L, store_gates=False)
    mc = MultiConceptRemoverWanda(None, 0, T, L, concepts_to_remove=concepts, removers=removers)
    distinct = [[], ["c0"], ["c1", "c2"], ["c0", "c1", "c2"]]
    sets = [distinct[i % 4] for i in range(a.prompts)]
    prompts = [f"prompt number {i}" for i in range(a.prompts)]

    def batched():
        return mc.remove_concepts_batch(pipe, prompts, sets)

    def loop():
        out = []
        for i, (p, cs) in enumerate(zip(prompts, sets)):
            pipe.prompt_offset = i
            if not cs:
                torch.manual_seed(0)
                out.append(pipe(p).images[0])
            elif len(cs) == 1:
                removers[cs[0]].reset_time_layer()
                out.append(removers[cs[0]].observe_activation(pipe, p)[0])
            else:
                mc.reset_union_remover()
                mc.handle_multiple_concepts(cs)
                mc.union_neuron_remover.reset_time_layer()
                out.append(mc.union_neuron_remover.observe_activation(pipe, p)[0])
        pipe.prompt_offset = 0
        return out

    def ceiling():
        u = mc.union_neuron_remover
        u.reset_time_layer()
        return u.observe_activation(pipe, prompts)[0]

    def rate(f, reps):
        f()  # warm: device masks, stacks, baked weights
        torch.cuda.synchronize()
        best = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            best.append(a.prompts / (time.perf_counter() - t0))
        return best

    print(f"SD-1.4 widths, {8 * a.size}^2, {a.steps} DDIM steps, {a.prompts} prompts, 4 distinct sets over 3 concepts"
          f"{', MoE-routed (relu, top-k 0.2, experts of 20)' if a.moe else ''}", flush=True)
    for name, f in (("batched per-prompt call", batched), ("one-prompt loop", loop)):
        r = rate(f, a.reps)
        print(f"{name:44s} " + " / ".join(f"{v:6.2f}" for v in r) + " images/s", flush=True)
    # the ceiling: one union of everything, in the GEMM (set up outside the timed region)
    mc.reset_union_remover()
    mc.handle_multiple_concepts(concepts)
    mc.union_neuron_remover.bake_budget_bytes = 0
    r = rate(ceiling, a.reps)
    print(f"{'uniform union, batched, in-GEMM (ceiling)':44s} " + " / ".join(f"{v:6.2f}" for v in r) + " images/s",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "pipeline"])
    ap.add_argument("--prev", default=os.path.join(ROOT, "diffusion-models-moe_amd", "sdmoe", "libsdmoe_hip_prev.so"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--size", type=int, default=64, help="latent side (64 = 512^2 images)")
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--moe", action="store_true", help="MoE-route the FFNs as bench.py does")
    a = ap.parse_args()
    (kernel if a.what == "kernel" else pipeline)(a)


if __name__ == "__main__":
    main()
