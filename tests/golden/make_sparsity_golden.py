"""Golden vectors for the gate-sparsity measurement, made by running the REFERENCE's own receiver and statistics class.

Runs only in the build container (the reference tree is not present on the GPU box). Through make_golden's stub of
the absent `diffusers` package it imports, from the reference tree,
  * SparsityMeasure.hook_fn   neuron_receivers/sparsity_measure.py:13-18 (the activated gate of every hooked call,
                              copied to the host)
  * utils.StatMeter           utils.py:276-317, driven as sparsity/check_sparsity.py:31-50 drives it: per prompt, hooked
                              call i updates cell (i // num_geglu, i % num_geglu) with the mean over tokens of
                              (exact zeros in the row / F), then StatMeter.save -> sparsity.json
and runs them on the CPU in fp16 on seeded inputs ([2, N, C] tokens, C = 320, N = 32, 2 modules x 2 timesteps, 3
prompts). Only data is written: seeds, per-call integer counts of the reference's gates (exact zeros, negatives), the
reference's per-call ratio, the saved sparsity.json bytes and the first call's output. No gate is stored; the tests
regenerate x and the weights from the seeds with synth.py.

Cases: relu; gelu with gate bias 0 (negatives in every call); gelu with gate bias -3.0 (deep-negative gates flush to
-0 in fp16 and count as zeros). The generator fails if one of these facts does not hold.

Fixture kind: sparsity. index.json is left alone.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sparsity_golden.py
"""
from __future__ import annotations

import os
import sys
import tempfile

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402
import make_neuron_golden as NG  # noqa: E402
import synth  # noqa: E402


def saved_json(meter):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "sparsity.json")
        meter.save(p)
        with open(p, "rb") as f:
            return np.frombuffer(f.read(), dtype=np.uint8).copy()


def gen_sparsity(sp_mod, utils):
    cases = []
    C, N, T, L, P = 320, 32, 2, 2, 3
    for i, (act, gb) in enumerate([("relu", 0.0), ("gelu", 0.0), ("gelu", -3.0)]):
        seed = 7600 + 10 * i
        mods = NG.modules(C, seed, L, act, gb)
        rec = MG.quiet(sp_mod.SparsityMeasure, 0)
        results = utils.StatMeter(T=T, n_layers=L)
        zeros, negs, ratios, out0 = [], [], [], None
        for p in range(P):
            rec.gates = []  # base_receiver.py: observe_activation starts every prompt with an empty list
            for call in range(T * L):
                x = torch.from_numpy(synth.tokens((2, N, C), NG.x_seed(seed, p, 0, call))).half()
                with torch.no_grad():
                    o = rec.hook_fn(mods[call % L], (x,), None)
                if out0 is None:
                    out0 = o.numpy()
            gates = rec.gates
            assert len(gates) == T * L and gates[0].dtype == torch.float16 and gates[0].shape == (2, N, 4 * C)
            z, n, r = [], [], []
            for i0 in range(0, len(gates), L):  # check_sparsity.py:34-46
                for j, gate in enumerate(gates[i0:i0 + L]):
                    mask = gate == 0.0
                    exact_zero_ratio = mask.int().sum(-1).float() / gate.shape[-1]
                    exact_zero_ratio = exact_zero_ratio.mean()
                    results.update(exact_zero_ratio.item(), i0 // L, j)
                    r.append(exact_zero_ratio.item())
                    z.append(int(mask.sum()))
                    n.append(int((gate < 0).sum()))
            zeros.append(z)
            negs.append(n)
            ratios.append(r)
        zeros, negs, ratios = np.array(zeros, np.int64), np.array(negs, np.int64), np.array(ratios, np.float64)
        elements = 2 * N * 4 * C
        if act == "relu":
            assert (negs == 0).all() and (ratios > 0.3).all() and (ratios < 0.7).all(), ratios
        elif gb == 0.0:
            assert (negs > 0).all(), negs
        else:
            assert (zeros > 0).any(), zeros
        cases.append(dict(
            name=f"sparsity_C{C}_{act}_gb{gb}", kind="sparsity", dtype="float16", C=C, N=N, T=T, L=L, P=P, act=act,
            seed=seed, gate_bias=gb, zeros=zeros, negatives=negs, elements=elements, ratio_ref=ratios,
            json=saved_json(results), out0=out0))
    return cases


def main():
    MG.install_stubs()
    MG.load_ref("neuron_receivers.base_receiver", "neuron_receivers/base_receiver.py")
    utils = MG.load_ref("utils", "utils.py")
    sp = MG.load_ref("neuron_receivers.sparsity_measure", "neuron_receivers/sparsity_measure.py")
    NG.save(gen_sparsity(sp, utils))


if __name__ == "__main__":
    main()
