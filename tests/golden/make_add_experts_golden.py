"""Golden vectors for AddExperts, made by running the REFERENCE's own AddExperts.hook_fn.

Runs only in the build container (the reference tree is not present on the GPU box). Through make_golden's stub of
the absent `diffusers` package it imports, from the reference tree,
  * AddExperts (constructor and hook_fn)   neuron_receivers/add_skilled_experts.py:9-71
  * helper.modify_ffn                      moefication/helper.py:48-62 (labels -> patterns, k; E = 4C / 20, top-k 0.2)
and runs the hook on the CPU in fp16 on seeded inputs. Only data is written (seeds, lists, statistics, recorded
outputs); the tests regenerate x and the weights from the seeds with synth.py.

The constructor reads its lists from path_expert_indx and its statistics from
<prefix before adj>/<adj>/predictivity_base_expert.json with adj = path_expert_indx.split('/')[-3] (:13-15), so both are
written into a temporary directory of the shape <tmp>/<adj>/x/y. The generator sets rec.timestep / rec.layer before
every hooked call.
Cells of the T = L = 2 grid, in call order: (0, 0) a single expert, (0, 1) a list longer than k' = int(0.8 k),
(1, 0) a list with a duplicate id, (1, 1) an empty list. The first call, whose out and masked gate are recorded, is
therefore a biased one.
std: positive, u * sigma with u uniform in [0.1, 0.3) and sigma the standard deviation of all expert scores of a
probe call of the module -- the bias 5 * std is then 0.5 - 1.5 sigma, which reorders rows without putting every listed
expert first in every row (asserted below).
Token seeds: every token ROW of a call has its own seed (x_seeds [calls, 2 N]; row r of the call is
synth.tokens((C,), seed)). They are searched on the reference's arithmetic alone: while more than 5 % of the call's rows
are near-tie rows under test_gpu_route_parity.near_tie_rows(biased score, k', slack_ulps=8), the seed of each such row
moves on by one and the whole call is evaluated again. (One seed for the whole call, as expert_freq uses for its 32
image-0 rows, cannot meet the cap here: about three rows in ten are near-tie rows at 8 ulps, and at C = 1280 all 16
rows of a call must be clear.) The device GEMM's summation order may legitimately reorder a near-tie row's k'-th and
(k'+1)-th experts, and the tests leave those rows out.

Fixture kind: add_experts. index.json is left alone.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_add_experts_golden.py
"""
from __future__ import annotations

import json
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
import synth  # noqa: E402
from make_expert_golden import NEAR_CAP, TOPK, modules, near_tie_rows  # noqa: E402
from make_neuron_golden import save  # noqa: E402

ADJ = "adj_add_experts"
TL = [(0, 0), (0, 1), (1, 0), (1, 1)]


def row_tokens(seeds, N, C):
    """x [2, N, C] fp16 from one seed per token row."""
    return torch.from_numpy(np.stack([synth.tokens((C,), int(s)) for s in seeds]).reshape(2, N, C)).half()


def cell_lists(rng, E, kk):
    single = [int(rng.integers(E))]
    longer = sorted(int(e) for e in rng.choice(E, size=kk + 3, replace=False))
    a, b, c = (int(e) for e in rng.choice(E, size=3, replace=False))
    return {(0, 0): single, (0, 1): longer, (1, 0): [a, b, a, c], (1, 1): []}


def gen_add_experts(helper, add_mod):
    near = near_tie_rows()
    cases = []
    T, L = 2, 2
    spec = [(320, 32, "relu"), (320, 32, "gelu"), (1280, 8, "gelu")]
    for i, (C, N, act) in enumerate(spec):
        seed = 8400 + 10 * i
        mods, labels, E = modules(helper, C, seed, L, act, 0.0)
        k = int(mods[0].k)
        kk = int(0.8 * k)
        rng = np.random.default_rng(seed)
        lists = cell_lists(rng, E, kk)
        std = {}
        for (t, l) in TL:
            m = mods[l]
            probe = torch.from_numpy(synth.tokens((2, N, C), seed + 500 + 2 * t + l)).half()
            with torch.no_grad():
                g = m.gelu(m.proj(probe).chunk(2, dim=-1)[1])
                sigma = float(torch.matmul(g.view(-1, 4 * C), m.patterns.transpose(0, 1)).float().std())
            std[(t, l)] = [float(v) for v in sigma * rng.uniform(0.1, 0.3, E)]
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, ADJ, "x", "y")
            os.makedirs(path)
            for (t, l), ids in lists.items():
                with open(os.path.join(path, f"timestep_{t}_layer_{l}.json"), "w") as f:
                    json.dump(ids, f)
            stats = {"time_steps": {str(t): {str(l): {"avg": [0.0] * E, "std": std[(t, l)]} for l in range(L)}
                                    for t in range(T)}}
            with open(os.path.join(d, ADJ, "predictivity_base_expert.json"), "w") as f:
                json.dump(stats, f)
            rec = MG.quiet(add_mod.AddExperts, 0, path, T, L)
        x_seeds, n_near, scores, labs, biases, out0, gate0, steps = [], [], [], [], [], None, None, []
        for call, (t, l) in enumerate(TL):
            m, ids = mods[l], lists[(t, l)]
            # (the searches of two rows never meet)
            seeds = np.array([seed + 1000 + 1000000 * call + 10000 * r for r in range(2 * N)], dtype=np.int64)
            first = seeds.copy()
            while True:
                x = row_tokens(seeds, N, C)
                with torch.no_grad():
                    gate = m.gelu(m.proj(x).chunk(2, dim=-1)[1])
                    raw = torch.matmul(gate.view(-1, 4 * C), m.patterns.transpose(0, 1))
                    score = raw.clone()
                    score[:, ids] = score[:, ids] + 5.0 * torch.tensor(std[(t, l)]).to(score.dtype)[ids]
                nr = near(score.numpy(), kk, slack_ulps=8)
                if int(nr.sum()) <= NEAR_CAP * 2 * N:
                    break
                seeds[nr] += 1
            nn_ = int(nr.sum())
            rec.timestep, rec.layer = t, l
            with torch.no_grad():
                out = MG.quiet(rec.hook_fn, m, (x,), None)
            lab = torch.topk(score, k=kk, dim=-1)[1]
            # the recorded score and indices are the hook's own: its masked gate keeps exactly these experts' neurons
            keep = torch.nn.functional.embedding(lab, m.patterns).sum(-2) != 0
            assert torch.equal(rec.gates[-1].view(-1, 4 * C) != 0, keep & (gate.view(-1, 4 * C) != 0))
            if ids:
                on = torch.zeros(score.shape, dtype=torch.bool).scatter_(1, lab, True)
                raw_on = torch.zeros(score.shape, dtype=torch.bool).scatter_(1, torch.topk(raw, k=kk, dim=-1)[1], True)
                listed = sorted(set(ids))
                assert not bool(on[:, listed].all()), "the bias puts every listed expert into every row's selection"
                assert bool((on != raw_on).any()), "the bias changes no selection"
            bias = torch.zeros(E, dtype=torch.float16)
            if ids:
                bias[ids] = (5.0 * torch.tensor(std[(t, l)]).to(torch.float16))[ids]
            x_seeds.append(seeds.copy())
            steps.append(int((seeds - first).sum()))
            n_near.append(nn_)
            scores.append(score.numpy())
            labs.append(lab.numpy())
            biases.append(bias.numpy())
            if call == 0:
                out0, gate0 = out.numpy(), rec.gates[-1].numpy()
        assert len(lists[(0, 1)]) > kk and len(set(lists[(1, 0)])) < len(lists[(1, 0)]) and lists[(1, 1)] == []
        cases.append(dict(
            name=f"add_experts_C{C}_{act}", kind="add_experts", dtype="float16", C=C, N=N, T=T, L=L, E=E, k=k, kk=kk,
            act=act, seed=seed, gate_bias=0.0, topk=TOPK, labels=labels, call_tl=np.array(TL), x_seeds=np.stack(x_seeds),
            n_near=np.array(n_near), lists=json.dumps({f"{t},{l}": v for (t, l), v in lists.items()}),
            std=np.array([std[tl] for tl in TL], dtype=np.float64), bias=np.stack(biases), score=np.stack(scores),
            labels_topk=np.stack(labs), out0=out0, gate0=gate0))
        print(f"  add_experts_C{C}_{act}: k' = {kk}, near-tie rows {n_near}, "
              f"seed steps {steps}", flush=True)
    return cases


def main():
    MG.install_stubs()
    helper = MG.load_ref("moefication_helper_ref", "moefication/helper.py")
    MG.load_ref("neuron_receivers.base_receiver", "neuron_receivers/base_receiver.py")
    MG.load_ref("utils", "utils.py")
    MG.load_ref("neuron_receivers.predictivity", "neuron_receivers/predictivity.py")
    add = MG.load_ref("neuron_receivers.add_skilled_experts", "neuron_receivers/add_skilled_experts.py")
    save(gen_add_experts(helper, add))


if __name__ == "__main__":
    main()
