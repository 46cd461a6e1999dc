"""A/B of the three ways to take a decode step, interleaved in one process on one GPU: the greedy fast path (decode_next), the
sampled fast path (decode_next_sample: the draw in the LM head's epilogue) and the sampled slow path (step_sample on full token
lists: logits stored, one sampler workgroup per row).  Median ms per step over rounds, host clock around calls that end in a
stream synchronise; every arm continues the same sequences, so contexts differ by a few tokens between arms only.

    python tools/ab_sampled_decode.py                      # Qwen3-0.6B shapes, 64 sequences, prompts U[64, 512]
    python tools/ab_sampled_decode.py --seqs 1 --prompt 128
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nano_vllm_candle_amd as pkg

ap = argparse.ArgumentParser()
ap.add_argument("--seqs", type=int, default=64)
ap.add_argument("--prompt", type=int, default=0, help="prompt length of every sequence; 0 = uniform in [64, 512]")
ap.add_argument("--steps", type=int, default=16, help="timed decode steps per arm and round")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--temperature", type=float, default=0.6)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()

cfg = pkg.Qwen3Config.qwen3_0_6b()
m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, a.seed, pkg.Context(0))
rng = np.random.default_rng(a.seed)
lens = [a.prompt] * a.seqs if a.prompt else rng.integers(64, 513, a.seqs).tolist()
arms = ["decode_next", "decode_next_sample", "step_sample"]
total = a.rounds * len(arms) * (a.steps + 1) + 8
m.kv_alloc(sum((n + total) // 256 + 1 for n in lens), a.seqs, 4096)
sids, temps = list(range(a.seqs)), [a.temperature] * a.seqs
toks = [rng.integers(0, cfg.vocab_size, n).tolist() for n in lens]


def step(arm):
    if arm == "decode_next":
        ids = m.decode_next()[:a.seqs]
    elif arm == "decode_next_sample":
        ids = m.decode_next_sample(temps, a.seed)[:a.seqs]
    else:
        ids, _ = m.step_sample(sids, toks, False, temps, a.seed)
    for t, i in zip(toks, ids):
        t.append(int(i))


ids, _ = m.step_sample(sids, toks, True, temps, a.seed)
for t, i in zip(toks, ids):
    t.append(int(i))
for arm in arms:  # warm-up: every arm's kernels loaded, the sampling state uploaded
    for _ in range(2):
        step(arm)
ms = {arm: [] for arm in arms}
for _ in range(a.rounds):
    for arm in arms:
        step(arm)  # the arm's first step after another arm is not timed
        m.ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step(arm)
        ms[arm].append(1e3 * (time.perf_counter() - t0) / a.steps)
print(f"Qwen3-0.6B shapes, {a.seqs} sequences, prompts {min(lens)}..{max(lens)} (mean {np.mean(lens):.0f}), temperature {a.temperature}, "
      f"seed {a.seed}; {a.steps} steps x {a.rounds} rounds per arm, interleaved")
for arm in arms:
    v = np.array(ms[arm])
    print(f"{arm:>20} {np.median(v):8.3f} ms/step (min {v.min():.3f}, max {v.max():.3f} over rounds)")
