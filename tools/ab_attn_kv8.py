"""A/B of the 16-bit and the 8-bit K/V cache on one GPU: us per decode attention launch (HIP events on the library stream,
nvllm_profile_kernel kind 1), two models in one process with their rounds interleaved, at a list of contexts.

    python tools/ab_attn_kv8.py --heads 16,8 --hidden 1024 --inter 3072      # the Qwen3-0.6B layer
    python tools/ab_attn_kv8.py --heads 32,8 --hidden 4096 --inter 12288     # the Qwen3-8B layer
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nano_vllm_candle_amd as pkg

ap = argparse.ArgumentParser()
ap.add_argument("--ctx", default="512,4096,8192", help="comma-separated context lengths")
ap.add_argument("--seqs", type=int, default=64)
ap.add_argument("--heads", default="16,8", help="q heads, kv heads (head_dim 128)")
ap.add_argument("--hidden", type=int, default=1024)
ap.add_argument("--inter", type=int, default=3072)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--steps", type=int, default=16, help="decode steps per arm and round")
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()

nh, kv = (int(x) for x in a.heads.split(","))
ctxs = [int(x) for x in a.ctx.split(",")]
cfg = pkg.Qwen3Config.tiny(vocab_size=8192, hidden_size=a.hidden, head_dim=128, num_hidden_layers=a.layers, num_attention_heads=nh,
                           num_key_value_heads=kv, intermediate_size=a.inter, max_position_embeddings=max(ctxs) + 4096)
ctx = pkg.Context(0)
arms = {}
for bits in (16, 8):
    arms[bits] = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 0, ctx)
    arms[bits].set_kv_cache_bits(bits, bits)
print(f"{a.seqs} sequences, {nh}/{kv} heads of 128, hidden {a.hidden}, {a.layers} layers; {a.steps} steps x {a.rounds} rounds per arm, interleaved")
rng = np.random.default_rng(0)
for n in ctxs:
    spare = a.steps * a.rounds + a.rounds + 16
    prompts = [rng.integers(0, cfg.vocab_size, n).tolist() for _ in range(a.seqs)]
    for m in arms.values():  # every sequence has blocks of its own: the launch reads all of them from HBM
        m.kv_alloc(a.seqs * ((n + spare) // 256 + 1), a.seqs, 4096)
        m.step(list(range(a.seqs)), prompts, True)
        for _ in range(4):
            m.decode_next()
    us = {bits: [] for bits in arms}
    for _ in range(a.rounds):
        for bits, m in arms.items():
            m.decode_next()  # the arm's first step of a round is not timed
            m.profile_kernel("attn")
            for _ in range(a.steps):
                m.decode_next()
            ms, launches = m.profile_read()
            m.profile_kernel(None)
            us[bits].append(1e3 * ms / launches)
    med = {bits: float(np.median(v)) for bits, v in us.items()}
    for bits, v in us.items():
        gb = a.seqs * n * arms[bits].kv_bytes_per_token / a.layers / 1e9
        print(f"context {n:5d}  K/V {bits:2d} bits  {med[bits]:9.2f} us per attention launch (min {min(v):.2f}, max {max(v):.2f} over rounds), "
              f"{gb:.3f} GB of K/V per launch = {gb / med[bits] * 1e3:.2f} TB/s")
    print(f"context {n:5d}  8-bit / 16-bit time {med[8] / med[16]:.3f}")
