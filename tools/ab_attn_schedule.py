"""A/B of the two decode attention schedules on one GPU, interleaved in one process: us per attention launch (HIP events on the
library stream, nvllm_profile_kernel) of the default per-sequence schedule and of the balanced one, for a list of contexts.

    python tools/ab_attn_schedule.py --ctx 8192 --fill 63x128          # one long conversation among 63 short ones
    python tools/ab_attn_schedule.py --ctx 2048 --wgs 0,256            # batch 1; automatic span count and one span per CU
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nano_vllm_candle_amd as pkg

ap = argparse.ArgumentParser()
ap.add_argument("--ctx", default="8192", help="comma-separated context lengths, one sequence each")
ap.add_argument("--fill", default="", help="NxLEN: N more sequences of LEN tokens")
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--steps", type=int, default=24, help="decode steps per arm and round")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--wgs", default="0", help="comma-separated attn_balanced_wgs values to time (0 = automatic)")
ap.add_argument("--kv-bits", default="16,16", help="K,V cache widths")
a = ap.parse_args()

lens = [int(x) for x in a.ctx.split(",") if x]
if a.fill:
    n, ln = a.fill.split("x")
    lens += [int(ln)] * int(n)
arms = [("per_sequence", 0)] + [("balanced", int(w)) for w in a.wgs.split(",")]

# Qwen3-0.6B layer shapes, a few layers, a small vocabulary: the attention launch is the model's own
cfg = pkg.Qwen3Config.tiny(vocab_size=8192, hidden_size=1024, head_dim=128, num_hidden_layers=a.layers, num_attention_heads=16,
                           num_key_value_heads=8, intermediate_size=3072, max_position_embeddings=max(lens) + 4096)
ctx = pkg.Context(0)
m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 0, ctx)
k_bits, v_bits = (int(x) for x in a.kv_bits.split(","))
m.set_kv_cache_bits(k_bits, v_bits)
spare = a.steps * a.rounds * len(arms) + 16
m.kv_alloc(sum((n + spare) // 256 + 1 for n in lens), len(lens), 2048)
rng = np.random.default_rng(0)
m.step(list(range(len(lens))), [rng.integers(0, cfg.vocab_size, n).tolist() for n in lens], True)
for _ in range(4):
    m.decode_next()
us = {arm: [] for arm in arms}
for _ in range(a.rounds):
    for arm in arms:  # interleaved: every arm sees the same machine state, contexts grow by a few tokens only
        m.set_attention_schedule(arm[0])
        m.set_option("attn_balanced_wgs", arm[1])
        m.decode_next()  # the arm's first step is not timed
        m.profile_kernel("attn")
        for _ in range(a.steps):
            m.decode_next()
        ms, launches = m.profile_read()
        m.profile_kernel(None)
        us[arm].append(1e3 * ms / launches)
print(f"contexts: {len(lens)} sequences, longest {max(lens)}, mean {np.mean(lens):.0f} tokens; K/V {k_bits}/{v_bits} bits; "
      f"{a.layers} layers, {a.steps} steps x {a.rounds} rounds per arm")
for arm in arms:
    v = np.array(us[arm])
    print(f"{arm[0]:>12} wgs={arm[1]:<4} {np.median(v):8.2f} us per attention launch (min {v.min():.2f}, max {v.max():.2f} over rounds)")
