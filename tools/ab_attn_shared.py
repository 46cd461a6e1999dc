"""A/B of the default decode attention schedule and the shared-prefix one on one GPU, interleaved in one process: us per
attention launch (HIP events on the library stream, nvllm_profile_kernel) and, for the shared-prefix arm, us of the row
kernel it puts in front (q/k norm + RoPE + KV write, which the default launch does in its prologue).

    python tools/ab_attn_shared.py --forks 64 --shared 2048      # a parent of 2049 tokens and 64 forks of it
    python tools/ab_attn_shared.py --forks 0 --lone 64x300       # no family at all: what the schedule costs with nothing to share
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nano_vllm_candle_amd as pkg

ap = argparse.ArgumentParser()
ap.add_argument("--forks", type=int, default=8, help="forks of the one parent (0: no parent either)")
ap.add_argument("--shared", type=int, default=512, help="tokens in whole shared blocks: the parent's prompt is one token longer")
ap.add_argument("--lone", default="", help="NxLEN: N more sequences of LEN tokens that share nothing")
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--steps", type=int, default=24, help="decode steps per arm, kernel class and round")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--kv-bits", default="16,16", help="K,V cache widths")
a = ap.parse_args()

lens = [a.shared + 1] if a.forks else []
if a.lone:
    n, ln = a.lone.split("x")
    lens += [int(ln)] * int(n)
arms = ["per_sequence", "shared_prefix"]
n_seqs = len(lens) + a.forks

# Qwen3-0.6B layer shapes, a few layers, a small vocabulary: the attention launch is the model's own
cfg = pkg.Qwen3Config.tiny(vocab_size=8192, hidden_size=1024, head_dim=128, num_hidden_layers=a.layers, num_attention_heads=16,
                           num_key_value_heads=8, intermediate_size=3072, max_position_embeddings=max(lens) + 4096)
ctx = pkg.Context(0)
m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 0, ctx)
k_bits, v_bits = (int(x) for x in a.kv_bits.split(","))
m.set_kv_cache_bits(k_bits, v_bits)
spare = 2 * a.steps * a.rounds * len(arms) + 64
m.kv_alloc(sum((n + spare) // 256 + 1 for n in lens) + a.forks * (spare // 256 + 2), n_seqs, 4096)
rng = np.random.default_rng(0)
seqs = [rng.integers(0, cfg.vocab_size, n).tolist() for n in lens]
sids = list(range(len(lens)))
m.step(sids, seqs, True)
for j in range(a.forks):  # every fork goes its own way from a token of its own
    m.seq_fork(0, len(lens) + j)
    sids.append(len(lens) + j)
    seqs.append(seqs[0] + [j + 1])
seqs[:len(lens)] = [s + [0] for s in seqs[:len(lens)]]
m.step(sids, seqs, False)
for _ in range(4):
    m.decode_next()
us = {(arm, kind): [] for arm in arms for kind in ("attn", "qk")}
for _ in range(a.rounds):
    for arm in arms:  # interleaved: every arm sees the same machine state, contexts grow by a few tokens only
        m.set_attention_schedule(arm)
        m.decode_next()  # the arm's first step is not timed
        for kind in ("attn", "qk"):
            m.profile_kernel(kind)
            for _ in range(a.steps):
                m.decode_next()
            ms, launches = m.profile_read()
            m.profile_kernel(None)
            n_attn = a.steps * a.layers
            us[arm, kind].append(1e3 * ms / n_attn if launches else 0.0)
print(f"{n_seqs} sequences: {a.forks} forks of a {a.shared + 1 if a.forks else 0}-token parent, {len(lens) - bool(a.forks)} that share nothing ({a.lone or '-'}); "
      f"K/V {k_bits}/{v_bits} bits; {a.layers} layers, {a.steps} steps x {a.rounds} rounds per arm; "
      f"shared-prefix launches {m.counter('attn_shared_launches')}")
for arm in arms:
    v, q = np.array(us[arm, "attn"]), np.array(us[arm, "qk"])
    print(f"{arm:>14} {np.median(v):8.2f} us per attention launch (min {v.min():.2f}, max {v.max():.2f} over rounds)"
          f" + {np.median(q):6.2f} us row kernel = {np.median(v) + np.median(q):8.2f}")
