"""bench.py's own contract: a plain run prints the headline line only, `--steps` is the number of timed steps, and
`--dump-outputs` writes what the last timed step returned (the greedy id of every live sequence)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "kernel_ms_per_step", "prefill", "cpu_baseline", "tp_scaling", "tp_projection", "all_decode_steps")


def test_bench_rejects_zero_timed_steps():
    # the timed loop always enqueues at least one step: --steps 0 could not mean what it says
    cp = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert cp.returncode == 2 and "--steps" in cp.stderr


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_ids_equal_the_same_steps_in_process(tmp_path):
    import bench
    import nano_vllm_candle_amd as pkg
    from nano_vllm_candle_amd import layers

    steps, warmup = 3, 2
    cp = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                         "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-2000:]
    lines = [l for l in cp.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == "decode tokens/sec" and out["unit"] == "tokens/s" and out["higher_is_better"] is True
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0 and "dtype" in out
    assert out["value"] == pytest.approx(64 * 1e3 / out["ms_per_step"], rel=1e-9)  # one step = one token of each of 64 sequences
    assert not [k for k in FULL_ONLY if k in out]
    assert os.listdir(tmp_path) == ["next_ids.npy"]
    got = np.load(tmp_path / "next_ids.npy")
    assert got.dtype == np.float64 and got.shape == (64,)

    # the same workload here: prefill, then warmup + steps device-feedback decode steps; the last one's ids
    cfg = pkg.Qwen3Config.qwen3_0_6b()
    prompts = bench.make_prompts(cfg, 64, 64, 512, 0)
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 0, layers.default_context())
    m.kv_alloc(num_blocks=64 * 3, max_seqs=64, max_batched_tokens=4096)
    m.step(list(range(64)), prompts, True)
    for _ in range(warmup + steps):
        ids = m.decode_next()[:64].copy()
    m.close()
    assert got.tolist() == ids.astype(np.float64).tolist()
