"""CPU: the 8-bit-cache attention kernel (attn_kv8.hip) keeps the budget DESIGN.md states for it: the decode form at least two
waves per SIMD, neither form any scratch (hipcc's own report, written beside the library by the build)."""
import os

import pytest

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nano-vllm-candle_amd", "kernel_resources_kv8.txt")


@pytest.mark.parametrize("prefix,min_waves", [("_ZN5nvllm15attn_kv8_kernelILi1EEE", 2), ("_ZN5nvllm15attn_kv8_kernelILi2EEE", 1)])
def test_kv8_attention_kernel_keeps_its_register_budget(prefix, min_waves):
    assert os.path.exists(PATH), "kernel_resources_kv8.txt missing: rebuild the library (make -C nano-vllm-candle_amd/csrc)"
    res = {}
    for blk in open(PATH).read().split("Function Name: ")[1:]:
        lines = blk.strip().splitlines()
        res[lines[0].strip()] = {k.strip(): int(v) for k, v in (l.split(":", 1) for l in lines[1:])}
    hits = [r for n, r in res.items() if n.startswith(prefix)]
    assert len(hits) == 1, prefix
    assert hits[0]["Occupancy [waves/SIMD]"] >= min_waves and hits[0]["ScratchSize [bytes/lane]"] == 0, (prefix, hits[0])
