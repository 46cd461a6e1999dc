"""CPU: the prefill kernels of the 24-bit K/V cache keep two waves per SIMD without scratch (hipcc's own report)."""
import pytest

from tests.test_abi import _kernel_resources


@pytest.mark.parametrize("prefix", ["_ZN5nvllm19attn_prefill_kernelILi128ELi2ELi0EEE", "_ZN5nvllm19attn_prefill_kernelILi128ELi2ELi1EEE",
                                    "_ZN5nvllm19attn_prefill_kernelILi128ELi2ELi2EEE",   # 16-bit, 24-bit V, 24-bit K+V
                                    "_ZN5nvllm16gemm_tile_kernelILi8ELi2ELi4EEE", "_ZN5nvllm16gemm_tile_kernelILi8ELi2ELi5EEE"])
def test_24_bit_prefill_kernels_keep_their_register_budget(prefix):
    hits = [r for n, r in _kernel_resources().items() if n.startswith(prefix)]
    assert len(hits) == 1, prefix
    assert hits[0]["Occupancy [waves/SIMD]"] >= 2 and hits[0]["ScratchSize [bytes/lane]"] == 0, (prefix, hits[0])
