"""CPU: the shared-prefix decode attention kernel keeps the two waves per SIMD DESIGN.md states for it, without scratch, at
every cache width (hipcc's own report)."""
import pytest

from tests.test_abi import _kernel_resources


@pytest.mark.parametrize("prefix", ["_ZN5nvllm18attn_shared_kernelILi128ELi0EEE", "_ZN5nvllm18attn_shared_kernelILi128ELi1EEE",
                                    "_ZN5nvllm18attn_shared_kernelILi128ELi2EEE"])  # 16-bit, 24-bit V, 24-bit K+V
def test_shared_attention_kernel_keeps_its_register_budget(prefix):
    hits = [r for n, r in _kernel_resources().items() if n.startswith(prefix)]
    assert len(hits) == 1, prefix
    assert hits[0]["Occupancy [waves/SIMD]"] == 2 and hits[0]["ScratchSize [bytes/lane]"] == 0, (prefix, hits[0])
