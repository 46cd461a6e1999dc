"""CPU: every instantiation of the fused-QKV FP8 prefill tile GEMM runs without scratch and keeps two waves per SIMD (hipcc's
own report, written beside the library by the build)."""
import os

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nano-vllm-candle_amd", "kernel_resources_w8_tile_qkv.txt")


def test_fp8_tile_qkv_kernels_keep_their_register_budget():
    assert os.path.exists(PATH), "kernel_resources_w8_tile_qkv.txt missing: rebuild the library (make -C nano-vllm-candle_amd/csrc)"
    res = {}
    for blk in open(PATH).read().split("Function Name: ")[1:]:
        lines = blk.strip().splitlines()
        res[lines[0].strip()] = {k.strip(): int(v) for k, v in (l.split(":", 1) for l in lines[1:])}
    hits = {n: r for n, r in res.items() if n.startswith("_ZN5nvllm23gemm_w8_tile_qkv_kernelILi")}
    assert len(hits) == 3, sorted(hits)  # 16-bit K/V, 24-bit V, 24-bit K and V
    for n, r in hits.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (n, r)
        assert r["Occupancy [waves/SIMD]"] >= 2, (n, r)
