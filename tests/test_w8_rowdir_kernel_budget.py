"""CPU: every instantiation of the FP8 register-direct decode GEMM runs without scratch, and the four forms the Qwen3-0.6B
layer uses at 64 rows keep at least four waves per SIMD, as their bf16 twins do (hipcc's own report, written beside the
library by the build)."""
import os

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nano-vllm-candle_amd", "kernel_resources_w8_rowdir.txt")


def test_fp8_rowdir_kernels_keep_their_register_budget():
    assert os.path.exists(PATH), "kernel_resources_w8_rowdir.txt missing: rebuild the library (make -C nano-vllm-candle_amd/csrc)"
    res = {}
    for blk in open(PATH).read().split("Function Name: ")[1:]:
        lines = blk.strip().splitlines()
        res[lines[0].strip()] = {k.strip(): int(v) for k, v in (l.split(":", 1) for l in lines[1:])}
    hits = {n: r for n, r in res.items() if n.startswith("_ZN5nvllm21gemm_rowdir_w8_kernelILi")}
    assert len(hits) == 22, sorted(hits)  # the (NT, TK) pairs of the planner: 9 for epilogue 0, 5 for 1, 8 for 2
    for n, r in hits.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (n, r)
    for inst in ("4ELi16ELi2ELi2E", "1ELi16ELi4ELi0E", "6ELi16ELi2ELi1E", "1ELi16ELi6ELi0E"):  # QKV, o_proj, gate/up, down_proj
        (r,) = [r for n, r in hits.items() if n.startswith("_ZN5nvllm21gemm_rowdir_w8_kernelILi" + inst)]
        assert r["Occupancy [waves/SIMD]"] >= 4, (inst, r)
