"""The FP8 weight GEMM (w8_gemm.hip) against the bf16 slab GEMMs on the Qwen3-8B / 32B layer shapes, kernel alone:
nvllm_debug_gemm_bench2 mode 8 (FP8) against mode 22 (streaming kernel, where it covers the shape) or mode 0 (planner's
chunked kernel), device events around 20 launches that cycle enough weight copies to stream cold HBM, arms interleaved,
three rounds; prints the median microseconds and the weight bytes per second of each arm.  Then the prompt-chunk rows
(512 and 4096): the FP8 prefill tile GEMM (w8_tile_gemm.hip, mode 9; mode 7 = its SwiGLU epilogue on gate_up) against
mode 8 (what FP8 chunks ran before it) and the bf16 tile GEMM (mode 1 / 3), with the MFMA rate of each arm.
`rowdir`: instead, the FP8 register-direct decode GEMM (w8_rowdir_gemm.hip, mode 30 + epilogue) against the bf16
gemm_rowdir_kernel (mode 10 + epilogue) and gemm_w8_kernel (mode 8) at the four Qwen3-0.6B layer shapes, 1 / 16 / 64 rows."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nano_vllm_candle_amd as pkg  # noqa: E402

SHAPES = {"8B qkv": (6144, 4096), "8B o": (4096, 4096), "8B gate_up": (24576, 4096), "8B down": (4096, 12288),
          "32B qkv": (10240, 5120), "32B o": (5120, 8192), "32B gate_up": (51200, 5120), "32B down": (5120, 25600)}


def main():
    ctx = pkg.Context(0)
    L = pkg._lib.lib()

    def bench(M, N, K, mode, rot):
        us = C.c_float()
        rc = L.nvllm_debug_gemm_bench2(ctx.h, M, N, K, 0, 0, 0, 0, mode, rot, 20, C.byref(us))
        return us.value if rc == 0 else float("nan")

    if sys.argv[1:] == ["rowdir"]:  # `ab_w8_gemm.py rowdir`: the fused decode path's GEMMs at the Qwen3-0.6B layer shapes
        # the FP8 register-direct kernel (mode 30 + epilogue) against its bf16 twin (10 + epilogue) and the FP8 slab GEMM (8)
        layer = {"0.6B qkv": (4096, 1024, 2), "0.6B o": (1024, 2048, 0), "0.6B gate_up": (6144, 1024, 1), "0.6B down": (1024, 3072, 0)}
        for name, (N, K, epi) in layer.items():
            for M in (1, 16, 64):
                rot = max(2, int(700e6 / (N * K * 2)))
                arms = {"fp8 rowdir": 30 + epi, "bf16 rowdir": 10 + epi, "fp8 gemm_w8": 8}
                t = {a: [] for a in arms}
                for _ in range(3):
                    for a, mode in arms.items():
                        t[a].append(bench(M, N, K, mode, rot))
                u = {a: statistics.median(v) for a, v in t.items()}
                print(f"{name:12s} epi {epi} M={M:3d}  " + "   ".join(f"{a} {u[a]:6.2f} us" for a in arms) +
                      f"   fp8/bf16 rowdir {u['fp8 rowdir'] / u['bf16 rowdir']:.2f}  rowdir/gemm_w8 {u['fp8 rowdir'] / u['fp8 gemm_w8']:.2f}", flush=True)
        return
    only_chunks = sys.argv[1:] == ["chunks"]  # `ab_w8_gemm.py chunks`: the prompt-chunk rows alone
    for name, (N, K) in SHAPES.items():
        for M in () if only_chunks else (1, 16, 64):
            rot = max(2, int(700e6 / (N * K * 2)))
            base_mode = 22 if bench(M, N, K, 22, 1) == bench(M, N, K, 22, 1) else 0  # NaN: the streaming kernel does not cover it
            t8, tb = [], []
            for _ in range(3):
                t8.append(bench(M, N, K, 8, rot))
                tb.append(bench(M, N, K, base_mode, rot))
            u8, ub = statistics.median(t8), statistics.median(tb)
            b8 = N * K + (N // 16) * (K // 128) * 4
            print(f"{name:12s} M={M:3d}  fp8 {u8:7.2f} us {b8 / u8 / 1e6:5.2f} TB/s   bf16 (mode {base_mode:2d}) {ub:7.2f} us "
                  f"{2 * N * K / ub / 1e6:5.2f} TB/s   fp8/bf16 time {u8 / ub:.2f}", flush=True)

    for name, (N, K) in SHAPES.items():
        gu = name.endswith("gate_up")
        for M in (512, 4096):
            rot = max(2, int(700e6 / (N * K * 2)))
            arms = {"fp8 tile": 7 if gu else 9, "fp8 gemm_w8": 8, "bf16 tile": 3 if gu else 1}
            t = {a: [] for a in arms}
            for _ in range(3):
                for a, mode in arms.items():
                    t[a].append(bench(M, N, K, mode, rot))
            u = {a: statistics.median(v) for a, v in t.items()}
            pf = 4.0 * M * N * K  # hi + lo planes
            print(f"{name:12s} M={M:4d}  " + "   ".join(f"{a} {u[a]:8.1f} us {pf / u[a] / 1e9:6.1f} PF/s" for a in arms) +
                  f"   tile/gemm_w8 {u['fp8 tile'] / u['fp8 gemm_w8']:.2f}  tile/bf16 tile {u['fp8 tile'] / u['bf16 tile']:.2f}", flush=True)


if __name__ == "__main__":
    main()
