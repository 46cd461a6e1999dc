"""GPU: the FP8 prefill tile GEMM (w8_tile_gemm.hip) -- the kernel alone against float64 with both epilogues, an FP8 checkpoint
whose prompt chunk runs it against the oracle on the dequantised weights, and the same at TP = 2."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests.test_fp8_weights_gpu import CFGS, E4M3, FINITE, check_steps, expand, fp8_case, run_steps, write_checkpoint
from tests.util import bf16_round, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import nano_vllm_candle_amd as p

    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    from nano_vllm_candle_amd import layers

    return layers.default_context()


def linear_fp8_tile(pkg, ctx, x, codes, scales, mode, act_packed=0, n_split=0):
    N = codes.shape[0]
    dx, dy = ctx.to_device(x), ctx.empty((x.shape[0], N // 2 if mode == 2 else N))
    pkg._lib.check(pkg._lib.lib().nvllm_debug_linear_fp8_tile(ctx.h, dx.ptr, codes.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p),
                                                              x.shape[0], N, codes.shape[1], mode, act_packed, n_split, dy.ptr), ctx.h)
    return dy.numpy()


def operands(M, N, K, exps, arbitrary=False):
    """x, codes holding all 254 finite values, power-of-two block scales (a wrong block index is an error of order one), w"""
    rng = np.random.default_rng(1000 * M + N + K)
    codes = rng.permutation(np.concatenate([FINITE, rng.choice(FINITE, N * K - FINITE.size)])).reshape(N, K)
    sshape = (-(-N // 128), K // 128)
    scales = (2.0 ** rng.integers(exps[0], exps[1], sshape)).astype(np.float32)
    if arbitrary:
        scales = (scales * rng.uniform(0.5, 1.0, sshape)).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    return x, codes, scales, E4M3[codes].astype(np.float64) * expand(scales, (N, K)).astype(np.float64)


# rows: a partial 16-row tile, the 128-row block edge, two blocks and a partial third; 256 x 128: one scale block;
# 512 x 384: three blocks (no K split divides them), two feature blocks; 256 x 1024: K splits 1, 2, 4
MODE0 = [(M, N, K, ns, False) for M in (65, 129, 300) for N, K, ns in ((256, 128, 0), (512, 384, 0), (256, 1024, 1), (256, 1024, 2), (256, 1024, 4))]
MODE0.append((129, 512, 384, 0, True))  # arbitrary f32 scales


@pytest.mark.parametrize("M,N,K,n_split,arbitrary", MODE0)
def test_fp8_tile_gemm_against_float64(pkg, ctx, M, N, K, n_split, arbitrary):
    from nano_vllm_candle_amd import layers

    x, codes, scales, w = operands(M, N, K, (-6, 7), arbitrary)
    ref = x.astype(np.float64) @ w.T
    # power-of-two scales: w is bf16-exact, so nvllm_op_linear on it measures the same product; else on its bf16 rounding
    lin = layers.ReplicatedLinear(K, N, ctx=ctx)
    lin.load_weights(bf16_round(w.astype(np.float32)) if arbitrary else w.astype(np.float32))
    e_bf16, e_fp8 = rel_err(lin.forward(x), ref), rel_err(linear_fp8_tile(pkg, ctx, x, codes, scales, 0, 0, n_split), ref)
    print(f"M {M} N {N} K {K} split {n_split}: fp8 tile {e_fp8:.3e}  bf16 op_linear {e_bf16:.3e}")
    assert e_fp8 <= (2 * e_bf16 + 2.0 ** -8 if arbitrary else max(2 * e_bf16, 1e-6))


def test_fp8_tile_gemm_refuses_what_it_does_not_cover(pkg, ctx):
    x, codes, scales, _ = operands(65, 256, 384, (-6, 7))
    bad = [(x, codes[:128], scales[:1], 0, 0), (x, codes, scales, 0, 2), (x, codes, scales, 2, 3)]  # N % 256; 2 does not divide 3; split SwiGLU
    for xx, cc, ss, mode, ns in bad:
        with pytest.raises(pkg._lib.NvllmError) as e:
            linear_fp8_tile(pkg, ctx, xx, np.ascontiguousarray(cc), np.ascontiguousarray(ss), mode, 0, ns)
        assert e.value.code == pkg._lib.EINVAL


@pytest.mark.parametrize("act_packed", [0, 1])
@pytest.mark.parametrize("M,I,K", [(M, I, K) for M in (65, 300) for I, K in ((128, 128), (256, 384))])
def test_fp8_tile_swiglu_against_float64(pkg, ctx, M, I, K, act_packed):
    from nano_vllm_candle_amd import layers

    # scales 2^-10 .. 2^-7 keep gate and up of order one, where SiLU is not yet the identity
    x, codes, scales, w = operands(M, 2 * I, K, (-10, -6))
    gu = x.astype(np.float64) @ w.T
    g, u = gu[:, :I], gu[:, I:]
    ref = g / (1.0 + np.exp(-g)) * u
    lin = layers.ReplicatedLinear(K, 2 * I, ctx=ctx)
    lin.load_weights(w.astype(np.float32))
    e_ref = rel_err(layers.SiluAndMul(ctx).forward(lin.forward(x)), ref)
    e_fp8 = rel_err(linear_fp8_tile(pkg, ctx, x, codes, scales, 2, act_packed), ref)
    print(f"M {M} I {I} K {K} packed {act_packed}: fp8 tile {e_fp8:.3e}  op_linear + op_silu_mul {e_ref:.3e}")
    assert e_fp8 <= max(2 * e_ref, 2.0 ** -16)  # 2^-16: what a hi + lo bf16 plane pair can represent


# ---- models: hidden 256, 4 q / 2 kv heads of 128, intermediate 512 -- every projection is a multiple of 256 features wide,
# at TP = 2 as well; the 8 + 2 + 300-token prefill is one chunk of 310 rows (three row blocks, the last one partial)
@pytest.fixture(scope="module")
def case(pkg, oracle, tmp_path_factory):
    cfg, _, ckpt, steps = fp8_case(pkg, oracle, CFGS["hd128_tp2"])
    path = tmp_path_factory.mktemp("fp8_tile")
    write_checkpoint(path, cfg, ckpt)
    return cfg, str(path), steps


@pytest.mark.parametrize("tile_min_wgs", [1, 0])
def test_fp8_tile_model_against_the_oracle(pkg, ctx, case, tile_min_wgs):
    cfg, path, steps = case
    m = pkg.Qwen3ForCausalLM.from_hf_dir(path, ctx)
    m.set_option("tile_min_wgs", tile_min_wgs)
    m.kv_alloc(8, 4, 512)
    got = [m.step([0, 1, 2], steps[0][0], True, want_logits=True)]
    launches = m.counter("tile_gemm_launches")
    assert launches == (4 * cfg.num_hidden_layers if tile_min_wgs else 0)  # the predicates cover all four projections
    got += [m.step([0, 1, 2], seqs, False, want_logits=True) for seqs, _, _ in steps[1:]]
    assert m.counter("tile_gemm_launches") == launches  # decode rows stay on the FP8 GEMM
    check_steps(got, steps)


def test_fp8_tile_tp2_loopback(pkg, case):
    cfg, path, steps = case
    results, errors = [None, None], []

    def worker(rank):
        try:
            c = pkg.Context(0, tp_rank=rank, tp_size=2, loopback_group="gfp8tile")
            m = pkg.Qwen3ForCausalLM.from_hf_dir(path, c)
            m.set_option("tile_min_wgs", 1)
            results[rank] = (run_steps(m, steps), m.counter("tile_gemm_launches"))
            m.close()
            c.close()
        except Exception as e:  # noqa: BLE001
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert all(r is not None for r in results), "a rank hung"
    for got, launches in results:
        check_steps(got, steps)
        assert launches > 0
