"""GPU: the FP8 register-direct decode GEMM (w8_rowdir_gemm.hip) -- the kernel alone against float64 with its three epilogues,
an FP8 model at the Qwen3-0.6B layer shapes on the fused path against the oracle on the dequantised weights, and TP = 2
shards that have no register-direct form (the all-or-nothing rule of fused_plan)."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests.test_fp8_tile_gpu import ctx, operands, pkg  # noqa: F401  (pkg, ctx: the module fixtures)
from tests.test_fp8_weights_gpu import check_steps, quantise, write_checkpoint
from tests.util import bf16_round, oracle_config, rel_err

pytestmark = pytest.mark.gpu


def linear_fp8_rowdir(pkg, ctx, x, codes, scales, epi, xp, op, resid=None, next_w=None, row_ssq=None):
    """(y, x_next, ssq_out) of nvllm_debug_linear_fp8_rowdir; the last two for epilogue 0 only"""
    M, (N, K) = x.shape[0], codes.shape
    dx, dr, dw, ds = (ctx.to_device(a) if a is not None else None for a in (x, resid, next_w, row_ssq))
    ptr = lambda d: d.ptr if d is not None else None  # noqa: E731
    dy = ctx.empty((M, N // 2 if epi == 1 else N))
    dxn, dq = (ctx.empty((M, N)), ctx.empty((M,))) if epi == 0 else (None, None)
    pkg._lib.check(pkg._lib.lib().nvllm_debug_linear_fp8_rowdir(
        ctx.h, dx.ptr, codes.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p), M, N, K, epi, xp, op, ptr(dr), ptr(dw),
        ptr(ds), dy.ptr, ptr(dxn), ptr(dq)), ctx.h)
    return dy.numpy(), dxn.numpy() if epi == 0 else None, dq.numpy() if epi == 0 else None


# (epi, M, N or I, K, x_packed, o_packed, arbitrary scales).  K 1024 / 2048 / 3072 / 4096 = 2 / 4 / 6 / 8 k-tiles per wave (3072:
# a wave's slice straddles a scale-block edge, on either side by the wave's parity); M 1 and 16 take the one-row-block shapes
# (fewer n-tiles per workgroup), 17 leaves fifteen dead rows in its second block.  The 0.6B layer's forms: epi 2 N 1024 runs
# QKV's (1 n-tile at M <= 16, else 4); epi 0 N 1024 is o_proj (K 2048) and down_proj (K 3072); epi 1 I 1536, K 1024 is gate/up
# (2 n-tiles at M <= 16, else 6).  N 1040 = 65 n-tiles: a ragged last workgroup and a partial ninth scale row; N 2064 = 129
# n-tiles in groups of 4: the ssq sum through LDS with a ragged last group.
CASES = [(2, 1, 1024, 1024, 0, 0), (2, 16, 1024, 2048, 0, 0), (2, 17, 1024, 3072, 0, 0), (2, 17, 1024, 3072, 1, 0), (2, 64, 1024, 4096, 1, 0),
         (2, 64, 1040, 1024, 0, 0), (2, 17, 1040, 2048, 1, 0, True),  # True: arbitrary f32 scales
         (0, 1, 1024, 2048, 0, 0), (0, 16, 1024, 3072, 0, 0), (0, 17, 1024, 3072, 1, 1), (0, 64, 1024, 2048, 1, 1), (0, 64, 1024, 1024, 0, 1),
         (0, 64, 1024, 4096, 0, 0), (0, 17, 2064, 1024, 1, 0), (0, 64, 2064, 1024, 0, 0),
         (1, 1, 1536, 1024, 0, 0), (1, 16, 1536, 1024, 0, 0), (1, 17, 1536, 1024, 1, 1), (1, 64, 1536, 1024, 1, 1), (1, 64, 1536, 1024, 0, 0),
         (1, 17, 512, 2048, 0, 1), (1, 64, 512, 2048, 1, 0)]


@pytest.mark.parametrize("epi,M,N,K,xp,op,arbitrary", [c if len(c) == 7 else c + (False,) for c in CASES])
def test_fp8_rowdir_gemm_against_float64(pkg, ctx, epi, M, N, K, xp, op, arbitrary):  # noqa: F811
    from nano_vllm_candle_amd import layers

    rng = np.random.default_rng(7 * M + N + K + epi)
    if epi == 1:  # N = I here; scales 2^-12 .. 2^-9 keep gate and up of order one, where SiLU is not yet the identity
        x, codes, scales, w = operands(M, 2 * N, K, (-12, -8))
    else:
        x, codes, scales, w = operands(M, N, K, (-6, 7), arbitrary)
    # power-of-two scales: w is bf16-exact, so nvllm_op_linear on it measures the same product; else on its bf16 rounding
    lin = layers.ReplicatedLinear(K, w.shape[0], ctx=ctx)
    lin.load_weights(bf16_round(w.astype(np.float32)) if arbitrary else w.astype(np.float32))
    prod, prod_bf16 = x.astype(np.float64) @ w.T, lin.forward(x)
    tag = f"epi {epi} M {M} N {N} K {K} packed {xp}/{op}:"
    if epi == 2:
        y, _, _ = linear_fp8_rowdir(pkg, ctx, x, codes, scales, 2, xp, op)
        e_bf16, e_fp8 = rel_err(prod_bf16, prod), rel_err(y, prod)
        print(f"{tag} fp8 {e_fp8:.3e}  bf16 op_linear {e_bf16:.3e}")
        assert e_fp8 <= (2 * e_bf16 + 2.0 ** -8 if arbitrary else max(2 * e_bf16, 1e-6))
    elif epi == 1:
        row_ssq = (rng.uniform(0.5, 2.0, M) * K).astype(np.float32)  # a pending norm: rinv = 1 / sqrt(ssq / K + 1e-6)
        rinv = 1.0 / np.sqrt(row_ssq.astype(np.float64) / K + 1e-6)
        g, u = prod[:, :N] * rinv[:, None], prod[:, N:] * rinv[:, None]
        ref = g / (1.0 + np.exp(-g)) * u
        e_ref = rel_err(layers.SiluAndMul(ctx).forward((prod_bf16 * rinv[:, None]).astype(np.float32)), ref)
        y, _, _ = linear_fp8_rowdir(pkg, ctx, x, codes, scales, 1, xp, op, row_ssq=row_ssq)
        e_fp8 = rel_err(y, ref)
        print(f"{tag} fp8 {e_fp8:.3e}  op_linear + op_silu_mul {e_ref:.3e}")
        assert e_fp8 <= max(2 * e_ref, 2.0 ** -16)  # 2^-16: what a hi + lo bf16 plane pair can represent
    else:
        resid = (rng.standard_normal((M, N)) * np.abs(prod).max()).astype(np.float32)
        next_w = rng.uniform(0.5, 2.0, N).astype(np.float32)
        ref = resid.astype(np.float64) + prod
        host = prod_bf16 + resid  # op_linear + the residual add and the norm weight on the host, in f32
        y, x_next, ssq = linear_fp8_rowdir(pkg, ctx, x, codes, scales, 0, xp, op, resid=resid, next_w=next_w)
        e_bf16, e_y = rel_err(host, ref), rel_err(y, ref)
        e_ref, e_x = rel_err(host * next_w, ref * next_w), rel_err(x_next, ref * next_w)
        ssq_ref = (ref ** 2).sum(axis=1)
        e_sq = float(np.abs(ssq / ssq_ref - 1).max())
        print(f"{tag} resid fp8 {e_y:.3e} ref {e_bf16:.3e}  x' fp8 {e_x:.3e} ref {e_ref:.3e}  ssq fp8 {e_sq:.3e}")
        assert e_y <= max(2 * e_bf16, 1e-6)
        assert e_x <= max(2 * e_ref, 2.0 ** -16)
        assert e_sq <= max(4 * e_bf16, 1e-6)  # squares double the relative error


# ---- models: two layers at the Qwen3-0.6B layer shapes (the configuration of smoke()) ---------------------------------------
SHAPES = dict(vocab_size=8192, hidden_size=1024, head_dim=128, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=8, intermediate_size=3072)
_CASES = {}


def model_case(pkg, oracle, tmp_path_factory, batch):
    """(config, checkpoint directory, greedy trajectory of the oracle on the dequantised weights), built once per batch"""
    if "ckpt" not in _CASES:
        cfg = pkg.Qwen3Config.tiny(**SHAPES)
        om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(7)
        ckpt = {}
        for n, s in cfg.hf_tensor_shapes().items():
            t = om.get_tensor(n, s)
            if "_proj.weight" in n:
                codes, scale, deq = quantise(t)
                om.set_tensor(n, deq)
                ckpt[n], ckpt[n + "_scale_inv"] = ("F8_E4M3", codes), ("F32", scale)
            else:
                ckpt[n] = ("BF16", (np.ascontiguousarray(t).view(np.uint32) >> 16).astype(np.uint16))  # synthetic values are bf16-exact
        path = tmp_path_factory.mktemp("fp8_rowdir")
        write_checkpoint(path, cfg, ckpt)
        _CASES["ckpt"] = (cfg, str(path), om)
    cfg, path, om = _CASES["ckpt"]
    if batch not in _CASES:
        rng = np.random.default_rng(batch)
        seqs = [rng.integers(0, cfg.vocab_size, 2 + (i % 11)).tolist() for i in range(batch)]  # prompts of 2 .. 12 tokens
        steps = []
        for _ in range(4):  # prefill, then three greedy steps
            rid, rlg = om.run_greedy(seqs)
            steps.append(([list(s) for s in seqs], rid, rlg))
            for s, t in zip(seqs, rid):
                s.append(int(t))
        _CASES[batch] = steps
    return cfg, path, _CASES[batch]


def run_model(m, steps):
    """prefill in chunks of at most 128 rows (each one a fused chunk), then the decode steps; returns (outputs, chunks run)"""
    ids = list(range(len(steps[0][0])))
    m.kv_alloc(len(ids) + 2, len(ids), 128)
    got = [m.step(ids, seqs, i == 0, want_logits=True) for i, (seqs, _, _) in enumerate(steps)]
    return got, -(-sum(len(s) for s in steps[0][0]) // 128) + len(steps) - 1


@pytest.mark.parametrize("batch,option", [(1, None), (17, None), (17, "no_xpack"), (33, None), (17, "no_fused")])
def test_fp8_rowdir_model_against_the_oracle(pkg, ctx, oracle, tmp_path_factory, batch, option):  # noqa: F811
    cfg, path, steps = model_case(pkg, oracle, tmp_path_factory, batch)
    m = pkg.Qwen3ForCausalLM.from_hf_dir(path, ctx)
    if option:
        m.set_option(option, 1)
    got, chunks = run_model(m, steps)
    check_steps(got, steps)
    # all four projections of every layer of every chunk, or (generic path) none
    assert m.counter("w8_rowdir_launches") == (0 if option == "no_fused" else 4 * cfg.num_hidden_layers * chunks)
    m.close()


def test_fp8_rowdir_tp2_shards_without_a_form_stay_generic(pkg, oracle, tmp_path_factory):  # noqa: F811
    # per rank: o_proj K 1024, gate/up I 1536, down_proj K 1536 -- no register-direct form for the last, so no projection fuses
    cfg, path, steps = model_case(pkg, oracle, tmp_path_factory, 17)
    results, errors = [None, None], []

    def worker(rank):
        try:
            c = pkg.Context(0, tp_rank=rank, tp_size=2, loopback_group="gfp8rowdir")
            m = pkg.Qwen3ForCausalLM.from_hf_dir(path, c)
            results[rank] = (run_model(m, steps)[0], m.counter("w8_rowdir_launches"))
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
        assert launches == 0
