"""GPU: block-scaled FP8 (e4m3) projection weights -- the FP8 GEMM alone against float64, FP8 models (checkpoint codes through
from_hf_dir, and bf16 weights quantised in place) against the oracle on the dequantised weights, TP = 2, and the refusals."""
import ctypes as C
import json
import struct
import threading

import numpy as np
import pytest

from tests.util import LOGITS_TOL, bf16_round, oracle_config, rel_err, row_rel_err

pytestmark = pytest.mark.gpu

# OCP e4m3fn: decode through a 256-entry table, encode by nearest-even search over the 127 non-negative finite values
_c = np.arange(256)
E4M3 = (np.where((_c >> 3) & 15, (1 + (_c & 7) / 8) * 2.0 ** (((_c >> 3) & 15) - 7), (_c & 7) * 2.0 ** -9) * np.where(_c & 0x80, -1, 1)).astype(np.float32)
E4M3[(_c & 0x7F) == 0x7F] = np.nan
FINITE = _c[(_c & 0x7F) != 0x7F].astype(np.uint8)


def e4m3_encode(x):
    pos = E4M3[:127].astype(np.float64)
    a = np.minimum(np.abs(x.astype(np.float64)), 448.0)
    hi = np.clip(np.searchsorted(pos, a), 1, 126)
    lo = hi - 1
    dl, dh = a - pos[lo], pos[hi] - a
    code = np.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def expand(scale, shape):
    return np.repeat(np.repeat(scale, 128, 0), 128, 1)[:shape[0], :shape[1]]


def quantise(w):
    """[R][C] f32 -> (codes, one f32 scale per 128 x 128 block, dequantised f32): scale = amax / 448, or 1 for a zero block"""
    br, bc = -(-w.shape[0] // 128), -(-w.shape[1] // 128)
    wp = np.zeros((br * 128, bc * 128), np.float32)
    wp[:w.shape[0], :w.shape[1]] = w
    amax = np.abs(wp).reshape(br, 128, bc, 128).max(axis=(1, 3))
    scale = np.where(amax > 0, amax / np.float32(448), np.float32(1)).astype(np.float32)
    codes = e4m3_encode(w / expand(scale, w.shape))
    return codes, scale, E4M3[codes] * expand(scale, w.shape)


@pytest.fixture(scope="module")
def pkg():
    import nano_vllm_candle_amd as p

    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    from nano_vllm_candle_amd import layers

    return layers.default_context()


def linear_fp8(pkg, ctx, x, codes, scales):
    dx, dy = ctx.to_device(x), ctx.empty((x.shape[0], codes.shape[0]))
    pkg._lib.check(pkg._lib.lib().nvllm_debug_linear_fp8(ctx.h, dx.ptr, codes.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p),
                                                         x.shape[0], codes.shape[0], codes.shape[1], dy.ptr), ctx.h)
    return dy.numpy()


# (128, 128): one block; (272, 384): partial scale block, odd K split, block-accumulator rollover; (256, 1024): many blocks
GEMM_CASES = [(M, N, K, False) for N, K in ((128, 128), (272, 384), (256, 1024)) for M in (1, 16, 17, 64, 129, 300)]
GEMM_CASES.append((17, 272, 384, True))  # arbitrary f32 scales


@pytest.mark.parametrize("M,N,K,arbitrary", GEMM_CASES)
def test_fp8_gemm_against_float64(pkg, ctx, M, N, K, arbitrary):
    from nano_vllm_candle_amd import layers

    rng = np.random.default_rng(1000 * M + N + K)
    codes = rng.permutation(np.concatenate([FINITE, rng.choice(FINITE, N * K - FINITE.size)])).reshape(N, K)  # all 254 finite codes
    sshape = (-(-N // 128), -(-K // 128))
    scales = (2.0 ** rng.integers(-6, 7, sshape)).astype(np.float32)  # a wrong block index is an error of order one
    if arbitrary:
        scales = (scales * rng.uniform(0.5, 1.0, sshape)).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = E4M3[codes].astype(np.float64) * expand(scales, (N, K)).astype(np.float64)
    ref = x.astype(np.float64) @ w.T
    # power-of-two scales: w is bf16-exact, so nvllm_op_linear on it measures the same product; else on its bf16 rounding
    lin = layers.ReplicatedLinear(K, N, ctx=ctx)
    lin.load_weights(bf16_round(w.astype(np.float32)) if arbitrary else w.astype(np.float32))
    e_bf16, e_fp8 = rel_err(lin.forward(x), ref), rel_err(linear_fp8(pkg, ctx, x, codes, scales), ref)
    print(f"M {M} N {N} K {K}: fp8 {e_fp8:.3e}  bf16 op_linear {e_bf16:.3e}")
    assert e_fp8 <= (2 * e_bf16 + 2.0 ** -8 if arbitrary else max(2 * e_bf16, 1e-6))


# ---- models ----------------------------------------------------------------------------------------------------------
CFGS = {"tiny": dict(), "hd128": dict(hidden_size=256, head_dim=128, num_key_value_heads=2, intermediate_size=384),
        "hd128_tp2": dict(hidden_size=256, head_dim=128, num_key_value_heads=2, intermediate_size=512)}


def fp8_case(pkg, oracle, kw, seed=7):
    """(config, tensors as a checkpoint holds them, the oracle on the dequantised weights, its greedy trajectory)"""
    cfg = pkg.Qwen3Config.tiny(**kw)
    om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(seed)
    f32 = {n: om.get_tensor(n, s) for n, s in cfg.hf_tensor_shapes().items()}
    ckpt = {}
    for n, t in f32.items():
        if "_proj.weight" in n:
            codes, scale, deq = quantise(t)
            om.set_tensor(n, deq)
            ckpt[n], ckpt[n + "_scale_inv"] = ("F8_E4M3", codes), ("F32", scale)
        else:
            ckpt[n] = ("BF16", (np.ascontiguousarray(t).view(np.uint32) >> 16).astype(np.uint16))  # synthetic values are bf16-exact
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, cfg.vocab_size, n).tolist() for n in (8, 2, 300)]  # 300: a chunk above 128 rows, across a block
    steps = []
    for _ in range(4):  # prefill, then three greedy steps
        rid, rlg = om.run_greedy(seqs)
        steps.append(([list(s) for s in seqs], rid, rlg))
        for s, t in zip(seqs, rid):
            s.append(int(t))
    return cfg, f32, ckpt, steps


def write_checkpoint(path, cfg, ckpt):
    """config.json with quantization_config + one model.safetensors (8-byte header length, JSON header, raw data)"""
    header, blobs, off = {}, [], 0
    for name, (dtype, arr) in ckpt.items():
        raw = np.ascontiguousarray(arr).tobytes()
        header[name] = {"dtype": dtype, "shape": list(arr.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(header).encode()
    hj += b" " * ((8 - len(hj) % 8) % 8)
    (path / "model.safetensors").write_bytes(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))
    d = {k: getattr(cfg, k) for k in cfg.__dataclass_fields__}
    d["quantization_config"] = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128]}
    (path / "config.json").write_text(json.dumps(d))


def run_steps(m, steps):
    m.kv_alloc(8, 4, 512)
    return [m.step([0, 1, 2], seqs, i == 0, want_logits=True) for i, (seqs, _, _) in enumerate(steps)]


def check_steps(got, steps):
    for (ids, lg), (_, rid, rlg) in zip(got, steps):
        assert row_rel_err(lg, rlg) < LOGITS_TOL, row_rel_err(lg, rlg)
        for k in range(len(rid)):  # tests/util.py's near-tie rule: two logits closer than twice the tolerance may swap
            gap = float(rlg[k, int(rid[k])] - rlg[k, int(ids[k])]) / float(np.abs(rlg[k]).max())
            assert 0.0 <= gap <= 2 * LOGITS_TOL, (k, int(ids[k]), int(rid[k]), gap)


@pytest.mark.parametrize("source", ["checkpoint", "quantise-after-load"])
@pytest.mark.parametrize("name", ["tiny", "hd128"])
def test_fp8_model_against_the_oracle(pkg, ctx, oracle, tmp_path, name, source):
    cfg, f32, ckpt, steps = fp8_case(pkg, oracle, CFGS[name])
    if source == "checkpoint":
        write_checkpoint(tmp_path, cfg, ckpt)
        m = pkg.Qwen3ForCausalLM.from_hf_dir(str(tmp_path), ctx)
        assert m.cfg == cfg
    else:
        m = pkg.Qwen3ForCausalLM.from_state_dict(cfg, f32, ctx)
        m.set_weight_format("fp8")
    mats = [((cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim, cfg.hidden_size),
            (cfg.hidden_size, cfg.num_attention_heads * cfg.head_dim), (2 * cfg.intermediate_size, cfg.hidden_size),
            (cfg.hidden_size, cfg.intermediate_size)]
    delta = cfg.num_hidden_layers * sum(-n * k + (n // 16) * (k // 128) * 4 for n, k in mats)  # one byte less per element, plus scales
    assert m.weight_bytes == pkg.Qwen3ForCausalLM(cfg, ctx).weight_bytes + delta
    check_steps(run_steps(m, steps), steps)


def test_fp8_checkpoint_tp2_loopback(pkg, oracle, tmp_path):
    cfg, _, ckpt, steps = fp8_case(pkg, oracle, CFGS["hd128_tp2"])  # intermediate_size must divide by 128 * tp
    write_checkpoint(tmp_path, cfg, ckpt)
    results, errors = [None, None], []

    def worker(rank):
        try:
            c = pkg.Context(0, tp_rank=rank, tp_size=2, loopback_group="gfp8")
            m = pkg.Qwen3ForCausalLM.from_hf_dir(str(tmp_path), c)
            results[rank] = run_steps(m, steps)
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
    for got in results:
        check_steps(got, steps)


def test_fp8_refusals(pkg, ctx, oracle):
    L = pkg._lib
    cfg, f32, ckpt, steps = fp8_case(pkg, oracle, CFGS["tiny"])
    q = "model.layers.0.self_attn.q_proj.weight"

    def code_of(fn):
        with pytest.raises(L.NvllmError) as e:
            fn()
        return e.value.code

    bf = pkg.Qwen3ForCausalLM(cfg, ctx)
    assert code_of(lambda: bf.load_tensor(q, ckpt[q][1], L.DTYPE_F8E4M3)) == L.EINVAL  # F8 into a bf16-format model
    m = pkg.Qwen3ForCausalLM(cfg, ctx, weight_format="fp8")
    assert code_of(lambda: m.load_tensor(q + "_scale_inv", np.ones((3, 1), np.float32))) == L.EINVAL  # wrong scale shape
    bad = ckpt[q][1].copy()
    bad[5, 9] = 0xFF
    assert code_of(lambda: m.load_tensor(q, bad, L.DTYPE_F8E4M3)) == L.EINVAL  # a NaN code
    for n, (dt, arr) in ckpt.items():
        if n != q + "_scale_inv":
            m.load_tensor(n, arr, {"F8_E4M3": L.DTYPE_F8E4M3, "F32": L.DTYPE_F32, "BF16": L.DTYPE_BF16}[dt])
    assert code_of(m.finalize) == L.ESTATE  # codes without their scales
    assert code_of(lambda: m.set_weight_format(7)) == L.EINVAL
    ok = pkg.Qwen3ForCausalLM.from_state_dict(cfg, f32, ctx)
    ok.set_weight_format("fp8")
    got = run_steps(ok, steps[:1])
    assert code_of(lambda: ok.set_weight_format("bf16")) == L.ESTATE  # after kv_alloc
    check_steps(got + [ok.step([0, 1, 2], s, False, want_logits=True) for s, _, _ in steps[1:]], steps)
