"""GPU: the 8-bit K/V cache (per (token, kv head) row 128 e4m3 codes + one f32 scale) and its attention kernel
(attn_kv8_kernel<1 | 2>), reached through the public calls: layers.Attention(kv_bits=(8, 8)), set_kv_cache_bits(8, 8)
and the kv_k_bits / kv_v_bits options."""
import numpy as np
import pytest

from tests.test_fp8_weights_gpu import E4M3, FINITE, e4m3_encode
from tests.test_kv24_prefill_gpu import attention_f64
from tests.test_operating_point_gpu import oracle_rows
from tests.test_ops_gpu import ATTN_OP_TOL
from tests.util import LOGITS_TOL, oracle_config, rel_err, row_rel_err

pytestmark = pytest.mark.gpu

# Logits of the hd-128 tiny config on an 8-bit pool against the oracle: the worst row measured over every step of
# test_model_on_an_8_bit_pool is 5.03e-2 (e4m3 keeps 3 mantissa bits, 2^-4 relative per stored element: the attention op alone
# is 3.5e-2 .. 6.7e-2 off attention on unquantised K/V, test_attention_against_the_dequantised_cache prints it); the bound
# is twice that, for accumulation order across builds.
KV8_LOGITS_MEASURED = 5.03e-2
KV8_LOGITS_TOL = 2 * KV8_LOGITS_MEASURED
SHAPES = [(2, 4, 2, 33), (1, 8, 1, 130), (2, 4, 2, 300), (1, 16, 8, 97)]


@pytest.fixture(scope="module")
def pkg():
    import nano_vllm_candle_amd as p

    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    from nano_vllm_candle_amd import layers

    return layers.default_context()


def quantise_rows(x):
    """the numpy twin of the cache writers: per row of 128, scale = amax / 448 (1 for a zero row), code = e4m3(x / scale)"""
    amax = np.abs(x).max(-1, keepdims=True)
    scale = np.where(amax > 0, amax / np.float32(448), np.float32(1)).astype(np.float32)
    return E4M3[e4m3_encode(x / scale)] * scale


def exact_rows(rng, shape, lo, hi):
    """rows that quantise without error: e4m3 values times a power-of-two row scale, one element of each row at +-448"""
    x = E4M3[rng.choice(FINITE, shape)]
    at = rng.integers(0, shape[-1], shape[:-1])
    np.put_along_axis(x, at[..., None], rng.choice([-448.0, 448.0], shape[:-1])[..., None].astype(np.float32), -1)
    return (x * 2.0 ** rng.integers(lo, hi, shape[:-1] + (1,))).astype(np.float32)


# (2,4,2,33): one token in the second 32-token half; (1,8,1,130): gqa 8, one token in the third 64-token step;
# (2,4,2,300): crosses a block; (1,16,8,97): gqa 2
@pytest.mark.parametrize("B,nh,kv,T", SHAPES)
def test_attention_on_exactly_representable_rows(ctx, B, nh, kv, T):
    from nano_vllm_candle_amd import layers

    rng = np.random.default_rng(8000 + T)
    q = rng.standard_normal((B, nh, T, 128)).astype(np.float32)
    k, v = exact_rows(rng, (B, kv, T, 128), -12, -6), exact_rows(rng, (B, kv, T, 128), -10, -3)  # seven octaves of row scales
    assert np.array_equal(quantise_rows(k), k) and np.array_equal(quantise_rows(v), v)
    err = rel_err(layers.Attention(nh, 128, 128 ** -0.5, ctx=ctx, kv_bits=(8, 8))(q, k, v), attention_f64(q, k, v))
    print(f"[parity] 8-bit attention, exact rows, B={B} nh={nh} kv={kv} T={T}: {err:.3e} (op bound {ATTN_OP_TOL:g})")
    assert err < ATTN_OP_TOL


@pytest.mark.parametrize("B,nh,kv,T", SHAPES)
def test_attention_against_the_dequantised_cache(ctx, B, nh, kv, T):
    from nano_vllm_candle_amd import layers

    rng = np.random.default_rng(1000 * T + nh)
    q = rng.standard_normal((B, nh, T, 128)).astype(np.float32)
    k = (rng.standard_normal((B, kv, T, 128)) * 2.0 ** rng.uniform(-2, 2, (1, kv, 1, 128))).astype(np.float32)
    v = (rng.standard_normal((B, kv, T, 128)) * 2.0 ** rng.uniform(-2, 2, (1, kv, 1, 128))).astype(np.float32)
    got = layers.Attention(nh, 128, 128 ** -0.5, ctx=ctx, kv_bits=(8, 8))(q, k, v)
    err = rel_err(got, attention_f64(q, quantise_rows(k), quantise_rows(v)))
    print(f"[parity] 8-bit attention vs the dequantised cache, B={B} nh={nh} kv={kv} T={T}: {err:.3e} (op bound {ATTN_OP_TOL:g}); "
          f"vs unquantised K/V {rel_err(got, attention_f64(q, k, v)):.3e}")
    assert err < ATTN_OP_TOL


def tiny(pkg):
    return pkg.Qwen3Config.tiny(hidden_size=256, head_dim=128, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
                                num_hidden_layers=3, vocab_size=1024)


# (600,): set_attn_split cuts a context of more than 512 tokens (16 tiles) while sequences x kv heads < 512: the decode
# step at context 600 runs 5 parts of 4 tiles and the combine pass
@pytest.mark.parametrize("lens,n_decode", [((250, 37, 5), 8), ((600,), 2)])
def test_model_on_an_8_bit_pool(pkg, ctx, oracle, lens, n_decode):
    cfg = tiny(pkg)
    om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(3)
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 3, ctx)
    m.set_kv_cache_bits(8, 8)
    rng = np.random.default_rng(8)
    seqs = [rng.integers(0, cfg.vocab_size, n).tolist() for n in lens]
    sids = list(range(len(seqs)))
    # (a) the same tokens cached by the prefill form in one chunk, in 128-row chunks, and read by the decode form.  "All three
    # read the same codes" holds only while the projections run ONE kernel family: chunks of <= 128 rows take the fused
    # decode path (deferred norm), larger ones the generic path, and the 1e-4 by which their logits differ on a 16-bit pool
    # flips e4m3 codes (measured here: 1.55e-3 for (250, 37, 5), 8.5e-4 for (600,), printed below).  no_fused pins the path.
    ways = {}
    for way, chunk, no_fused in (("one chunk", 1024, 1), ("n - 1 + decode", 1024, 1), ("chunked", 128, 1), ("default path", 128, 0)):
        m.set_option("no_fused", no_fused)
        m.kv_alloc(num_blocks=6, max_seqs=4, max_batched_tokens=chunk)
        if way == "n - 1 + decode":
            m.step(sids, [s[:-1] for s in seqs], True)
        ways[way] = m.step(sids, seqs, way != "n - 1 + decode", want_logits=True)
    assert m.kv_bytes_per_token == cfg.num_hidden_layers * cfg.num_key_value_heads * 2 * 132
    agree = {way: (row_rel_err(ways[way][1], ways["chunked"][1]), bool(np.array_equal(ways[way][0], ways["chunked"][0])))
             for way in ("one chunk", "n - 1 + decode", "default path")}
    print(f"[parity] 8-bit pool {lens}: (logits error, ids equal) vs chunked prefill {agree} (tolerance {LOGITS_TOL:g})")
    ids, lg = ways["default path"]  # (b) goes on from the chunked prefill with every option at its default
    worst = 0.0
    for step in range(n_decode + 1):  # the 250-token sequence crosses its block edge at the 7th decode step
        if step:
            ids, lg = m.step(sids, seqs, False, want_logits=True)
        worst = max(worst, row_rel_err(lg, oracle_rows(om, seqs)[1]))
        for s, t in zip(seqs, ids):
            s.append(int(t))
    print(f"[parity] 8-bit pool {lens}: worst logits row vs the oracle {worst:.3e} (bound {KV8_LOGITS_TOL:g} = 2 x {KV8_LOGITS_MEASURED:g})")
    assert all(agree[way][0] < LOGITS_TOL and agree[way][1] for way in ("one chunk", "n - 1 + decode")), agree
    assert worst < KV8_LOGITS_TOL
    assert m.counter("attn_kv8_launches") > 0 and m.counter("attn_prefill_launches") == 0
    m.close()


def test_fork_copies_codes_and_scales(pkg, ctx):
    cfg = tiny(pkg)
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 3, ctx)
    m.set_kv_cache_bits(8, 8)
    m.kv_alloc(num_blocks=6, max_seqs=4, max_batched_tokens=512)
    seq = np.random.default_rng(4).integers(0, cfg.vocab_size, 300).tolist()  # 300 cached: a shared block and a 44-token tail
    ids, _ = m.step([0], [seq], True)
    m.seq_fork(0, 1)
    seq.append(int(ids[0]))
    _, lg = m.step([0, 1], [seq, seq], False, want_logits=True)
    assert np.array_equal(lg[0], lg[1]) and np.isfinite(lg).all()
    m.close()


def test_refusals(pkg, ctx):
    from nano_vllm_candle_amd import layers

    def refused(fn, *a):
        with pytest.raises(pkg._lib.NvllmError) as e:
            fn(*a)
        assert e.value.code == pkg._lib.EINVAL

    m = pkg.Qwen3ForCausalLM.from_synthetic(tiny(pkg), 3, ctx)
    for bits in ((8, 16), (16, 8), (8, 24), (24, 8), (24, 16)):
        refused(m.set_kv_cache_bits, *bits)
    x = np.zeros((1, 2, 4, 64), np.float32)
    refused(layers.Attention(2, 64, 0.125, ctx=ctx, kv_bits=(8, 8)), x, x, x)  # head_dim 64
    refused(layers.Attention(2, 128, 0.125, ctx=ctx, kv_bits=(8, 16)), *[np.zeros((1, 2, 4, 128), np.float32)] * 3)
    m64 = pkg.Qwen3ForCausalLM.from_synthetic(pkg.Qwen3Config.tiny(), 3, ctx)
    refused(m64.set_kv_cache_bits, 8, 8)
    m64.close()
    # a debug pair that does not match is refused by kv_alloc, and the pool that was there stays
    m.kv_alloc(num_blocks=6, max_seqs=4, max_batched_tokens=128)
    m.step([0], [[1, 2, 3]], True)
    m.set_option("kv_k_bits", 8)
    refused(m.kv_alloc, 6, 4, 128)
    assert m.free_blocks() == 5
    m.set_option("kv_v_bits", 8)
    m.kv_alloc(num_blocks=6, max_seqs=4, max_batched_tokens=128)
    assert m.kv_bytes_per_token == 3 * 2 * 2 * 132
    m.close()


def test_fp8_weights_with_an_8_bit_pool_run_the_slab_qkv(pkg, ctx):
    cfg = tiny(pkg)
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 3, ctx)
    m.set_weight_format("fp8")
    m.set_kv_cache_bits(8, 8)
    m.set_option("tile_min_wgs", 1)
    m.kv_alloc(num_blocks=6, max_seqs=4, max_batched_tokens=512)
    seq = np.random.default_rng(5).integers(0, cfg.vocab_size, 300).tolist()
    _, lg = m.step([0], [seq], True, want_logits=True)
    assert np.isfinite(lg).all()
    assert m.counter("tile_gemm_launches") > 0 and m.counter("tile_qkv_fused_launches") == 0 and m.counter("attn_kv8_launches") == 3
    m.close()
