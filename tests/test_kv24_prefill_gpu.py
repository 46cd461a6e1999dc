"""GPU: the 24-bit K/V cache (f16 + an e5m2 residual byte per element) in the two prefill kernels -- the LDS-staged
attention (attn_prefill_kernel<128, 2, VLO>) and the fused QKV tile-GEMM epilogue (gemm_tile_kernel<8, 2, 4 | 5>) --
reached through the public calls: layers.Attention(kv_bits=...) and Qwen3ForCausalLM.set_kv_cache_bits."""
import numpy as np
import pytest

from tests.test_operating_point_gpu import check_rows, oracle_rows
from tests.test_ops_gpu import ATTN_OP_TOL
from tests.util import LOGITS_TOL, oracle_config, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import nano_vllm_candle_amd as p

    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    from nano_vllm_candle_amd import layers

    return layers.default_context()


def attention_f64(q, k, v):
    B, nh, T, hd = q.shape
    g = nh // k.shape[1]  # q head h reads kv head h // g
    k, v = np.repeat(k.astype(np.float64), g, axis=1), np.repeat(v.astype(np.float64), g, axis=1)
    s = np.einsum("bhtd,bhsd->bhts", q.astype(np.float64), k) * hd ** -0.5
    s = np.where(np.tril(np.ones((T, T), bool)), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("bhts,bhsd->bthd", p / p.sum(-1, keepdims=True), v).reshape(B * T, nh * hd)


# (2,4,2,33): the second tile holds one token; (1,8,1,130): gqa 8, the 3-stage ring wraps, ragged tail; (2,4,2,300): crosses
# a 256-token block, 10 tiles, empty pad tiles; (1,16,8,97): gqa 2, exactly 4 tiles
@pytest.mark.parametrize("B,nh,kv,T", [(2, 4, 2, 33), (1, 8, 1, 130), (2, 4, 2, 300), (1, 16, 8, 97)])
def test_prefill_attention_24_bit_cache_vs_float64(pkg, ctx, B, nh, kv, T):
    # The bound on the K+V error is derived, not measured: the residual byte adds at least 2 significant bits to every
    # cache element (>= 4x less rounding); one factor of 2 is left for the bf8 operands of the residual MFMAs (which leave
    # that term 12 % accurate) and for accumulation order.  err16 comes from the 16-bit instantiation in the same test.
    from nano_vllm_candle_amd import layers

    rng = np.random.default_rng(1000 * T + nh)
    q = rng.standard_normal((B, nh, T, 128)).astype(np.float32)
    k = (rng.standard_normal((B, kv, T, 128)) * 2.0 ** rng.uniform(-2, 2, (1, kv, 1, 128))).astype(np.float32)
    v = (rng.standard_normal((B, kv, T, 128)) * 2.0 ** rng.uniform(-2, 2, (1, kv, 1, 128))).astype(np.float32)
    ref = attention_f64(q, k, v)
    err16, err_v24, err_kv24 = (rel_err(layers.Attention(nh, 128, 128 ** -0.5, ctx=ctx, kv_bits=bits)(q, k, v), ref)
                                for bits in ((16, 16), (16, 24), (24, 24)))
    print(f"[parity] prefill attention B={B} nh={nh} kv={kv} T={T}: 16-bit {err16:.3e}, 24-bit V {err_v24:.3e}, "
          f"24-bit K+V {err_kv24:.3e} (op bound {ATTN_OP_TOL:g})")
    assert max(err16, err_v24, err_kv24) < ATTN_OP_TOL
    assert err_kv24 < err16 / 2
    assert err_v24 < err16 * 1.2


@pytest.mark.parametrize("k_bits,v_bits", [(16, 24), (24, 24)])
def test_chunked_prefill_and_decode_on_a_24_bit_pool(pkg, ctx, oracle, k_bits, v_bits):
    # prompts (250, 37, 5) through 128-row chunks: later chunks start at positions > 0 (unmasked-tile path); the 250-token
    # sequence crosses the block boundary while decoding, on a cache the prefill writers wrote
    cfg = pkg.Qwen3Config.tiny(hidden_size=256, head_dim=128, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
                               num_hidden_layers=3, vocab_size=1024)
    om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(3)
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 3, ctx)
    with pytest.raises(pkg._lib.NvllmError) as e:
        m.set_kv_cache_bits(24, 16)
    assert e.value.code == pkg._lib.EINVAL
    m.set_kv_cache_bits(k_bits, v_bits)
    m.kv_alloc(num_blocks=6, max_seqs=4, max_batched_tokens=128)
    rng = np.random.default_rng(24)
    seqs = [rng.integers(0, cfg.vocab_size, n).tolist() for n in (250, 37, 5)]
    n_chunks = -(-sum(len(s) for s in seqs) // 128)
    for step in range(3):
        ids, lg = m.step([0, 1, 2], seqs, step == 0, want_logits=True)
        rid, rlg = oracle_rows(om, seqs)
        check_rows(f"K {k_bits} / V {v_bits} bits, step {step}", ids, lg, rid, rlg, LOGITS_TOL)
        assert m.counter("attn_prefill_launches") == cfg.num_hidden_layers * n_chunks
        for s, t in zip(seqs, rid):
            s.append(int(t))
    m.close()


# the smallest row counts at which the tile planner takes the 256 x 256 block (the only one with the fused epilogue) for
# N = (nh + 2 kv) * 128: the 128 x 256 block needs a second round of 256 workgroups from ceil(rows / 128) * N / 256 > 256
@pytest.mark.parametrize("nh,kv,rows", [(16, 8, 2100), (16, 2, 3210)])
def test_fused_qkv_epilogue_writes_the_24_bit_cache(pkg, ctx, oracle, nh, kv, rows):
    # one prompt chunk: 515 (crosses a block), 293 and 61 tokens, then fillers of 3..40: odd lengths, so 64-row wave tiles
    # start at pos % 4 != 0 and straddle sequences -- the LDS-transposed V path, its partial words, and the element-wise one
    cfg = pkg.Qwen3Config.tiny(hidden_size=256, head_dim=128, num_attention_heads=nh, num_key_value_heads=kv,
                               intermediate_size=512, num_hidden_layers=2, vocab_size=1024)
    om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(5)
    rng = np.random.default_rng(rows)
    lens = [515, 293, 61]
    while sum(lens) < rows:
        lens.append(min(int(rng.integers(3, 41)), rows - sum(lens)))
    seqs = [rng.integers(0, cfg.vocab_size, n).tolist() for n in lens]
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 5, ctx)
    m.set_option("tile_min_wgs", 1)
    m.set_kv_cache_bits(24, 24)
    m.kv_alloc(num_blocks=len(seqs) + 4, max_seqs=len(seqs), max_batched_tokens=rows)
    sids = list(range(len(seqs)))
    picked = [0, 1, 2, 3, len(seqs) // 2, len(seqs) - 1]  # the three long ones and three fillers
    for step in range(2):  # the prompt chunk, then one decode step over every sequence
        ids, lg = m.step(sids, seqs, step == 0, want_logits=True)
        assert m.counter("tile_qkv_fused_launches") == cfg.num_hidden_layers
        rid, rlg = oracle_rows(om, [seqs[i] for i in picked])
        check_rows(f"fused QKV epilogue nh={nh} kv={kv} rows={rows} step {step}", ids[picked], lg[picked], rid, rlg, LOGITS_TOL)
        for s, t in zip(seqs, ids):
            s.append(int(t))
    m.close()
