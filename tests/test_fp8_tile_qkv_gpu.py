"""GPU: the fused QKV epilogue of the FP8 prefill tile GEMM (w8_tile_qkv_gemm.hip) -- FP8 checkpoints whose prompt chunks run
it, against the oracle on the dequantised weights: every K/V cache width, chunks that start past position 0, TP = 2 (a q
head paired with the k head, another with the v head), and a head count the kernel refuses.

The 8 + 2 + 300-token prefill is 310 rows.  As one chunk: three row blocks, the last one partial; the first wave tile holds
three sequences (V element-wise), the others start at position 54 (pos % 4 == 2: the transposed V path with partial
words), and one of them straddles the 256-token cache block edge.  The decode steps read the cache the epilogue wrote."""
import threading

import pytest

from tests.test_fp8_weights_gpu import CFGS, check_steps, fp8_case, write_checkpoint

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import nano_vllm_candle_amd as p

    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    from nano_vllm_candle_amd import layers

    return layers.default_context()


def make_case(pkg, oracle, tmp_path_factory, kw):
    cfg, _, ckpt, steps = fp8_case(pkg, oracle, kw)
    path = tmp_path_factory.mktemp("fp8_tile_qkv")
    write_checkpoint(path, cfg, ckpt)
    return cfg, str(path), steps


@pytest.fixture(scope="module")
def case(pkg, oracle, tmp_path_factory):  # hidden 256, 4 q / 2 kv heads of 128: NQ = 1024 = 4 feature blocks
    return make_case(pkg, oracle, tmp_path_factory, CFGS["hd128_tp2"])


def run(m, steps, max_batched_tokens=512):
    """prefill + the decode steps; (results, fused QKV launches of the prefill, tile launches of the prefill)"""
    m.set_option("tile_min_wgs", 1)
    m.kv_alloc(8, 4, max_batched_tokens)
    got = [m.step([0, 1, 2], steps[0][0], True, want_logits=True)]
    fused, tiles = m.counter("tile_qkv_fused_launches"), m.counter("tile_gemm_launches")
    got += [m.step([0, 1, 2], seqs, False, want_logits=True) for seqs, _, _ in steps[1:]]
    assert (m.counter("tile_qkv_fused_launches"), m.counter("tile_gemm_launches")) == (fused, tiles)  # decode rows stay off the tile GEMMs
    return got, fused, tiles


@pytest.mark.parametrize("fuse_qk", [1, 0])
@pytest.mark.parametrize("k_bits,v_bits", [(16, 16), (16, 24), (24, 24)])
def test_fp8_fused_qkv_against_the_oracle(pkg, ctx, case, k_bits, v_bits, fuse_qk):
    cfg, path, steps = case
    m = pkg.Qwen3ForCausalLM.from_hf_dir(path, ctx)
    m.set_kv_cache_bits(k_bits, v_bits)
    m.set_option("tile_fuse_qk", fuse_qk)
    got, fused, tiles = run(m, steps)
    assert fused == (cfg.num_hidden_layers if fuse_qk else 0)
    assert tiles == 4 * cfg.num_hidden_layers  # the predicates cover all four projections
    check_steps(got, steps)


# 192: chunks of 192 and 118 rows (the second on the fused decode path); 140: 140 + 140 + 30, the second fused chunk starts
# at position 130 of the long prompt and crosses the cache block edge
@pytest.mark.parametrize("max_batched_tokens", [192, 140])
def test_fp8_fused_qkv_through_chunks(pkg, ctx, case, max_batched_tokens):
    cfg, path, steps = case
    m = pkg.Qwen3ForCausalLM.from_hf_dir(path, ctx)
    got, fused, _ = run(m, steps, max_batched_tokens)
    chunks = [min(max_batched_tokens, 310 - r0) for r0 in range(0, 310, max_batched_tokens)]
    assert fused == cfg.num_hidden_layers * sum(c > 128 for c in chunks)
    check_steps(got, steps)


def test_fp8_fused_qkv_three_scale_blocks(pkg, ctx, oracle, tmp_path_factory):
    """hidden 384: three scale blocks = six stages (the three-stage ring wraps, the scale prefetch advances and clamps),
    and no K split divides them, so the predicate still takes the fused kernel"""
    cfg, path, steps = make_case(pkg, oracle, tmp_path_factory, dict(CFGS["hd128_tp2"], hidden_size=384))
    got, fused, _ = run(pkg.Qwen3ForCausalLM.from_hf_dir(path, ctx), steps)
    assert fused == cfg.num_hidden_layers
    check_steps(got, steps)


def test_fp8_fused_qkv_tp2_loopback(pkg, case):
    """per rank 2 q + 1 k + 1 v heads: NQ = 512, two blocks, (q0, k) and (q1, v)"""
    cfg, path, steps = case
    results, errors = [None, None], []

    def worker(rank):
        try:
            c = pkg.Context(0, tp_rank=rank, tp_size=2, loopback_group="gfp8qkv")
            m = pkg.Qwen3ForCausalLM.from_hf_dir(path, c)
            results[rank] = run(m, steps)
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
    for got, fused, _ in results:
        check_steps(got, steps)
        assert fused > 0


def test_fp8_fused_qkv_refuses_an_odd_head_count(pkg, ctx, oracle, tmp_path_factory):
    """3 q + 1 k + 1 v heads: NQ = 640 is no multiple of 256, the QKV projection stays on the slab GEMM + row kernel"""
    kw = dict(CFGS["hd128_tp2"], num_attention_heads=3, num_key_value_heads=1)
    cfg, path, steps = make_case(pkg, oracle, tmp_path_factory, kw)
    got, fused, _ = run(pkg.Qwen3ForCausalLM.from_hf_dir(path, ctx), steps)
    assert fused == 0
    check_steps(got, steps)
