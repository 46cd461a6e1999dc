"""GPU: the work-balanced decode attention schedule (attn_balanced_kernel<128, VLO> behind its device-built plan), reached
through Qwen3ForCausalLM.set_attention_schedule, against the oracle's dense forward."""
import numpy as np
import pytest

from tests.test_operating_point_gpu import check_rows, oracle_rows
from tests.util import LOGITS_TOL, oracle_config

pytestmark = pytest.mark.gpu

# 700: crosses 256-token blocks, 22 tiles over >= 3 spans; 255 -> 256 crosses a block while decoding; 32 (and 33 + 31 one and
# two steps on) start a fresh tile that holds only the new token; 1: a single cached token
PROMPTS = (700, 255, 33, 32, 31, 5, 1)
N_STEPS = 8  # prefill, 3 x step, 2 x decode_next, 2 x decode_enqueue / collect


@pytest.fixture(scope="module")
def pkg():
    import nano_vllm_candle_amd as p

    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    from nano_vllm_candle_amd import layers

    return layers.default_context()


def tiny(pkg, nh, kv, hd=128):
    return pkg.Qwen3Config.tiny(hidden_size=256, head_dim=hd, num_attention_heads=nh, num_key_value_heads=kv, intermediate_size=512,
                               num_hidden_layers=2, vocab_size=1024)


@pytest.fixture(scope="module")
def reference(pkg, oracle):
    """(config, oracle model, [(token lists, greedy ids, logits) per step]) per head layout: the oracle decodes greedily on its own"""
    cache = {}

    def get(nh, kv):
        if (nh, kv) not in cache:
            cfg = tiny(pkg, nh, kv)
            om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(7)
            rng = np.random.default_rng(11)
            seqs = [rng.integers(0, cfg.vocab_size, n).tolist() for n in PROMPTS]
            steps = []
            for _ in range(N_STEPS):
                rid, rlg = oracle_rows(om, seqs)
                steps.append(([list(s) for s in seqs], rid, rlg))
                for s, t in zip(seqs, rid):
                    s.append(int(t))
            cache[nh, kv] = cfg, om, steps
        return cache[nh, kv]

    return get


def drive(pkg, ctx, ref, k_bits, v_bits, wgs):
    """the whole call sequence on a fresh pool; returns (model, the step() logits, every step's ids, the GPU's token lists)"""
    cfg, _, steps = ref
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 7, ctx)
    m.set_kv_cache_bits(k_bits, v_bits)
    m.set_attention_schedule("balanced")
    m.set_option("attn_balanced_wgs", wgs)
    m.kv_alloc(num_blocks=12, max_seqs=8, max_batched_tokens=1024)
    n, L = len(PROMPTS), cfg.num_hidden_layers
    logits, all_ids = [], []
    for k in range(4):  # the caller feeds the oracle's tokens: every step is comparable on its own
        ids, lg = m.step(list(range(n)), steps[k][0], k == 0, want_logits=True)
        check_rows(f"balanced wgs={wgs} K{k_bits}/V{v_bits} step {k}", ids, lg, steps[k][1], steps[k][2], LOGITS_TOL)
        assert m.counter("attn_balanced_launches") == L * k  # the prefill step runs none
        logits.append(lg)
        all_ids.append(np.array(ids))
    live = [list(s) for s in steps[4][0]]
    same = np.ones(n, bool)  # rows that have followed the oracle's tokens so far (a near-tie may part them)

    def resident(k, got):
        srt = np.sort(steps[k][2], axis=1)
        clear = (srt[:, -1] - srt[:, -2]) / np.abs(steps[k][2]).max(axis=1) > 2 * LOGITS_TOL
        assert (got == steps[k][1])[same & clear].all(), (k, got, steps[k][1])
        same[:] &= got == steps[k][1]
        for s, t in zip(live, got):
            s.append(int(t))
        all_ids.append(got)

    for k in (4, 5):  # the plan advances on the device: no host metadata from here on
        resident(k, np.array(m.decode_next()[:n]))
    m.decode_enqueue()
    m.decode_enqueue()
    for k in (6, 7):
        resident(k, np.array(m.decode_collect()[:n]))
    assert m.counter("attn_balanced_launches") == L * 7
    return m, logits, all_ids, live


# wgs 1: one workgroup walks every sequence, no merge; 3: spans begin and end mid-sequence and swallow short sequences whole;
# 0: automatic -- floor-sized spans at this size, the most merges
@pytest.mark.parametrize("wgs", [1, 3, 0])
@pytest.mark.parametrize("nh,kv,k_bits,v_bits", [(4, 2, 16, 16), (8, 1, 16, 16), (4, 2, 16, 24), (4, 2, 24, 24)])
def test_ragged_batch_vs_oracle(pkg, ctx, reference, nh, kv, k_bits, v_bits, wgs):
    drive(pkg, ctx, reference(nh, kv), k_bits, v_bits, wgs)[0].close()


def test_replay_is_bit_equal_and_tickets_re_arm(pkg, ctx, reference):
    ref = reference(4, 2)
    m1, lg1, ids1, _ = drive(pkg, ctx, ref, 16, 16, 3)
    m1.close()
    m2, lg2, ids2, live = drive(pkg, ctx, ref, 16, 16, 3)
    for a, b in zip(lg1 + ids1, lg2 + ids2):  # merged in span order, not arrival order
        assert np.array_equal(a, b)
    m2.seq_free(0)  # a new batch composition over tickets every earlier step has used
    sids = list(range(1, len(PROMPTS)))
    ids, lg = m2.step(sids, live[1:], False, want_logits=True)
    rid, rlg = oracle_rows(ref[1], live[1:])
    check_rows("balanced, after freeing the longest sequence", ids, lg, rid, rlg, LOGITS_TOL)
    m2.close()


def test_interface_and_head_dim_64_fallback(pkg, ctx, oracle):
    cfg = tiny(pkg, 4, 2, hd=64)
    om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(7)
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 7, ctx)
    with pytest.raises(pkg._lib.NvllmError) as e:
        m.set_attention_schedule("round_robin")
    assert e.value.code == pkg._lib.EINVAL
    m.set_attention_schedule("balanced")
    m.kv_alloc(num_blocks=4, max_seqs=2, max_batched_tokens=64)
    seqs = [list(range(3, 36)), [7, 8, 9, 10, 11]]
    for step in range(3):
        ids, lg = m.step([0, 1], seqs, step == 0, want_logits=True)
        rid, rlg = oracle_rows(om, seqs)
        check_rows(f"head_dim 64 with the balanced schedule selected, step {step}", ids, lg, rid, rlg, LOGITS_TOL)
        for s, t in zip(seqs, rid):
            s.append(int(t))
    assert m.counter("attn_balanced_launches") == 0
    m.close()
