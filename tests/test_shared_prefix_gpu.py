"""GPU: sequences forked over shared K/V blocks (Qwen3ForCausalLM.seq_fork) and the shared-prefix decode attention schedule
(attn_shared_kernel<128, VLO> behind its host-built plan), against the oracle's dense re-forward of every sequence."""
import numpy as np
import pytest

from tests.test_operating_point_gpu import check_rows, oracle_rows
from tests.util import LOGITS_TOL, oracle_config

pytestmark = pytest.mark.gpu

# (prompt tokens, forks).  603 + 9: blocks 0-1 shared, ten members exceed one sub-tile at gqa 2, 603 + 8 steps crosses the tile
# edge at 608; 765 + 2 crosses the block edge at 768 while decoding; 513: last cached token 512, blocks 0 and 1 shared;
# 512: block 1 private, block 0 shared; 300: in no family
FAMILIES = ((603, 9), (765, 2), (513, 1), (512, 1), (300, 0))
N_SEQS = sum(1 + f for _, f in FAMILIES)
N_STEPS = 7  # after the prefill and the forks: 3 x step, 2 x decode_next, 2 x decode_enqueue / collect
LAYOUTS = [(4, 2, 16, 16), (8, 1, 16, 16), (10, 2, 16, 16), (4, 2, 16, 24), (4, 2, 24, 24)]


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


def forked_batch(om, cfg, families):
    """(parent ids, prompts, (src, dst) forks, every sequence's token list for the first step after the fork): the parent is
    fed the oracle's token, fork j of it a different one each, so no two rows of a slab are equal"""
    rng = np.random.default_rng(11)
    prompts = [rng.integers(0, cfg.vocab_size, n).tolist() for n, _ in families]
    first = oracle_rows(om, prompts)
    parents, forks, seqs, sid = [], [], [], 0
    for p, t, (_, nf) in zip(prompts, first[0], families):
        parents.append(sid)
        forks += [(sid, sid + 1 + j) for j in range(nf)]
        seqs += [p + [(int(t) + j) % cfg.vocab_size] for j in range(nf + 1)]
        sid += nf + 1
    return parents, prompts, forks, seqs, first


@pytest.fixture(scope="module")
def reference(pkg, oracle):
    """(config, oracle model, batch, [(token lists, greedy ids, logits) per step]) per head layout, computed once"""
    cache = {}

    def get(nh, kv):
        if (nh, kv) not in cache:
            cfg = tiny(pkg, nh, kv)
            om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(7)
            batch = forked_batch(om, cfg, FAMILIES)
            seqs = [list(s) for s in batch[3]]
            steps = []
            for _ in range(N_STEPS):
                rid, rlg = oracle_rows(om, seqs)
                steps.append(([list(s) for s in seqs], rid, rlg))
                for s, t in zip(seqs, rid):
                    s.append(int(t))
            cache[nh, kv] = cfg, om, batch, steps
        return cache[nh, kv]

    return get


def start(pkg, ctx, cfg, batch, k_bits, v_bits, schedule, num_blocks=40):
    """prefill the parents and fork them; the free-block count falls by each fork's private tail only"""
    parents, prompts, forks, _, first = batch
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 7, ctx)
    m.set_kv_cache_bits(k_bits, v_bits)
    m.set_attention_schedule(schedule)
    m.kv_alloc(num_blocks=num_blocks, max_seqs=N_SEQS, max_batched_tokens=1024)
    ids, lg = m.step(parents, prompts, True, want_logits=True)
    check_rows(f"{schedule} K{k_bits}/V{v_bits} prefill of the parents", ids, lg, first[0], first[1], LOGITS_TOL)
    for src, dst in forks:
        n = len(prompts[parents.index(src)])
        before = m.free_blocks()
        m.seq_fork(src, dst)
        assert before - m.free_blocks() == -(-n // 256) - (n - 1) // 256, (src, dst)
    return m


def drive(pkg, ctx, ref, k_bits, v_bits, schedule="shared_prefix"):
    """the whole call sequence on a fresh pool; returns (model, the step() logits, every step's ids, the GPU's token lists)"""
    cfg, _, batch, steps = ref
    m = start(pkg, ctx, cfg, batch, k_bits, v_bits, schedule)
    sids, L = list(range(N_SEQS)), cfg.num_hidden_layers
    shared = schedule == "shared_prefix"
    logits, all_ids = [], []
    for k in range(3):  # the caller feeds the oracle's tokens: every step is comparable on its own
        ids, lg = m.step(sids, steps[k][0], False, want_logits=True)
        check_rows(f"{schedule} K{k_bits}/V{v_bits} step {k}", ids, lg, steps[k][1], steps[k][2], LOGITS_TOL)
        assert m.counter("attn_shared_launches") == (L * (k + 1) if shared else 0)
        logits.append(lg)
        all_ids.append(np.array(ids))
    live = [list(s) for s in steps[3][0]]
    same = np.ones(N_SEQS, bool)  # rows that have followed the oracle's tokens so far (a near-tie may part them)

    def resident(k, got):
        srt = np.sort(steps[k][2], axis=1)
        clear = (srt[:, -1] - srt[:, -2]) / np.abs(steps[k][2]).max(axis=1) > 2 * LOGITS_TOL
        assert (got == steps[k][1])[same & clear].all(), (k, got, steps[k][1])
        same[:] &= got == steps[k][1]
        for s, t in zip(live, got):
            s.append(int(t))
        all_ids.append(got)

    for k in (3, 4):  # positions advance on the device; the plan does not move
        resident(k, np.array(m.decode_next()[:N_SEQS]))
    m.decode_enqueue()
    m.decode_enqueue()
    for k in (5, 6):
        resident(k, np.array(m.decode_collect()[:N_SEQS]))
    assert m.counter("attn_shared_launches") == (L * 7 if shared else 0)
    return m, logits, all_ids, live


@pytest.mark.parametrize("nh,kv,k_bits,v_bits", LAYOUTS)
def test_families_vs_oracle(pkg, ctx, reference, nh, kv, k_bits, v_bits):
    drive(pkg, ctx, reference(nh, kv), k_bits, v_bits)[0].close()


def test_forks_under_the_default_schedule(pkg, ctx, reference):
    drive(pkg, ctx, reference(4, 2), 16, 16, "per_sequence")[0].close()  # the pool alone: every kernel reads block tables


def test_replay_is_bit_equal_and_references_keep_blocks_alive(pkg, ctx, reference):
    ref = reference(4, 2)
    m1, lg1, ids1, _ = drive(pkg, ctx, ref, 16, 16)
    m1.close()
    m2, lg2, ids2, live = drive(pkg, ctx, ref, 16, 16)
    for a, b in zip(lg1 + ids1, lg2 + ids2):  # merged in a fixed order, not in arrival order
        assert np.array_equal(a, b)
    m2.seq_free(0)  # the parent of nine forks: its shared blocks stay, its tail returns
    sids = list(range(1, N_SEQS))
    ids, lg = m2.step(sids, live[1:], False, want_logits=True)
    rid, rlg = oracle_rows(ref[1], live[1:])
    check_rows("shared_prefix, after freeing a parent", ids, lg, rid, rlg, LOGITS_TOL)
    m2.close()


def test_pool_books_and_errors(pkg, ctx, reference):
    cfg, _, batch, steps = reference(4, 2)
    E = pkg._lib
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 7, ctx)
    with pytest.raises(E.NvllmError) as e:
        m.seq_fork(0, 1)
    assert e.value.code == E.ESTATE  # before kv_alloc
    m.close()
    used = sum(-(-n // 256) + f * (-(-n // 256) - (n - 1) // 256) for n, f in FAMILIES)
    m = start(pkg, ctx, cfg, batch, 16, 16, "shared_prefix", num_blocks=used)  # checks every fork's private tail
    assert m.free_blocks() == 0

    def refused(code, *args):
        free = m.free_blocks()
        with pytest.raises(E.NvllmError) as e:
            m.seq_fork(*args)
        assert e.value.code == code and m.free_blocks() == free, (args, e.value.code)

    refused(E.EINVAL, 999, 1000)  # unknown source
    refused(E.EINVAL, 0, 1)       # destination already live
    m.seq_free(N_SEQS - 1)        # the 300-token sequence: a slot and two blocks
    m.seq_fork(10, N_SEQS - 1)    # 765 tokens: one private block
    refused(E.ENOMEM, 0, 1000)    # no free slot
    m.seq_free(N_SEQS - 1)
    m.seq_free(N_SEQS - 2)        # the fork of the 512-token parent: its one private block
    assert m.free_blocks() == 3
    m.step([1], [steps[0][0][1][:600]], True)  # re-prefill of a fork gives back only its own tail and takes three blocks
    assert m.free_blocks() == 1
    m.seq_fork(10, 1000)        # the last free block
    refused(E.ENOMEM, 1, 1001)  # a free slot, but no block for the tail
    m.decode_enqueue()
    refused(E.ESTATE, 0, 1001)  # an enqueued step is not collected
    m.decode_collect()
    for s in list(range(N_SEQS)) + [1000]:
        m.seq_free(s)
    assert m.free_blocks() == used
    m.close()


@pytest.mark.parametrize("hd,n", [(128, 100), (64, 603)])  # no whole shared block; a head_dim the kernel does not serve
def test_fallbacks_keep_the_default_launch(pkg, ctx, oracle, hd, n):
    cfg = tiny(pkg, 4, 2, hd=hd)
    om = oracle.Model(oracle_config(oracle, cfg)).fill_synthetic(7)
    families = ((n, 2), (40, 0))
    batch = forked_batch(om, cfg, families)
    m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, 7, ctx)
    m.set_attention_schedule("shared_prefix")
    m.kv_alloc(num_blocks=12, max_seqs=4, max_batched_tokens=1024)
    m.step(batch[0], batch[1], True)
    for src, dst in batch[2]:
        m.seq_fork(src, dst)
    seqs = batch[3]
    for step in range(3):
        ids, lg = m.step([0, 1, 2, 3], seqs, False, want_logits=True)
        rid, rlg = oracle_rows(om, seqs)
        check_rows(f"head_dim {hd}, {n}-token parent, step {step}", ids, lg, rid, rlg, LOGITS_TOL)
        for s, t in zip(seqs, rid):
            s.append(int(t))
    assert m.counter("attn_shared_launches") == 0
    m.close()
