"""GPU: the sampled decode fast path (nvllm_decode_next_sample / nvllm_decode_enqueue_sample: the draw in the LM head's epilogue)
against the slow path it must reproduce id for id -- nvllm_step_sample on full token lists, itself held to the host mirror of
the draw (engine.sample_token_host) applied to the logits it returns."""
import itertools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TEMPS = [0.0, 0.6, 1.0, 5.0]
SEEDS = (0, 2**63 + 5)
K = 6


@pytest.fixture(scope="module")
def pkg():
    import nano_vllm_candle_amd as p

    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    from nano_vllm_candle_amd import layers

    return layers.default_context()


def _prompts(cfg, n):
    rng = np.random.default_rng(n)
    return [rng.integers(3, cfg.vocab_size, int(k)).tolist() for k in rng.integers(2, 13, n)]


def _temps(n):
    return [TEMPS[i % len(TEMPS)] for i in range(n)]


def slow(m, sids, prompts, temps, seed, greedy_at=()):
    """K + 1 steps of step_sample (step k in greedy_at: the greedy step); every sampled id is the mirror's draw from the returned logits"""
    from nano_vllm_candle_amd.engine import sample_key, sample_token_host

    my, out = [list(p) for p in prompts], []
    for k in range(K + 1):
        if k in greedy_at:
            ids, _ = m.step(sids, my, False)
        else:
            ids, lg = m.step_sample(sids, my, k == 0, temps, seed, want_logits=True)
            assert ids.tolist() == [sample_token_host(lg[i], temps[i], sample_key(seed, sids[i], len(my[i]))) for i in range(len(my))], k
            for i, t in enumerate(temps):
                if t == 0.0 and np.isfinite(lg[i]).all():  # the clamp 1e-6 makes the draw the arg-max (last max)
                    assert int(ids[i]) == int(np.flatnonzero(lg[i] == lg[i].max())[-1])
        out.append(ids.tolist())
        for s, t in zip(my, ids):
            s.append(int(t))
    return out


def fast(m, sids, prompts, temps, seed, greedy_at=(), pipelined=False):
    n = len(sids)
    out = [m.step_sample(sids, prompts, True, temps, seed)[0].tolist()]
    if pipelined:
        for k in range(0, K, 3):
            for _ in range(3):
                m.decode_enqueue_sample(temps, seed)
            out += [m.decode_collect()[:n].tolist() for _ in range(3)]
        return out
    for k in range(1, K + 1):
        out.append((m.decode_next() if k in greedy_at else m.decode_next_sample(temps, seed))[:n].tolist())
    return out


def make(pkg, ctx, kw, n):
    m = pkg.Qwen3ForCausalLM.from_synthetic(pkg.Qwen3Config.tiny(**kw), 9, ctx)
    m.kv_alloc(n + 2, n, 256)
    return m


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kw,n", [
    (dict(), 5),                                        # hidden 128: the chunked kernel, ticketed finish
    (dict(hidden_size=256), 5),                         # streaming kernel, 1 / 2 / 4 row blocks, the last one partly filled
    (dict(hidden_size=256), 17),
    (dict(hidden_size=256), 40),
    (dict(hidden_size=256), 65),                        # > 64 rows: the chunked kernel again
    (dict(hidden_size=256, vocab_size=528), 3),         # 33 n-tiles: idle waves in the last workgroup (partials with index -1)
    (dict(hidden_size=256, vocab_size=40000), 3),       # 2 500 n-tiles: two per wave, 1 250 waves, a partial last workgroup
])
def test_fast_path_draws_what_step_sample_draws(pkg, ctx, kw, n, seed):
    m = make(pkg, ctx, kw, n)
    sids, prompts, temps = list(range(50, 50 + n)), _prompts(m.cfg, n), _temps(n)
    assert fast(m, sids, prompts, temps, seed) == slow(m, sids, prompts, temps, seed)


def test_pipelined_mixed_and_reseeded(pkg, ctx):
    m = make(pkg, ctx, dict(hidden_size=256), 5)
    sids, prompts, temps = [7, 8, 9, 10, 11], _prompts(m.cfg, 5), _temps(5)
    want = slow(m, sids, prompts, temps, 3)
    assert fast(m, sids, prompts, temps, 3, pipelined=True) == want
    # a greedy fast step between sampled ones == the slow path on the same schedule
    assert fast(m, sids, prompts, temps, 3, greedy_at=(2, 5)) == slow(m, sids, prompts, temps, 3, greedy_at=(2, 5))
    # another seed: the temperature-5 row (index 3) draws something else somewhere; new temperatures are taken up too
    other = fast(m, sids, prompts, temps, 4)
    assert [r[3] for r in other] != [r[3] for r in want]
    cold = [0.0] * 5
    assert fast(m, sids, prompts, cold, 3) == slow(m, sids, prompts, cold, 3)
    with pytest.raises(pkg._lib.NvllmError) as e:
        pkg._lib.check(pkg._lib.lib().nvllm_decode_next_sample(m.h, None, 0, None), m.ctx.h)
    assert e.value.code == pkg._lib.EINVAL


def test_vocab_parallel_shards_share_the_random_stream(pkg):
    cfg, tp, seed = pkg.Qwen3Config.tiny(hidden_size=256), 2, SEEDS[1]
    sids, prompts, temps = [0, 1, 2, 3, 4], _prompts(cfg, 5), _temps(5)
    res, errors = [None] * tp, []

    def worker(rank):
        try:
            c = pkg.Context(0, tp_rank=rank, tp_size=tp, loopback_group="gsampled")
            m = pkg.Qwen3ForCausalLM.from_synthetic(cfg, seed=4, ctx=c)
            m.kv_alloc(8, 5, 64)
            res[rank] = (slow(m, sids, prompts, temps, seed), fast(m, sids, prompts, temps, seed))
            m.close()
            c.close()
        except BaseException as e:  # noqa: BLE001
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(tp)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    assert not errors, errors
    assert all(r is not None for r in res), "a rank hung"
    assert res[0][0] == res[0][1] == res[1][0] == res[1][1]


def test_non_finite_logits_take_the_plain_winner(pkg, ctx):
    # lm_head row 7 = +inf: logit 7 is +-inf or NaN, the row has no distribution; the expected ids are still the mirror's
    cfg = pkg.Qwen3Config.tiny(hidden_size=256)
    rng = np.random.default_rng(1)
    tensors = {name: (1.0 + 0.1 * rng.standard_normal(s) if name.endswith("norm.weight") else 0.05 * rng.standard_normal(s)).astype(np.float32)
               for name, s in cfg.hf_tensor_shapes().items()}
    tensors["lm_head.weight"][7] = np.inf
    m = pkg.Qwen3ForCausalLM.from_state_dict(cfg, tensors, ctx)
    m.kv_alloc(8, 5, 64)
    sids, prompts, temps = [0, 1, 2, 3, 4], _prompts(cfg, 5), _temps(5)
    assert fast(m, sids, prompts, temps, 0) == slow(m, sids, prompts, temps, 0)


def test_engine_fast_decode_returns_the_same_tokens(pkg, ctx):
    import nano_vllm_candle_amd.engine as E

    m = make(pkg, ctx, dict(hidden_size=256), 8)
    prompts = _prompts(m.cfg, 5)
    calls = []
    real = m.decode_next_sample
    m.decode_next_sample = lambda *a, **k: calls.append(1) or real(*a, **k)

    def gen(fast_decode):
        E._SEQ_COUNTER = itertools.count(7000)  # the draw is keyed by (seed, seq_id, position)
        eng = E.LLMEngine(E.Scheduler(E.SchedulerConfig(max_num_seqs=3, eos=m.cfg.eos_token_id)),
                          E.Qwen3ModelRunner(m, seed=5, raise_errors=True, fast_decode=fast_decode))
        return eng.generate(prompts, E.SamplingParams(temperature=1.5, max_tokens=8, ignore_eos=True))

    want = gen(False)
    assert not calls
    assert gen(True) == want and calls
