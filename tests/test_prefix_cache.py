# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Prefix cache on CPU: the ops.kv_block_copy reference, PrefixIndex,
LlamaDecodeEngine.prefill_cached and the prefix_cache_blocks servers on
the tiny config.  A suffix prefill over copied KV rows runs the same
per-row math as a one-shot prefill_packed on the CPU, so every
comparison here is exact."""

import concurrent.futures

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaServer, SamplingParams)
from mlrun_amd.models.prefix_cache import PrefixIndex

BT = ops.KV_BLOCK_TOKENS


def _i32(values):
    return torch.tensor(values, dtype=torch.int32)


# ------------------------------------------------------------------- op

L, HKV, D, POOL_N, CACHE_B, SMAX = 2, 2, 128, 5, 3, 150


def block_copy_case(seed=0):
    """Pool [L, 5, Hkv, 32, D] and cache [L, 3, Hkv, 150, D] of distinct
    random bf16 values (K and V differ), as (pool_k, pool_v, cache_k,
    cache_v)."""
    gen = torch.Generator().manual_seed(seed)

    def rand(*shape):
        return torch.randn(*shape, generator=gen).to(torch.bfloat16)
    return (rand(L, POOL_N, HKV, BT, D), rand(L, POOL_N, HKV, BT, D),
            rand(L, CACHE_B, HKV, SMAX, D), rand(L, CACHE_B, HKV, SMAX, D))


# pool -> cache: (pool id, 0, slot, block).  Block 3 is the last whole
# one (rows 96..127); block 4 would cross Smax = 150; slot 3 and pool
# id 5 do not exist.
GATHER = [(0, 0, 1, 0), (4, 0, 2, 3), (2, 0, 0, 4), (1, 0, 3, 0),
          (3, 0, 0, 2), (5, 0, 1, 1)]
GATHER_DONE = [0, 1, 4]
# cache -> pool: (slot, block, pool id, 0)
SCATTER = [(2, 3, 0, 0), (0, 0, 4, 0), (1, 4, 1, 0), (-1, 0, 2, 0),
           (1, 1, 3, 0), (0, 0, 2, 1)]
SCATTER_DONE = [0, 1, 4]


def expected_copy(src, dst, entries, done):
    """dst after the entries ``done`` of ``entries`` were copied, built
    with plain slicing."""
    want = dst.clone()
    for i in done:
        sr, sb, dr, db = entries[i]
        want[:, dr, :, db * BT:(db + 1) * BT] = \
            src[:, sr, :, sb * BT:(sb + 1) * BT]
    return want


def run_block_copy(src_k, src_v, dst_k, dst_v, entries, device="cpu"):
    """kv_block_copy of ``entries`` on ``device``; returns the new
    (dst_k, dst_v) on the CPU and leaves the arguments unchanged."""
    rows = [_i32(column).to(device) for column in zip(*entries)]
    out_k, out_v = dst_k.clone().to(device), dst_v.clone().to(device)
    ops.kv_block_copy(src_k.to(device), src_v.to(device), out_k, out_v,
                      *rows)
    return out_k.cpu(), out_v.cpu()


class TestBlockCopyReference:
    def test_gather_and_scatter_touch_the_named_blocks_only(self):
        pool_k, pool_v, cache_k, cache_v = block_copy_case()
        got_k, got_v = run_block_copy(pool_k, pool_v, cache_k, cache_v,
                                      GATHER)
        # every row outside the three named blocks keeps its old value
        assert torch.equal(got_k, expected_copy(pool_k, cache_k, GATHER,
                                                GATHER_DONE))
        assert torch.equal(got_v, expected_copy(pool_v, cache_v, GATHER,
                                                GATHER_DONE))
        assert torch.equal(got_k[:, 2, :, 96:128], pool_k[:, 4])
        assert torch.equal(got_k[:, :, :, 128:], cache_k[:, :, :, 128:])
        assert not torch.equal(got_k, cache_k)
        got_k, got_v = run_block_copy(cache_k, cache_v, pool_k, pool_v,
                                      SCATTER)
        assert torch.equal(got_k, expected_copy(cache_k, pool_k, SCATTER,
                                                SCATTER_DONE))
        assert torch.equal(got_v, expected_copy(cache_v, pool_v, SCATTER,
                                                SCATTER_DONE))
        assert torch.equal(got_v[:, 0], cache_v[:, 2, :, 96:128])
        assert torch.equal(got_k[:, 1], pool_k[:, 1])  # block 4: skipped
        assert torch.equal(got_k[:, 2], pool_k[:, 2])  # row -1, block 1

    def test_bad_arguments_raise(self):
        pool_k, pool_v, cache_k, cache_v = block_copy_case()
        idx = [_i32([0])] * 4

        def call(*tensors, index=idx):
            ops.kv_block_copy(*tensors, *index)
        with pytest.raises(ValueError, match="bf16"):
            call(pool_k.float(), pool_v, cache_k, cache_v)
        with pytest.raises(ValueError, match="dimensions"):
            call(pool_k, pool_v, cache_k[0], cache_v[0])
        with pytest.raises(ValueError, match="contiguous"):
            call(pool_k, pool_v, cache_k[:, :, :, ::2], cache_v)
        with pytest.raises(ValueError, match="equal shapes"):
            call(pool_k, pool_v[:, :4].contiguous(), cache_k, cache_v)
        with pytest.raises(ValueError, match="L, Hkv or D"):
            call(pool_k[:1].contiguous(), pool_v[:1].contiguous(),
                 cache_k, cache_v)
        with pytest.raises(ValueError, match="L, Hkv or D"):
            call(pool_k[..., :64].contiguous(),
                 pool_v[..., :64].contiguous(), cache_k, cache_v)
        with pytest.raises(ValueError, match="16 bytes"):
            call(*(t[..., :4].contiguous()
                   for t in (pool_k, pool_v, cache_k, cache_v)))
        with pytest.raises(ValueError, match="entries"):
            call(pool_k, pool_v, cache_k, cache_v,
                 index=[_i32([0]), _i32([0]), _i32([0, 1]), _i32([0])])
        with pytest.raises(ValueError, match="int32"):
            call(pool_k, pool_v, cache_k, cache_v,
                 index=[torch.tensor([0])] * 4)
        # nothing was written by the failed calls
        again = block_copy_case()
        for got, want in zip((pool_k, pool_v, cache_k, cache_v), again):
            assert torch.equal(got, want)


# ---------------------------------------------------------------- index


def toks(*blocks, tail=0):
    """A prompt of 32-token blocks, block b filled with b, plus ``tail``
    tokens of 999."""
    return [b for b in blocks for _ in range(BT)] + [999] * tail


class TestPrefixIndex:
    def test_longest_chain_and_the_cap(self):
        index = PrefixIndex(8)
        assert index.insert(toks(1, 2, 3, tail=5)) == \
            [(0, 0), (1, 1), (2, 2)]
        assert index.insert(toks(1, 2, 3, tail=5)) == []
        assert index.lookup(toks(1, 2, 3, 4, tail=1)) == [0, 1, 2]
        assert index.lookup(toks(1, 2, 7, tail=1)) == [0, 1]
        assert index.lookup(toks(9, 2, 3, tail=1)) == []
        # (len - 1) // 32 blocks at most: one token is always left
        for length, want in ((32, []), (33, [0]), (64, [0]), (65, [0, 1])):
            assert index.lookup(toks(1, 2, 3)[:length]) == want
        assert index.lookup([]) == []
        stats = index.stats()
        assert stats["lookups"] == 8 and stats["inserted"] == 3
        assert stats["hit_tokens"] == (3 + 2 + 0 + 0 + 1 + 1 + 2 + 0) * BT
        assert stats["prompt_tokens"] == 129 + 97 + 97 + 32 + 33 + 64 + 65
        assert stats["blocks_in_use"] == 3 and stats["capacity"] == 8

    def test_adapter_and_content_are_part_of_the_key(self):
        index = PrefixIndex(8)
        index.insert(toks(1, 2), adapter=0)
        assert index.lookup(toks(1, 2, tail=1), adapter=0) == [0, 1]
        assert index.lookup(toks(1, 2, tail=1), adapter=-1) == []
        assert index.lookup(toks(1, 2, tail=1), adapter=1) == []
        # an equal first block, then a different second one: one block
        assert index.lookup(toks(1, 5, tail=1), adapter=0) == [0]
        # an equal SECOND block under another first one is no hit
        assert index.lookup(toks(4, 2, tail=1), adapter=0) == []
        # one token off inside a block
        near = toks(1, 2, tail=1)
        near[40] += 1
        assert index.lookup(near, adapter=0) == [0]

    def test_lru_leaf_eviction_at_capacity_3(self):
        index = PrefixIndex(3)
        index.begin()
        assert index.insert(toks(1, 2)) == [(0, 0), (1, 1)]
        index.begin()
        assert index.insert(toks(3)) == [(0, 2)]
        index.begin()
        # full.  Block 0 is the oldest but has a child: the LRU LEAF
        # goes, which is block 1 (the chain 1,2 was touched before 3)
        assert index.insert(toks(4)) == [(0, 1)]
        assert index.stats()["evicted"] == 1
        assert index.stats()["blocks_in_use"] == 3
        # the recycled id 1 gives no false hit: chain (1, 2) ends at 1
        index.begin()
        assert index.lookup(toks(1, 2, tail=1)) == [0]
        assert index.lookup(toks(4, tail=1)) == [1]
        # ... and nothing under the old key's parent reaches it
        assert index.lookup(toks(1, 4, tail=1)) == [0]
        # now 3 (id 2) is the LRU leaf
        index.begin()
        assert index.insert(toks(5)) == [(0, 2)]
        assert index.lookup(toks(3, tail=1)) == []
        index.clear()
        assert index.stats()["blocks_in_use"] == 0
        assert index.lookup(toks(1, tail=1)) == []
        assert index.insert(toks(1)) == [(0, 0)]

    def test_blocks_of_the_current_call_are_not_evicted(self):
        index = PrefixIndex(3)
        index.begin()
        index.insert(toks(1))
        index.insert(toks(2))
        index.insert(toks(3))
        index.begin()
        assert index.lookup(toks(1, tail=1)) == [0]   # pins 0
        # 6 and 7 take the unpinned leaves 1 and 2; then everything is
        # pinned and the insert stops without a parentless child
        assert index.insert(toks(6, 7, 8)) == [(0, 1), (1, 2)]
        assert index.insert(toks(9)) == []
        assert index.lookup(toks(1, tail=1)) == [0]
        assert index.lookup(toks(6, 7, 8, tail=1)) == [1, 2]
        # the next call may evict them again, leaves first
        index.begin()
        assert index.insert(toks(9)) == [(0, 0)]
        assert index.insert(toks(10)) == [(0, 2)]
        assert index.lookup(toks(6, 7, tail=1)) == [1]

    def test_capacity_must_be_positive(self):
        with pytest.raises(ValueError, match="capacity"):
            PrefixIndex(0)


# --------------------------------------------------------------- engine

CFG = LlamaConfig.tiny()


def prompt(seed, length, shared=None):
    """``length`` random token ids; the first len(shared) are ``shared``."""
    gen = torch.Generator().manual_seed(seed)
    out = torch.randint(0, CFG.vocab_size, (length,), generator=gen).tolist()
    if shared:
        out[:len(shared)] = shared
    return out


SHARED = prompt(100, 70)
P1 = prompt(1, 90, SHARED)
P2 = prompt(2, 150, SHARED)


@pytest.fixture(scope="module")
def weights():
    return LlamaDecodeEngine(CFG, 1, device="cpu", use_graph=False).weights


def engine(weights, blocks=0, B=3, **kwargs):
    return LlamaDecodeEngine(CFG, B, device="cpu", use_graph=False,
                             weights=weights, prefix_cache_blocks=blocks,
                             **kwargs)


def decode(eng, slot, steps=8):
    out = []
    for _ in range(steps):
        eng.decode_step()
        out.append(int(eng.buf_tokens[slot]))
    return out


def assert_slot_equal(got, got_slot, want, want_slot, length):
    assert int(got.cache_lens[got_slot]) == length
    assert int(want.cache_lens[want_slot]) == length
    assert torch.equal(got.k_cache[:, got_slot, :, :length],
                       want.k_cache[:, want_slot, :, :length])
    assert torch.equal(got.v_cache[:, got_slot, :, :length],
                       want.v_cache[:, want_slot, :, :length])
    assert int(got.buf_tokens[got_slot]) == int(want.buf_tokens[want_slot])


class TestEngine:
    def test_flag_off_allocates_nothing(self, weights):
        eng = engine(weights)
        assert eng.prefix_index is None and eng.pc_k is None \
            and eng.pc_v is None
        with pytest.raises(ValueError, match="prefix_cache_blocks"):
            eng.prefill_cached([[1, 2]], [0])
        with pytest.raises(ValueError, match="prefix_cache_blocks"):
            eng.prefix_stats
        eng.clear_prefix_cache()  # a no-op

    def test_constructor_conflicts(self, weights):
        with pytest.raises(ValueError, match="prefix_cache_blocks.*fp8"):
            LlamaDecodeEngine(CFG, 2, device="cpu", kv_dtype="fp8",
                              prefix_cache_blocks=4)
        with pytest.raises(ValueError, match="prefix_cache_blocks.*tp_size"):
            LlamaDecodeEngine(CFG, 2, device="cpu", tp_size=2,
                              prefix_cache_blocks=4)
        with pytest.raises(ValueError, match="prefix_cache_blocks.*head_dim"):
            LlamaDecodeEngine(LlamaConfig.tiny(head_dim=64), 2,
                              device="cpu", prefix_cache_blocks=4)
        with pytest.raises(ValueError, match="negative"):
            engine(weights, blocks=-1)
        eng = engine(weights, blocks=8)
        assert eng.pc_k.shape == (CFG.num_layers, 8, CFG.num_kv_heads, BT,
                                  CFG.head_dim)
        assert eng.pc_v.shape == eng.pc_k.shape
        assert eng.pc_k.dtype == torch.bfloat16

    def test_hit_equals_cold_prefill(self, weights):
        cold = engine(weights)
        want = cold.prefill_packed([P2], [2])
        eng = engine(weights, blocks=8)
        eng.prefill_cached([P1], [0])
        assert eng.prefix_stats["hit_tokens"] == 0
        assert eng.prefix_stats["blocks_in_use"] == 2   # 90 // 32
        got = eng.prefill_cached([P2], [2])
        stats = eng.prefix_stats
        assert stats["hit_tokens"] == 64 and stats["lookups"] == 2
        assert stats["prompt_tokens"] == 90 + 150
        assert stats["blocks_in_use"] == 2 + 2          # 150 // 32 - 2 new
        assert torch.equal(got, want)
        assert_slot_equal(eng, 2, cold, 2, 150)
        # the pool holds the slot's rows, block by block
        for j, block in enumerate(eng.prefix_index.lookup(P2)):
            assert torch.equal(eng.pc_k[:, block],
                               eng.k_cache[:, 2, :, j * BT:(j + 1) * BT])
            assert torch.equal(eng.pc_v[:, block],
                               eng.v_cache[:, 2, :, j * BT:(j + 1) * BT])
        assert decode(eng, 2) == decode(cold, 2)
        # reset() leaves the cache alone
        eng.reset()
        assert eng.prefix_stats["blocks_in_use"] == 4
        eng.clear_prefix_cache()
        assert eng.prefix_stats["blocks_in_use"] == 0

    def test_mixed_group_and_slot_reuse(self, weights):
        eng = engine(weights, blocks=8)
        eng.prefill_cached([P2], [1])
        miss, one = prompt(3, 45), [17]
        group = [P1, miss, one]
        got = eng.prefill_cached(group, [0, 2, 1])
        assert eng.prefix_stats["hit_tokens"] == 64
        for i, (tokens, slot) in enumerate(zip(group, [0, 2, 1])):
            alone = engine(weights)
            want = alone.prefill_packed([tokens], [0])
            assert torch.equal(got[i], want[0])
            assert_slot_equal(eng, slot, alone, 0, len(tokens))
        # slot 1 held the 150 tokens of P2, then a 1-token prompt; now a
        # shorter cached prompt than P2 goes into slot 2's place
        short = P2[:100]
        logits = eng.prefill_cached([short], [2])
        assert eng.prefix_stats["hit_tokens"] == 64 + 96
        alone = engine(weights)
        assert torch.equal(logits, alone.prefill_packed([short], [0]))
        assert_slot_equal(eng, 2, alone, 0, 100)
        assert eng.cache_lens.tolist() == [90, 1, 100]
        assert decode(eng, 2, 3) == decode(alone, 0, 3)

    def test_pool_pressure_keeps_results_exact(self, weights):
        """3 pool blocks for prompts of 4 full blocks: inserts stop when
        every block is pinned, later calls evict, hits stay exact."""
        eng = engine(weights, blocks=3)
        eng.prefill_cached([P2], [0])
        assert eng.prefix_stats["blocks_in_use"] == 3
        other = prompt(4, 80)
        eng.prefill_cached([other], [1])
        assert eng.prefix_stats["evicted"] == 2
        got = eng.prefill_cached([P2], [2])
        assert eng.prefix_stats["hit_tokens"] == 32
        cold = engine(weights)
        assert torch.equal(got, cold.prefill_packed([P2], [2]))
        assert_slot_equal(eng, 2, cold, 2, 150)

    def test_adapters_key_the_cache(self, weights):
        gen = torch.Generator().manual_seed(5)

        def make_adapter(weights, r, gen):
            state = {"alpha": float(r)}
            for li, layer in enumerate(weights.layers):
                for proj in ("wqkv", "wo", "wgu", "wdown"):
                    n, k = layer[proj].shape
                    state[f"layers.{li}.{proj}.lora_A"] = (
                        torch.randn(r, k, generator=gen) * 0.05
                    ).to(torch.bfloat16)
                    state[f"layers.{li}.{proj}.lora_B"] = (
                        torch.randn(n, r, generator=gen) * 0.1
                    ).to(torch.bfloat16)
            return state

        eng = engine(weights, blocks=8, max_adapters=1, lora_rank=8)
        eng.load_adapter(0, make_adapter(weights, 8, gen))
        eng.prefill_cached([P1], [0], adapters=[0])
        assert eng.prefix_stats["blocks_in_use"] == 2
        # the same tokens under the base model do not hit
        got = eng.prefill_cached([P1], [1])
        assert eng.prefix_stats["hit_tokens"] == 0
        assert torch.equal(got, engine(weights).prefill_packed([P1], [0]))
        # ... and under the adapter they do, with the adapter's rows
        got = eng.prefill_cached([P2], [2], adapters=[0])
        assert eng.prefix_stats["hit_tokens"] == 64
        twin = engine(weights, lora=eng.lora)
        assert torch.equal(got, twin.prefill_packed([P2], [2], adapters=[0]))
        assert_slot_equal(eng, 2, twin, 2, 150)
        assert eng.buf_adapter.tolist() == [0, -1, 0]
        # a new adapter in the slot makes its cached rows stale
        eng.load_adapter(0, make_adapter(weights, 8, gen))
        assert eng.prefix_stats["blocks_in_use"] == 0
        eng.prefill_cached([P1], [0], adapters=[0])
        assert eng.prefix_stats["hit_tokens"] == 64
        eng.unload_adapter(0)
        assert eng.prefix_stats["blocks_in_use"] == 0
        with pytest.raises(ValueError, match="adapter id"):
            eng.prefill_cached([P1], [0], adapters=[1])

    def test_logit_processors_count_the_cached_tokens(self, weights):
        """A cache hit is a fresh request: its cached tokens are in the
        prompt for the penalties.  Greedy tokens under a repetition
        penalty and their logprobs match an engine without the cache."""
        params = SamplingParams(repetition_penalty=1.8)
        plain = engine(weights, sampling="request", logit_processors=True)
        plain.set_sampling_slots([2], [params])
        plain.prefill_packed([P2], [2])
        eng = engine(weights, blocks=8, sampling="request",
                     logit_processors=True)
        eng.prefill_cached([P1], [0])
        eng.set_sampling_slots([2], [params])
        eng.prefill_cached([P2], [2])
        assert eng.prefix_stats["hit_tokens"] == 64
        assert torch.equal(eng.buf_tok_state[2], plain.buf_tok_state[2])
        # every distinct token of the WHOLE prompt has its in-prompt bit
        assert int(eng.buf_tok_state[2].sum()) == len(set(P2)) \
            > len(set(P2[64:]))
        assert int(eng.buf_tokens[2]) == int(plain.buf_tokens[2])
        assert float(eng.buf_logprob[2]) == float(plain.buf_logprob[2])
        for _ in range(8):
            eng.decode_step()
            plain.decode_step()
            assert int(eng.buf_tokens[2]) == int(plain.buf_tokens[2])
            assert float(eng.buf_logprob[2]) == float(plain.buf_logprob[2])

    def test_failed_call_changes_nothing(self, weights):
        eng = engine(weights, blocks=8)
        eng.prefill_cached([P1], [0])
        before = eng.prefix_stats
        pool = eng.pc_k.clone()
        bad = P2[:140] + [CFG.vocab_size]
        for args in (([P2, bad], [1, 2]), ([P2, []], [1, 2]),
                     ([P2], [3]), ([P2, P1], [1, 1]),
                     ([P2 + P2], [1])):
            with pytest.raises(ValueError):
                eng.prefill_cached(*args)
        assert eng.prefix_stats == before
        assert torch.equal(eng.pc_k, pool)
        assert eng.cache_lens.tolist() == [90, 0, 0]


# --------------------------------------------------------------- server


class _Ev:
    id = "ev"
    path = ""

    def __init__(self, inputs, max_tokens, **extra):
        self.body = {"inputs": inputs, "max_tokens": max_tokens, **extra}


def ask(server, prompts, max_tokens=5, **fields):
    return server.do_event(_Ev(prompts, max_tokens, **fields)).body


def make_server(**kwargs):
    server = LlamaServer(name="s", config=LlamaConfig.tiny(), batch_size=4,
                         max_new_tokens=5, use_graph=False, device="cpu",
                         **kwargs)
    server.load()
    return server


DOC = prompt(200, 96)
Q1 = prompt(201, 110, DOC)
Q2 = prompt(202, 103, DOC)

# sampling="request" servers prefill through the packed pass with the
# flag off too, so the two servers run the same attention code and the
# outputs can be compared exactly (the dense prefill of a
# sampling="engine" server agrees with it within a bound only)
SERVER_MODES = {
    "batch": dict(sampling="request"),
    "continuous": dict(sampling="request", scheduling="continuous"),
    "continuous-packed-engine": dict(scheduling="continuous",
                                     prefill="packed"),
}


class TestServer:
    @pytest.mark.parametrize("mode", list(SERVER_MODES))
    def test_outputs_equal_a_server_without_the_flag(self, mode):
        kwargs = SERVER_MODES[mode]
        fields = dict(seed=11, temperature=0.7, logprobs=True) \
            if "sampling" in kwargs else {}
        plain = make_server(**kwargs)
        try:
            assert plain.stats() == ({"sampling": {
                "requests": 0, "sampled": 0, "greedy": 0}}
                if "sampling" in kwargs else {})
            want = [ask(plain, [q], **fields) for q in (Q1, Q2)]
            assert "prefix_cache" not in plain.stats()
        finally:
            plain.shutdown()
        server = make_server(prefix_cache_blocks=8, **kwargs)
        try:
            got = [ask(server, [q], **fields) for q in (Q1, Q2)]
            assert got == want
            assert len(got[0]["outputs"][0]) == 5
            stats = server.stats()
            assert stats["prefix_cache"] == {
                "requests": 2, "prompt_tokens": 110 + 103,
                "hit_tokens": 96, "blocks": 3, "capacity": 8,
                "evictions": 0}
            assert ("sampling" in stats) == ("sampling" in kwargs)
        finally:
            server.shutdown()

    def test_combinations(self):
        """Logit processors, a two-prompt request and concurrent clients
        on the continuous server; the batcher on the batch server."""
        plain = make_server(sampling="request", logit_processors=True,
                            scheduling="continuous")
        server = make_server(sampling="request", logit_processors=True,
                             scheduling="continuous", prefix_cache_blocks=8)
        try:
            fields = dict(repetition_penalty=1.8, seed=3, logprobs=True)
            want = ask(plain, [Q1, Q2], **fields)
            ask(server, [DOC + [5]])
            assert ask(server, [Q1, Q2], **fields) == want
            assert server.stats()["prefix_cache"]["hit_tokens"] == 2 * 96
            with concurrent.futures.ThreadPoolExecutor(3) as pool:
                futures = [pool.submit(ask, server, [q], **fields)
                           for q in (Q1, Q2, Q1)]
                rows = [f.result(timeout=120) for f in futures]
            assert rows[0]["outputs"] == [want["outputs"][0]]
            assert rows[2] == rows[0]
        finally:
            plain.shutdown()
            server.shutdown()
        batcher = make_server(sampling="request", batch_window_ms=20,
                              prefix_cache_blocks=8)
        try:
            first = ask(batcher, [Q1], seed=3)
            with concurrent.futures.ThreadPoolExecutor(2) as pool:
                futures = [pool.submit(ask, batcher, [q], seed=3)
                           for q in (Q1, Q2)]
                rows = [f.result(timeout=120) for f in futures]
            assert rows[0] == first
            assert batcher.stats()["prefix_cache"]["hit_tokens"] >= 96
        finally:
            batcher.shutdown()

    def test_constructor_errors(self):
        with pytest.raises(ValueError, match="prefix_cache_blocks.*fp8"):
            LlamaServer(name="s", config=LlamaConfig.tiny(),
                        kv_dtype="fp8", prefix_cache_blocks=8)
        with pytest.raises(ValueError,
                           match="prefix_cache_blocks.*speculative"):
            LlamaServer(name="s", config=LlamaConfig.tiny(),
                        speculative=2, prefix_cache_blocks=8)
        with pytest.raises(ValueError, match="negative"):
            LlamaServer(name="s", config=LlamaConfig.tiny(),
                        prefix_cache_blocks=-1)

    def test_failed_admission_inserts_nothing(self):
        server = make_server(scheduling="continuous", prefix_cache_blocks=8)
        try:
            bad = DOC + [CFG.vocab_size]
            with pytest.raises(ValueError, match="token id"):
                ask(server, [bad])
            stats = server.stats()["prefix_cache"]
            assert stats["blocks"] == 0 and stats["requests"] == 0
            # the server still serves, and the good prefix goes in
            assert len(ask(server, [Q1])["outputs"][0]) == 5
            assert server.stats()["prefix_cache"]["blocks"] == 3
        finally:
            server.shutdown()
