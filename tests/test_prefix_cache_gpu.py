# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Prefix cache on MI355X: the kv_block_copy HIP kernel against its CPU
path (a copy: bit-equal), prefill_cached on a cuda engine against a cold
prefill_packed, and the continuous server with the flag on."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaServer)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# the project's bound for "same prefill, different reduction order"
# (tests/test_prefill_packed_gpu.py): a warm call runs its library GEMMs
# over fewer rows than a cold one, which may round a row differently
PREFILL_MAX_ERR = 0.25

BT = ops.KV_BLOCK_TOKENS
L, HKV, D, POOL_N, CACHE_B, SMAX = 2, 2, 128, 5, 3, 150


def _i32(values):
    return torch.tensor(values, dtype=torch.int32)


def _case(seed):
    gen = torch.Generator().manual_seed(seed)

    def rand(*shape):
        return torch.randn(*shape, generator=gen).to(torch.bfloat16)
    return (rand(L, POOL_N, HKV, BT, D), rand(L, POOL_N, HKV, BT, D),
            rand(L, CACHE_B, HKV, SMAX, D), rand(L, CACHE_B, HKV, SMAX, D))


def _both(src_k, src_v, dst_k, dst_v, entries):
    """kv_block_copy on the CPU and on the GPU over the same inputs;
    returns ((k, v) reference, (k, v) kernel result on the CPU)."""
    rows = [_i32(column) for column in zip(*entries)]
    ref_k, ref_v = dst_k.clone(), dst_v.clone()
    ops.kv_block_copy(src_k, src_v, ref_k, ref_v, *rows)
    got_k, got_v = dst_k.cuda(), dst_v.cuda()
    ops.kv_block_copy(src_k.cuda(), src_v.cuda(), got_k, got_v,
                      *(r.cuda() for r in rows))
    torch.cuda.synchronize()
    return (ref_k, ref_v), (got_k.cpu(), got_v.cpu())


def _bits(t):
    return t.view(torch.int16)


@requires_gpu
class TestBlockCopyKernel:
    def test_gather_matches_cpu_path(self):
        """Pool -> cache, 6 entries: the last whole block (rows
        96..127) is copied, block 4 (past Smax = 150) and slot 3 (out of
        range) are skipped."""
        pool_k, pool_v, cache_k, cache_v = _case(0)
        entries = [(0, 0, 1, 0), (4, 0, 2, 3), (2, 0, 0, 4), (1, 0, 3, 0),
                   (3, 0, 0, 2), (2, 0, 1, 1)]
        ref, got = _both(pool_k, pool_v, cache_k, cache_v, entries)
        for r, g, before, pool in zip(ref, got, (cache_k, cache_v),
                                      (pool_k, pool_v)):
            assert torch.equal(_bits(g), _bits(r))
            assert torch.equal(g[:, 2, :, 96:128], pool[:, 4])
            # untouched: rows past the last whole block, skipped entries
            assert torch.equal(g[:, :, :, 128:], before[:, :, :, 128:])
            assert torch.equal(g[:, 0, :, :64], before[:, 0, :, :64])
            changed = (g != before).any(-1).any(-1).any(0)  # [B, Hkv]
            assert changed.all()  # every slot and head got a block

    def test_scatter_matches_cpu_path(self):
        """Cache -> pool, 6 entries, 2 skipped (source block 4 would
        cross Smax; source row -1)."""
        pool_k, pool_v, cache_k, cache_v = _case(1)
        entries = [(2, 3, 0, 0), (0, 0, 4, 0), (1, 4, 1, 0), (-1, 0, 2, 0),
                   (1, 1, 3, 0), (0, 2, 2, 0)]
        ref, got = _both(cache_k, cache_v, pool_k, pool_v, entries)
        for r, g, before, cache in zip(ref, got, (pool_k, pool_v),
                                       (cache_k, cache_v)):
            assert torch.equal(_bits(g), _bits(r))
            assert torch.equal(g[:, 0], cache[:, 2, :, 96:128])
            assert torch.equal(g[:, 2], cache[:, 0, :, 64:96])
            assert torch.equal(g[:, 1], before[:, 1])  # skipped

    def test_unaligned_single_entry(self):
        """n = 1, cache -> cache with all four indices different: rows
        32..63 of slot 2 go to rows 96..127 of row 1 of a second cache
        of another Smax; every other row keeps its sentinel."""
        _, _, src_k, src_v = _case(2)
        dst_k = torch.full((L, 2, HKV, 130, D), -7.0, dtype=torch.bfloat16)
        dst_v = torch.full((L, 2, HKV, 130, D), 9.0, dtype=torch.bfloat16)
        ref, got = _both(src_k, src_v, dst_k, dst_v, [(2, 1, 1, 3)])
        for r, g, src, fill in zip(ref, got, (src_k, src_v), (-7.0, 9.0)):
            assert torch.equal(_bits(g), _bits(r))
            assert torch.equal(g[:, 1, :, 96:128], src[:, 2, :, 32:64])
            assert (g[:, 0] == fill).all()
            assert (g[:, 1, :, :96] == fill).all()
            assert (g[:, 1, :, 128:] == fill).all()

    def test_bad_arguments_raise_before_launch(self):
        pool_k, pool_v, cache_k, cache_v = (t.cuda() for t in _case(3))
        idx = [_i32([0]).cuda()] * 4
        with pytest.raises(ValueError, match="bf16"):
            ops.kv_block_copy(pool_k.float(), pool_v, cache_k, cache_v, *idx)
        with pytest.raises(ValueError, match="is on"):
            ops.kv_block_copy(pool_k, pool_v, cache_k, cache_v.cpu(), *idx)
        with pytest.raises(ValueError, match="is on"):
            ops.kv_block_copy(pool_k, pool_v, cache_k, cache_v,
                              idx[0].cpu(), *idx[1:])


@requires_gpu
class TestEnginePrefillCachedGpu:
    def test_warm_call_matches_cold_prefill_and_decodes(self):
        cfg = LlamaConfig.tiny()
        eng = LlamaDecodeEngine(cfg, 3, device="cuda:0", use_graph=True,
                                prefix_cache_blocks=8)
        cold = LlamaDecodeEngine(cfg, 3, device="cuda:0", use_graph=True,
                                 weights=eng.weights)
        assert cold.pc_k is None and cold.prefix_index is None
        gen = torch.Generator().manual_seed(71)
        shared = torch.randint(0, cfg.vocab_size, (70,),
                               generator=gen).tolist()
        p1 = shared + torch.randint(0, cfg.vocab_size, (20,),
                                    generator=gen).tolist()
        p2 = shared + torch.randint(0, cfg.vocab_size, (80,),
                                    generator=gen).tolist()
        eng.prefill_cached([p1], [0])
        got = eng.prefill_cached([p2], [2])
        want = cold.prefill_packed([p2], [2])
        torch.cuda.synchronize()
        stats = eng.prefix_stats
        assert stats["hit_tokens"] == 64 and stats["blocks_in_use"] == 4
        assert got.shape == (1, cfg.vocab_size)
        assert torch.isfinite(got.float()).all()
        err = (got.float() - want.float()).abs().max().item()
        assert err < PREFILL_MAX_ERR, err
        assert eng.cache_lens.tolist() == [90, 0, 150]
        # the gathered rows are the pool's blocks, bit for bit; those
        # blocks came from slot 0, where p1 was prefilled
        chain = eng.prefix_index.lookup(p2)
        assert len(chain) == 4
        for j, block in enumerate(chain):
            rows = slice(j * BT, (j + 1) * BT)
            for pool, cache in ((eng.pc_k, eng.k_cache),
                                (eng.pc_v, eng.v_cache)):
                assert torch.equal(_bits(cache[:, 2, :, rows]),
                                   _bits(pool[:, block]))
                if j < 2:
                    assert torch.equal(_bits(cache[:, 0, :, rows]),
                                       _bits(pool[:, block]))
        eng.capture_graph()
        for _ in range(4):
            eng.decode_step()
        torch.cuda.synchronize()
        assert eng.cache_lens.tolist() == [94, 4, 154]
        assert 0 <= int(eng.buf_tokens[2]) < cfg.vocab_size


class _Ev:
    id = "ev"
    path = ""

    def __init__(self, inputs, max_tokens):
        self.body = {"inputs": inputs, "max_tokens": max_tokens}


@requires_gpu
class TestServerGpu:
    def test_continuous_server_hits_on_the_second_wave(self):
        """Two waves of three prompts behind one 64-token prefix.  The
        second wave hits 3 x 64 tokens.  The first hits nothing when the
        scheduler admits its prompts as one group (no de-duplication
        inside a group); should the worker wake between two of the
        queue puts, the later group already hits, so the first wave's
        count is one of 0, 64, 128 and the second wave is counted from
        there."""
        cfg = LlamaConfig.tiny()
        server = LlamaServer(name="s", config=cfg, batch_size=4,
                             max_new_tokens=4, device="cuda:0",
                             scheduling="continuous", prefix_cache_blocks=16)
        server.load()
        try:
            gen = torch.Generator().manual_seed(72)
            shared = torch.randint(0, cfg.vocab_size, (64,),
                                   generator=gen).tolist()
            first_wave = 0
            for wave in range(2):
                prompts = [shared + torch.randint(
                    0, cfg.vocab_size, (5 + 3 * i,), generator=gen).tolist()
                    for i in range(3)]
                out = server.do_event(_Ev(prompts, 4)).body["outputs"]
                assert [len(row) for row in out] == [4, 4, 4]
                assert all(0 <= t < cfg.vocab_size
                           for row in out for t in row)
                stats = server.stats()["prefix_cache"]
                assert stats["requests"] == 3 * (wave + 1)
                if wave == 0:
                    first_wave = stats["hit_tokens"]
                    assert first_wave in (0, 64, 128)
                else:
                    assert stats["hit_tokens"] - first_wave == 3 * 64
        finally:
            server.shutdown()
