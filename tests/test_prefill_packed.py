# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Packed (varlen) prefill on CPU: the fp32 references of
ops.rope_kv_varlen / ops.attn_prefill, LlamaDecodeEngine.prefill_packed
and the prefill="packed" continuous server."""

import concurrent.futures
import threading

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaServer)

# the project's bound for "same prefill, different reduction order"
# (tests/test_tensor_parallel.py, prefill_max_err)
PREFILL_MAX_ERR = 0.25


def _rand_bf16(*shape, scale=1.0, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return (torch.randn(*shape, dtype=torch.float32) * scale).to(
        torch.bfloat16)


def _i32(values):
    return torch.tensor(values, dtype=torch.int32)


# ------------------------------------------------------------------ ops


class TestOpReferences:
    def test_len1_chunks_equal_attn_decode(self):
        """Every sequence one token long with kv_start = L-1 is decode
        attention with seq_lens = L: same caches, same bits."""
        B, Hq, Hkv, Smax, D = 3, 4, 2, 40, 128
        q = _rand_bf16(B, Hq, D, seed=0)
        kc = _rand_bf16(B, Hkv, Smax, D, seed=1)
        vc = _rand_bf16(B, Hkv, Smax, D, seed=2)
        lens = [1, 17, 40]
        ref = ops.attn_decode(q, kc, vc, _i32(lens))
        got = ops.attn_prefill(q, kc, vc, _i32([0, 1, 2, 3]),
                               _i32([0, 1, 2]),
                               _i32([n - 1 for n in lens]))
        assert got.shape == (B, Hq * D) and got.dtype == torch.bfloat16
        assert torch.equal(got.view(B, Hq, D), ref)

    def test_attn_prefill_is_causal_per_sequence(self):
        """Two packed sequences in swapped slots: each matches a dense
        masked softmax over its OWN cache row and nothing else."""
        Hq, Hkv, Smax, D = 4, 2, 24, 128
        lens, slots, starts = [5, 3], [2, 0], [0, 4]
        T = sum(lens)
        q = _rand_bf16(T, Hq, D, seed=3)
        kc = _rand_bf16(3, Hkv, Smax, D, seed=4)
        vc = _rand_bf16(3, Hkv, Smax, D, seed=5)
        got = ops.attn_prefill(q, kc, vc, _i32([0, 5, 8]), _i32(slots),
                               _i32(starts)).view(T, Hq, D)
        row = 0
        for length, slot, start in zip(lens, slots, starts):
            total = start + length
            for h in range(Hq):
                keys = kc[slot, h // 2, :total].float()
                vals = vc[slot, h // 2, :total].float()
                s = q[row:row + length, h].float() @ keys.t() / D ** 0.5
                pos = torch.arange(start, total)[:, None]
                s = s.masked_fill(torch.arange(total)[None, :] > pos,
                                  float("-inf"))
                want = torch.softmax(s, dim=-1) @ vals
                assert torch.allclose(got[row:row + length, h].float(),
                                      want, atol=2e-2, rtol=2e-2)
            row += length

    def test_rope_kv_varlen_reference(self):
        """= rope_inplace + manual scatter; every other cache element
        keeps its sentinel bits."""
        Hq, Hkv, D, B, Smax = 4, 2, 128, 4, 16
        lens, slots, starts = [3, 1, 5], [2, 0, 3], [0, 7, 4]
        T = sum(lens)
        qkv = _rand_bf16(T, (Hq + 2 * Hkv) * D, seed=6)
        cos_sin = ops.build_rope_cos_sin(Smax, D)
        positions = _i32([s + j for n, s in zip(lens, starts)
                          for j in range(n)])
        tok_slot = _i32([sl for n, sl in zip(lens, slots)
                         for _ in range(n)])
        sentinel = torch.tensor(-7.0).to(torch.bfloat16)
        kc = torch.full((B, Hkv, Smax, D), -7.0, dtype=torch.bfloat16)
        vc = torch.full((B, Hkv, Smax, D), -7.0, dtype=torch.bfloat16)

        want = qkv.clone()
        wq = want[:, :Hq * D].view(T, Hq, D)
        wk = want[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
        wv = want[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        ops.rope_inplace(wq, positions, cos_sin)
        ops.rope_inplace(wk, positions, cos_sin)

        ops.rope_kv_varlen(qkv, kc, vc, positions, tok_slot, cos_sin, Hq)
        assert torch.equal(qkv, want)
        written = torch.zeros(B, Smax, dtype=torch.bool)
        for t in range(T):
            slot, pos = int(tok_slot[t]), int(positions[t])
            assert torch.equal(kc[slot, :, pos], wk[t])
            assert torch.equal(vc[slot, :, pos], wv[t])
            written[slot, pos] = True
        untouched = ~written[:, None, :, None].expand_as(kc)
        assert torch.equal(kc[untouched],
                           sentinel.expand(int(untouched.sum())))
        assert torch.equal(vc[untouched],
                           sentinel.expand(int(untouched.sum())))


# --------------------------------------------------------------- engine


def _engine_pair(batch_size=4, **kwargs):
    cfg = LlamaConfig.tiny()
    first = LlamaDecodeEngine(cfg, batch_size, device="cpu", **kwargs)
    twin = LlamaDecodeEngine(cfg, batch_size, device="cpu",
                             weights=first.weights, **kwargs)
    return first, twin


class TestEnginePrefillPacked:
    def test_single_prompt_matches_prefill_slots(self):
        packed, exact = _engine_pair()
        prompt = [5, 9, 2, 77, 31, 8, 100]
        slot, S = 2, len(prompt)
        got = packed.prefill_packed([prompt], [slot])
        ref = exact.prefill_slots(torch.tensor([prompt]),
                                  torch.tensor([slot]))
        assert got.shape == ref.shape == (1, packed.cfg.vocab_size)
        err = (got.float() - ref.float()).abs().max().item()
        assert err < PREFILL_MAX_ERR, err
        assert packed.cache_lens.tolist() == exact.cache_lens.tolist()
        assert packed.cache_lens[slot] == S
        for cache_p, cache_e in ((packed.k_cache, exact.k_cache),
                                 (packed.v_cache, exact.v_cache)):
            assert torch.allclose(cache_p[:, slot, :, :S].float(),
                                  cache_e[:, slot, :, :S].float(),
                                  atol=3e-2, rtol=3e-2)
            # nothing else was written
            rest = cache_p.clone()
            rest[:, slot, :, :S] = 0
            assert not rest.any()
        assert packed.buf_tokens[slot] == got[0].argmax()

    def test_two_chunk_continuation(self):
        oneshot, chunked = _engine_pair()
        prompt = [3, 14, 15, 92, 65, 35, 89, 79, 32, 38, 46]
        k, slot, S = 4, 1, len(prompt)
        ref = oneshot.prefill_packed([prompt], [slot])
        chunked.prefill_packed([prompt[:k]], [slot])
        assert chunked.cache_lens[slot] == k
        got = chunked.prefill_packed([prompt[k:]], [slot], starts=[k])
        assert chunked.cache_lens[slot] == S
        err = (got.float() - ref.float()).abs().max().item()
        assert err < PREFILL_MAX_ERR, err
        for cache_c, cache_o in ((chunked.k_cache, oneshot.k_cache),
                                 (chunked.v_cache, oneshot.v_cache)):
            assert torch.allclose(cache_c[:, slot, :, :S].float(),
                                  cache_o[:, slot, :, :S].float(),
                                  atol=3e-2, rtol=3e-2)

    def test_mixed_lengths_then_decode(self):
        """Three lengths in one pass; each row agrees with its own
        single-prompt pass and a decode step advances every slot."""
        packed, alone = _engine_pair()
        prompts = [[1, 2, 3], [4, 5, 6, 7, 8, 9, 10], [11]]
        slots = [3, 0, 2]
        got = packed.prefill_packed(prompts, slots)
        assert got.shape == (3, packed.cfg.vocab_size)
        for i, (prompt, slot) in enumerate(zip(prompts, slots)):
            alone.reset()
            ref = alone.prefill_packed([prompt], [slot])
            err = (got[i].float() - ref[0].float()).abs().max().item()
            assert err < PREFILL_MAX_ERR, (i, err)
        assert packed.cache_lens.tolist() == [7, 0, 1, 3]
        packed.decode_step()
        assert packed.cache_lens.tolist() == [8, 1, 2, 4]

    def test_duplicate_slots_raise(self):
        engine, _ = _engine_pair()
        with pytest.raises(ValueError, match="duplicate slots"):
            engine.prefill_packed([[1, 2], [3]], [1, 1])

    def test_overlong_sequence_raises(self):
        engine, _ = _engine_pair()
        smax = engine.cfg.max_seq_len
        with pytest.raises(ValueError, match="max_seq_len"):
            engine.prefill_packed([[1] * smax], [0])
        with pytest.raises(ValueError, match="max_seq_len"):
            engine.prefill_packed([[1, 2, 3]], [0], starts=[smax - 3])
        # the longest sequence that still leaves room for one token
        engine.prefill_packed([[1, 2, 3]], [0], starts=[smax - 4])

    def test_out_of_range_token_raises_before_any_write(self):
        engine, _ = _engine_pair()
        for bad in ([1, engine.cfg.vocab_size], [-1, 2]):
            with pytest.raises(ValueError, match="token id"):
                engine.prefill_packed([[1, 2], bad], [0, 1])
        assert engine.cache_lens.tolist() == [0, 0, 0, 0]
        assert not engine.k_cache.any()

    def test_fp8_kv_raises(self):
        engine = LlamaDecodeEngine(LlamaConfig.tiny(), 2, device="cpu",
                                   kv_dtype="fp8")
        with pytest.raises(ValueError,
                           match="packed prefill needs a bf16 KV cache"):
            engine.prefill_packed([[1, 2, 3]], [0])


# --------------------------------------------------------------- server


class _Ev:
    path = "/infer"
    id = "t"

    def __init__(self, inputs, max_tokens):
        self.body = {"inputs": inputs, "max_tokens": max_tokens}


def _server(prefill=None, **kwargs):
    extra = {} if prefill is None else {"prefill": prefill}
    server = LlamaServer(name="p", config=LlamaConfig.tiny(),
                         batch_size=4, max_new_tokens=6,
                         scheduling="continuous", use_graph=False,
                         device="cpu", **extra, **kwargs)
    server.load()
    return server


class TestPackedServer:
    def test_batch_invariance(self):
        """A prompt served alone and the same prompt admitted together
        with two prompts of other lengths: exactly the same tokens."""
        server = _server("packed")
        try:
            prompt = [4, 5, 6, 7]
            alone = server.do_event(_Ev([prompt], 5)).body["outputs"][0]
            mixed = server.do_event(
                _Ev([[1, 2, 3, 9, 9, 9, 9, 9, 9], prompt, [8, 9]], 5)
            ).body["outputs"]
            assert len(alone) == 5
            assert mixed[1] == alone
        finally:
            server.shutdown()

    @pytest.mark.parametrize("mode,want", [("packed", (1, 0)),
                                           (None, (0, 3))])
    def test_one_pass_for_a_mixed_group(self, mode, want):
        """Three prompts of three lengths queued before the loop starts:
        one prefill_packed call under "packed", three prefill_slots
        calls under the default."""
        server = _server(mode)
        server.shutdown()  # stop the worker; the loop is restarted below
        engine = server.engines[0]
        calls = {"packed": 0, "slots": 0}
        real_packed, real_slots = engine.prefill_packed, engine.prefill_slots

        def count_packed(*args, **kwargs):
            calls["packed"] += 1
            return real_packed(*args, **kwargs)

        def count_slots(*args, **kwargs):
            calls["slots"] += 1
            return real_slots(*args, **kwargs)

        engine.prefill_packed = count_packed
        engine.prefill_slots = count_slots
        futures = []
        for prompt in ([1, 2, 3], [4, 5, 6, 7], [8, 9]):
            future = concurrent.futures.Future()
            server._tasks.put((prompt, 3, future))
            futures.append(future)
        worker = threading.Thread(target=server._continuous_loop,
                                  args=(engine,), daemon=True)
        worker.start()
        try:
            outputs = [f.result(timeout=60) for f in futures]
        finally:
            server._tasks.put(None)
            worker.join(timeout=10)
        assert all(len(out) == 3 for out in outputs)
        assert (calls["packed"], calls["slots"]) == want

    def test_bad_prompt_fails_its_request_not_the_loop(self):
        server = _server("packed")
        try:
            with pytest.raises(ValueError, match="token id"):
                server.do_event(_Ev([[10 ** 9]], 3))
            out = server.do_event(_Ev([[1, 2, 3]], 3)).body["outputs"]
            assert len(out[0]) == 3
        finally:
            server.shutdown()

    def test_default_mode_is_exact(self):
        server = LlamaServer(name="p", config=LlamaConfig.tiny())
        assert server.prefill == "exact"
        with pytest.raises(ValueError, match="prefill mode"):
            LlamaServer(name="p", config=LlamaConfig.tiny(),
                        prefill="padded")

    def test_fp8_kv_with_packed_fails_at_load(self):
        server = LlamaServer(name="p", config=LlamaConfig.tiny(),
                             batch_size=2, scheduling="continuous",
                             use_graph=False, kv_dtype="fp8",
                             device="cpu", prefill="packed")
        with pytest.raises(ValueError, match="bf16 KV cache"):
            server.load()
        assert not server.engines
