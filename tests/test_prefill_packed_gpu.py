# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU numerics of packed (varlen) prefill: the attn_prefill and
rope_kv_varlen HIP kernels against the CPU fp32 references of the same
ops, and LlamaDecodeEngine.prefill_packed against prefill_slots."""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

D = 128
# bf16 attention vs the fp32 reference (TestAttnDecode's bound)
ATOL = RTOL = 3e-2
# "same prefill, different reduction order" (test_tensor_parallel.py)
PREFILL_MAX_ERR = 0.25


def _rand_bf16(*shape, scale=1.0, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return (torch.randn(*shape, dtype=torch.float32) * scale).to(
        torch.bfloat16)


def _i32(values):
    return torch.tensor(values, dtype=torch.int32)


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return _i32(cu)


def _run_both(q, kc, vc, lens, slots, starts):
    """(reference on CPU, kernel result copied back)"""
    from mlrun_amd import ops

    cu, slots, starts = _cu(lens), _i32(slots), _i32(starts)
    ref = ops.attn_prefill(q, kc, vc, cu, slots, starts)
    got = ops.attn_prefill(q.cuda(), kc.cuda(), vc.cuda(), cu.cuda(),
                           slots.cuda(), starts.cuda(),
                           max_q_len=max(lens))
    torch.cuda.synchronize()
    return ref, got.cpu()


def _close(got, ref):
    assert torch.isfinite(got.float()).all()
    err = (got.float() - ref.float()).abs().max().item()
    assert torch.allclose(got.float(), ref.float(), atol=ATOL,
                          rtol=RTOL), err


@requires_gpu
class TestAttnPrefill:
    @pytest.mark.parametrize("hq,hkv", [(8, 2), (2, 2), (8, 1)])
    def test_tile_edge_lengths(self, hq, hkv):
        """Lengths around the 16-row wave tile and the 64-row block and
        KV tiles, one packed call, slots out of order, Smax no tile
        multiple."""
        lens = [1, 15, 17, 63, 64, 65, 130]
        slots = [5, 2, 7, 0, 3, 6, 1]
        q = _rand_bf16(sum(lens), hq, D, seed=10)
        kc = _rand_bf16(8, hkv, 160, D, seed=11)
        vc = _rand_bf16(8, hkv, 160, D, seed=12)
        ref, got = _run_both(q, kc, vc, lens, slots, [0] * len(lens))
        _close(got, ref)

    def test_kv_start_offsets(self):
        """A diagonal that does not begin at a tile origin, a pure
        decode row, and a chunk that crosses a KV tile edge."""
        lens, starts = [5, 33, 1, 70], [0, 40, 64, 7]
        slots = [3, 1, 6, 4]
        q = _rand_bf16(sum(lens), 8, D, seed=20)
        kc = _rand_bf16(8, 2, 160, D, seed=21)
        vc = _rand_bf16(8, 2, 160, D, seed=22)
        ref, got = _run_both(q, kc, vc, lens, slots, starts)
        _close(got, ref)

    def test_stale_rows_contribute_nothing(self):
        """Cache rows past a sequence's end hold NaN: the output stays
        finite and right (0 x NaN in the P.V product is the trap)."""
        lens, starts = [5, 33, 1, 70], [0, 40, 64, 7]
        slots = [3, 1, 6, 4]
        q = _rand_bf16(sum(lens), 8, D, seed=30)
        kv = _rand_bf16(2, 8, 2, 160, D, seed=31)
        kc = torch.full((8, 2, 160, D), float("nan"),
                        dtype=torch.bfloat16)
        vc = kc.clone()
        for n, slot, start in zip(lens, slots, starts):
            kc[slot, :, :start + n] = kv[0, slot, :, :start + n]
            vc[slot, :, :start + n] = kv[1, slot, :, :start + n]
        ref, got = _run_both(q, kc, vc, lens, slots, starts)
        assert torch.isfinite(ref.float()).all()
        _close(got, ref)

    def test_rescale_branch(self):
        """One key row whose score dominates arrives after earlier KV
        tiles were accumulated: the running max jumps and the O built
        so far must be rescaled, not dropped."""
        lens, slots = [130], [4]
        q = _rand_bf16(130, 8, D, seed=40)
        kc = _rand_bf16(8, 2, 160, D, seed=41)
        vc = _rand_bf16(8, 2, 160, D, seed=42)
        kc[4, :, 100] = (kc[4, :, 100].float() * 12.0).to(torch.bfloat16)
        ref, got = _run_both(q, kc, vc, lens, slots, [0])
        # the spike really moves the max for the rows that see it
        scores = q[100:, 0].float() @ kc[4, 0, :101].float().t()
        assert (scores.argmax(dim=1) == 100).any()
        _close(got, ref)

    def test_strided_q_view(self):
        """q as a view into the packed qkv buffer = its dense copy."""
        from mlrun_amd import ops

        hq, hkv = 8, 2
        lens, slots = [17, 65], [1, 0]
        T = sum(lens)
        qkv = _rand_bf16(T, (hq + 2 * hkv) * D, seed=50).cuda()
        kc = _rand_bf16(2, hkv, 160, D, seed=51).cuda()
        vc = _rand_bf16(2, hkv, 160, D, seed=52).cuda()
        q_view = qkv[:, :hq * D].view(T, hq, D)
        assert not q_view.is_contiguous()
        args = (kc, vc, _cu(lens).cuda(), _i32(slots).cuda(),
                _i32([0, 0]).cuda())
        strided = ops.attn_prefill(q_view, *args, max_q_len=max(lens))
        dense = ops.attn_prefill(q_view.contiguous(), *args,
                                 max_q_len=max(lens))
        assert torch.equal(strided, dense)
        ref = ops.attn_prefill(q_view.cpu(), *(a.cpu() for a in args))
        _close(strided.cpu(), ref)


@requires_gpu
class TestRopeKvVarlen:
    def test_matches_reference(self):
        """T = 37 tokens over 3 slots: roped q/k, cache rows, and
        sentinel bits everywhere else."""
        from mlrun_amd import ops

        hq, hkv, B, smax = 4, 2, 4, 48
        lens, slots, starts = [10, 20, 7], [2, 0, 3], [0, 3, 5]
        T = sum(lens)
        assert T == 37
        qkv = _rand_bf16(T, (hq + 2 * hkv) * D, seed=60)
        cos_sin = ops.build_rope_cos_sin(smax, D)
        positions = _i32([s + j for n, s in zip(lens, starts)
                          for j in range(n)])
        tok_slot = _i32([sl for n, sl in zip(lens, slots)
                         for _ in range(n)])
        kc = torch.full((B, hkv, smax, D), -7.0, dtype=torch.bfloat16)
        vc = torch.full((B, hkv, smax, D), 9.0, dtype=torch.bfloat16)
        qkv_g, kc_g, vc_g = qkv.cuda(), kc.cuda(), vc.cuda()
        ops.rope_kv_varlen(qkv_g, kc_g, vc_g, positions.cuda(),
                           tok_slot.cuda(), cos_sin.cuda(), hq)
        torch.cuda.synchronize()
        ops.rope_kv_varlen(qkv, kc, vc, positions, tok_slot, cos_sin, hq)
        assert torch.allclose(qkv_g.cpu().float(), qkv.float(),
                              atol=2e-2, rtol=2e-2)
        kc_g, vc_g = kc_g.cpu(), vc_g.cpu()
        written = torch.zeros(B, smax, dtype=torch.bool)
        written[tok_slot.long(), positions.long()] = True
        assert int(written.sum()) == T
        mask = written[:, None, :, None].expand_as(kc)
        assert torch.allclose(kc_g[mask].float(), kc[mask].float(),
                              atol=2e-2, rtol=2e-2)
        # v is a plain copy
        assert torch.equal(vc_g[mask], vc[mask])
        assert torch.equal(kc_g[~mask].view(torch.int16),
                           kc[~mask].view(torch.int16))
        assert torch.equal(vc_g[~mask].view(torch.int16),
                           vc[~mask].view(torch.int16))
        assert (kc_g[~mask] == -7.0).all() and (vc_g[~mask] == 9.0).all()


@requires_gpu
class TestEnginePrefillPackedGpu:
    def test_matches_prefill_slots_and_decodes(self):
        from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

        cfg = LlamaConfig.tiny()
        packed = LlamaDecodeEngine(cfg, 4, device="cuda:0",
                                   use_graph=False)
        exact = LlamaDecodeEngine(cfg, 4, device="cuda:0",
                                  use_graph=False, weights=packed.weights)
        gen = torch.Generator().manual_seed(70)
        lens, slots = [3, 9, 20], [2, 0, 3]
        prompts = [torch.randint(0, cfg.vocab_size, (n,),
                                 generator=gen).tolist() for n in lens]
        got = packed.prefill_packed(prompts, slots)
        refs = [exact.prefill_slots(torch.tensor([p]),
                                    torch.tensor([s]))
                for p, s in zip(prompts, slots)]
        torch.cuda.synchronize()
        assert got.shape == (3, cfg.vocab_size)
        for i, ref in enumerate(refs):
            err = (got[i].float() - ref[0].float()).abs().max().item()
            assert err < PREFILL_MAX_ERR, (i, err)
        assert packed.cache_lens.tolist() == exact.cache_lens.tolist() \
            == [9, 0, 3, 20]
        for n, slot in zip(lens, slots):
            for mine, theirs in ((packed.k_cache, exact.k_cache),
                                 (packed.v_cache, exact.v_cache)):
                assert torch.allclose(mine[:, slot, :, :n].float(),
                                      theirs[:, slot, :, :n].float(),
                                      atol=ATOL, rtol=RTOL)
        packed.decode_step()
        torch.cuda.synchronize()
        assert packed.cache_lens.tolist() == [10, 1, 4, 21]
