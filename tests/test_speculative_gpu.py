# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU numerics of speculative decoding: the attn_verify and
ngram_draft HIP kernels against the CPU references of the same ops, and
LlamaDecodeEngine.verify_step against decode_step."""

import pytest
import torch

from test_speculative import NGRAM_CASES

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

D = 128
# bf16 attention vs the fp32 reference (TestAttnDecode's bound)
ATOL = RTOL = 3e-2
# "same math, different reduction order" (test_tensor_parallel.py)
PREFILL_MAX_ERR = 0.25

B, SMAX = 6, 256
# no prefix, both sides of the 64-key tile edge, a chunk that straddles
# it (63 with QL >= 2), a multi-tile walk
BASE_LENS = [0, 1, 63, 64, 65, 200]
HEADS = [(8, 2), (2, 2), (8, 1)]
QLS = [1, 4, 8]


def _rand_bf16(*shape, scale=1.0, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return (torch.randn(*shape, dtype=torch.float32) * scale).to(
        torch.bfloat16)


def _i32(values):
    return torch.tensor(values, dtype=torch.int32)


def _close(got, ref):
    assert torch.isfinite(got.float()).all()
    err = (got.float() - ref.float()).abs().max().item()
    assert torch.allclose(got.float(), ref.float(), atol=ATOL,
                          rtol=RTOL), err


def _gpu(q, kc, vc, base, **kwargs):
    from mlrun_amd import ops

    got = ops.attn_verify(q.cuda(), kc.cuda(), vc.cuda(), base.cuda(),
                          **kwargs)
    torch.cuda.synchronize()
    return got.cpu()


_cases = {}


def _case(hq, hkv, ql):
    """(q, kc, vc, base, CPU reference), computed once per shape."""
    from mlrun_amd import ops

    key = (hq, hkv, ql)
    if key not in _cases:
        seed = 1000 + 100 * hq + 10 * hkv + ql
        q = _rand_bf16(B, ql, hq, D, seed=seed)
        kc = _rand_bf16(B, hkv, SMAX, D, seed=seed + 1)
        vc = _rand_bf16(B, hkv, SMAX, D, seed=seed + 2)
        base = _i32(BASE_LENS)
        _cases[key] = (q, kc, vc, base, ops.attn_verify(q, kc, vc, base))
    return _cases[key]


@requires_gpu
class TestAttnVerify:
    @pytest.mark.parametrize("ql", QLS)
    @pytest.mark.parametrize("hq,hkv", HEADS)
    def test_shapes(self, hq, hkv, ql):
        """G x QL covers 1 column, a partial tile, exactly 16, 32 and
        64; the default split count."""
        q, kc, vc, base, ref = _case(hq, hkv, ql)
        got = _gpu(q, kc, vc, base)
        assert got.shape == (B * ql, hq * D)
        _close(got, ref)

    @pytest.mark.parametrize("ql", QLS)
    @pytest.mark.parametrize("hq,hkv", HEADS)
    def test_forced_nsplit(self, hq, hkv, ql):
        """1, 2 and 4 splits on the same inputs, more splits than the
        short rows have tiles: each agrees with the reference, and they
        agree with each other."""
        q, kc, vc, base, ref = _case(hq, hkv, ql)
        outs = [_gpu(q, kc, vc, base, nsplit=ns) for ns in (1, 2, 4)]
        for got in outs:
            _close(got, ref)
        _close(outs[1], outs[0])
        _close(outs[2], outs[0])

    @pytest.mark.parametrize("nsplit", [1, 4])
    def test_stale_rows_contribute_nothing(self, nsplit):
        """Cache rows at and past base + QL hold NaN: the output stays
        finite and right."""
        ql = 4
        q = _rand_bf16(B, ql, 8, D, seed=30)
        kv = _rand_bf16(2, B, 2, SMAX, D, seed=31)
        kc = torch.full((B, 2, SMAX, D), float("nan"),
                        dtype=torch.bfloat16)
        vc = kc.clone()
        for b, n in enumerate(BASE_LENS):
            kc[b, :, :n + ql] = kv[0, b, :, :n + ql]
            vc[b, :, :n + ql] = kv[1, b, :, :n + ql]
        from mlrun_amd import ops

        base = _i32(BASE_LENS)
        ref = ops.attn_verify(q, kc, vc, base)
        assert torch.isfinite(ref.float()).all()
        _close(_gpu(q, kc, vc, base, nsplit=nsplit), ref)

    @pytest.mark.parametrize("nsplit", [1, 2, 4])
    def test_rescale_branch(self, nsplit):
        """Key magnitudes grow with the position, so the running max
        rises in every later tile and every later split: what was
        accumulated at the old max must be rescaled, not dropped."""
        from mlrun_amd import ops

        ql = 4
        q = _rand_bf16(B, ql, 8, D, seed=40)
        kc = _rand_bf16(B, 2, SMAX, D, seed=41)
        ramp = 0.25 + torch.arange(SMAX, dtype=torch.float32) / 64.0
        kc = (kc.float() * ramp.view(1, 1, SMAX, 1)).to(torch.bfloat16)
        vc = _rand_bf16(B, 2, SMAX, D, seed=42)
        base = _i32(BASE_LENS)
        ref = ops.attn_verify(q, kc, vc, base)
        _close(_gpu(q, kc, vc, base, nsplit=nsplit), ref)

    @pytest.mark.parametrize("ql", [1, 4])
    def test_strided_q_view(self, ql):
        """q as the engine passes it: a view into the qkv buffer."""
        from mlrun_amd import ops

        hq, hkv = 8, 2
        qkv = _rand_bf16(B * ql, (hq + 2 * hkv) * D, seed=50)
        kc = _rand_bf16(B, hkv, SMAX, D, seed=51)
        vc = _rand_bf16(B, hkv, SMAX, D, seed=52)
        base = _i32(BASE_LENS)
        ref = ops.attn_verify(qkv[:, :hq * D].view(B, ql, hq, D), kc, vc,
                              base)
        got = ops.attn_verify(
            qkv.cuda()[:, :hq * D].view(B, ql, hq, D), kc.cuda(),
            vc.cuda(), base.cuda())
        torch.cuda.synchronize()
        _close(got.cpu(), ref)

    def test_single_row_agrees_with_attn_decode(self):
        from mlrun_amd import ops

        q, kc, vc, base, _ = _case(8, 2, 1)
        got = _gpu(q, kc, vc, base)
        dec = ops.attn_decode(q.view(B, 8, D).cuda(), kc.cuda(), vc.cuda(),
                              (base + 1).cuda())
        torch.cuda.synchronize()
        _close(got.view(B, 8, D), dec.cpu())

    def test_preallocated_out_and_workspace(self):
        """The engine's calling convention: no allocation inside."""
        from mlrun_amd import ops

        q, kc, vc, base, ref = _case(8, 2, 4)
        out = torch.zeros(B * 4, 8 * D, dtype=torch.bfloat16,
                          device="cuda")
        ws = torch.empty(ops.attn_verify_ws_numel(B, 4, 8, 4),
                         dtype=torch.float32, device="cuda")
        got = ops.attn_verify(q.cuda(), kc.cuda(), vc.cuda(), base.cuda(),
                              out=out, nsplit=4, partial_ws=ws)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        _close(out.cpu(), ref)


@requires_gpu
class TestNgramDraft:
    @pytest.mark.parametrize("name", sorted(NGRAM_CASES))
    def test_case(self, name):
        from mlrun_amd import ops

        hist, length, k, n, want = NGRAM_CASES[name]
        got = ops.ngram_draft(
            torch.tensor([hist], dtype=torch.int64).cuda(),
            _i32([length]).cuda(), k, n=n)
        assert got.cpu()[0].tolist() == want

    @pytest.mark.parametrize("n", [1, 2, 3])
    def test_random_history_equals_reference(self, n):
        """Four symbols: many matches per row, so the max-reduction over
        lanes and waves decides; lengths from 0 to the whole row."""
        from mlrun_amd import ops

        gen = torch.Generator().manual_seed(7)
        hist = torch.randint(0, 4, (8, 256), generator=gen)
        lens = _i32([0, 1, 2, 3, 64, 255, 256, 300])
        want = ops.ngram_draft(hist, lens, 5, n=n)
        got = ops.ngram_draft(hist.cuda(), lens.cuda(), 5, n=n)
        assert torch.equal(got.cpu(), want)


@requires_gpu
class TestSpeculativeLoopGpu:
    """The loop end to end on the device.  Tokens are not compared with
    plain decoding beyond the first one (it comes from the same
    prefill): the verify pass and the decode step use different GEMMs,
    and a near-tie on random weights may resolve differently."""

    def test_generate_speculative(self):
        from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

        nb, s, new, k = 4, 9, 24, 3
        gen = torch.Generator().manual_seed(3)
        prompts = torch.randint(0, 1024, (nb, s), generator=gen)
        cfg = LlamaConfig.tiny()
        plain = LlamaDecodeEngine(cfg, nb, device="cuda:0",
                                  use_graph=False, seed=5)
        spec = LlamaDecodeEngine(cfg, nb, device="cuda:0",
                                 use_graph=False, seed=5)
        want = plain.generate(prompts, new).cpu()
        got = spec.generate_speculative(prompts, new, k=k).cpu()
        assert got.shape == (nb, new) and got.dtype == torch.int64
        assert torch.equal(got[:, 0], want[:, 0])
        assert int(got.min()) >= 0 and int(got.max()) < cfg.vocab_size
        stats = spec.spec_stats
        # every step emits at least one and at most k + 1 tokens per row
        assert (new - 1 + k) // (k + 1) <= stats["steps"] <= new - 1
        assert 0 <= stats["accepted"] <= stats["drafted"]
        assert stats["drafted"] <= stats["steps"] * nb * k
        # the cache holds every token but the pending one; rows stop
        # between new and new + k tokens
        lens = spec.cache_lens.cpu().tolist()
        assert all(s + new - 1 <= n <= s + new - 1 + k for n in lens)

    def test_server_switch(self):
        from mlrun_amd.models.llama import LlamaConfig, LlamaServer

        class Ev:
            path, id = "/infer", "t"

            def __init__(self, inputs, max_tokens):
                self.body = {"inputs": inputs, "max_tokens": max_tokens}

        prompts = [[1, 2, 3, 9, 9, 9, 9, 9, 9], [4, 5, 6, 7], [8, 9]]
        outs = []
        for kwargs in ({}, {"speculative": 3}):
            server = LlamaServer(name="s", config=LlamaConfig.tiny(),
                                 batch_size=4, use_graph=False,
                                 device="cuda:0", **kwargs)
            server.load()
            try:
                outs.append(server.do_event(Ev(prompts, 12)
                                            ).body["outputs"])
                stats = server.stats()
            finally:
                server.shutdown()
        assert [len(row) for row in outs[1]] == [12] * 3
        assert [row[0] for row in outs[1]] == [row[0] for row in outs[0]]
        assert all(0 <= t < 1024 for row in outs[1] for t in row)
        assert 3 <= stats["speculative"]["steps"] <= 11


@requires_gpu
class TestVerifyStepGpu:
    def test_logits_match_decode_steps(self):
        """Engine A decodes 8 tokens one by one; engine B (same seed)
        scores the same tokens at the same positions in two verify
        passes of 4 rows."""
        from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

        nb, s, k = 4, 9, 3
        gen = torch.Generator().manual_seed(3)
        prompts = torch.randint(0, 1024, (nb, s), generator=gen)

        def engine():
            eng = LlamaDecodeEngine(LlamaConfig.tiny(), nb,
                                    device="cuda:0", use_graph=False,
                                    seed=5)
            eng.buf_tokens.copy_(eng.prefill(prompts).argmax(dim=-1))
            return eng

        a, b = engine(), engine()
        tokens = [a.buf_tokens.clone()]   # tokens[i] is fed at s + i
        logits_a = []
        for _ in range(8):
            a.decode_step()
            logits_a.append(a.buf_logits.float().cpu())
            tokens.append(a.buf_tokens.clone())
        assert torch.equal(b.buf_tokens, tokens[0])
        for step in range(2):
            first = 4 * step
            # the same inputs as A whatever step 0 accepted
            b.cache_lens.fill_(s + first)
            b.buf_tokens.copy_(tokens[first])
            drafts = torch.stack(tokens[first + 1:first + 1 + k], dim=1)
            pred, n_acc = b.verify_step(drafts)
            torch.cuda.synchronize()
            got = b.buf_verify_logits.float().cpu()
            assert torch.isfinite(got).all()
            for j in range(k + 1):
                err = (got[:, j] - logits_a[first + j]).abs().max().item()
                print(f"verify step {step} row {j}: max err {err:.4f}")
                assert err < PREFILL_MAX_ERR, (step, j, err)
            # state recomputed on the host from pred and the drafts
            pred_h, drafts_h = pred.cpu(), drafts.cpu()
            # pred is an argmax of the kept logits (bf16 ties allowed)
            assert torch.equal(got.gather(2, pred_h.unsqueeze(-1)),
                               got.max(dim=-1, keepdim=True).values)
            for row in range(nb):
                n = 0
                while n < k and drafts_h[row, n] == pred_h[row, n]:
                    n += 1
                assert int(n_acc[row]) == n
                assert int(b.cache_lens[row]) == s + first + n + 1
                assert int(b.buf_tokens[row]) == int(pred_h[row, n])
