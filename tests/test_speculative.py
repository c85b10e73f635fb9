# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Speculative greedy decoding on the CPU reference path: the
attn_verify and ngram_draft references, LlamaDecodeEngine.verify_step
and generate_speculative against plain greedy decoding, and the
LlamaServer(speculative=k) switch."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaServer)

D = 128


def _rand_bf16(*shape, seed):
    torch.manual_seed(seed)
    return torch.randn(*shape, dtype=torch.float32).to(torch.bfloat16)


def _i32(values):
    return torch.tensor(values, dtype=torch.int32)


# ------------------------------------------------------ ops.attn_verify


class TestAttnVerifyReference:
    def test_equals_attn_prefill_reference(self):
        B, QL, hq, hkv = 3, 4, 4, 2
        q = _rand_bf16(B, QL, hq, D, seed=1)
        kc = _rand_bf16(B, hkv, 96, D, seed=2)
        vc = _rand_bf16(B, hkv, 96, D, seed=3)
        base = _i32([0, 17, 90])
        got = ops.attn_verify(q, kc, vc, base)
        want = ops.attn_prefill(q.reshape(B * QL, hq, D), kc, vc,
                                _i32([0, 4, 8, 12]), _i32([0, 1, 2]), base)
        assert got.shape == (B * QL, hq * D)
        assert got.dtype == torch.bfloat16
        assert torch.equal(got, want)

    def test_strided_q_view(self):
        B, QL, hq, hkv = 2, 3, 2, 2
        qkv = _rand_bf16(B * QL, (hq + 2 * hkv) * D, seed=4)
        kc = _rand_bf16(B, hkv, 40, D, seed=5)
        vc = _rand_bf16(B, hkv, 40, D, seed=6)
        base = _i32([5, 30])
        view = qkv[:, :hq * D].view(B, QL, hq, D)
        got = ops.attn_verify(view, kc, vc, base)
        want = ops.attn_verify(view.contiguous(), kc, vc, base)
        assert torch.equal(got, want)

    def test_single_row_equals_attn_decode(self):
        B, hq, hkv = 3, 4, 2
        q = _rand_bf16(B, 1, hq, D, seed=7)
        kc = _rand_bf16(B, hkv, 50, D, seed=8)
        vc = _rand_bf16(B, hkv, 50, D, seed=9)
        base = _i32([0, 11, 49])
        got = ops.attn_verify(q, kc, vc, base)
        want = ops.attn_decode(q.view(B, hq, D), kc, vc, base + 1)
        assert torch.equal(got.view(B, hq, D), want)

    def test_unsupported_shapes_raise(self):
        kc = _rand_bf16(1, 1, 32, D, seed=10)
        base = _i32([4])
        with pytest.raises(ValueError, match="QL"):
            ops.attn_verify(_rand_bf16(1, 9, 1, D, seed=11), kc, kc, base)
        with pytest.raises(ValueError, match="QL"):
            ops.attn_verify(_rand_bf16(1, 0, 1, D, seed=11), kc, kc, base)
        with pytest.raises(ValueError, match="head_dim"):
            k64 = _rand_bf16(1, 1, 32, 64, seed=12)
            ops.attn_verify(_rand_bf16(1, 2, 1, 64, seed=13), k64, k64,
                            base)
        with pytest.raises(ValueError, match="bf16"):
            k8 = torch.zeros(1, 1, 32, D, dtype=torch.uint8)
            ops.attn_verify(_rand_bf16(1, 2, 1, D, seed=14), k8, k8, base)
        with pytest.raises(ValueError, match="kv head"):
            ops.attn_verify(_rand_bf16(1, 2, 16, D, seed=15), kc, kc, base)


# ------------------------------------------------------ ops.ngram_draft

# (history, len, k, n, expected drafts)
NGRAM_CASES = {
    "match_in_the_middle":
        ([1, 2, 3, 4, 5, 6, 2, 3, 0, 0], 8, 3, 2, [4, 5, 6]),
    "latest_of_two_matches":
        ([7, 8, 1, 7, 8, 2, 5, 7, 8, 0], 9, 2, 2, [2, 5]),
    "continuation_runs_off_the_end":
        ([9, 4, 4, 4, 0, 0, 0, 0, 0, 0], 4, 3, 2, [4, 4, 4]),
    "continuation_padded_with_last":
        ([3, 5, 6, 3, 5, 0, 0, 0, 0, 0], 5, 4, 2, [6, 3, 5, 5]),
    "no_match":
        ([1, 2, 3, 4, 5, 0, 0, 0, 0, 0], 5, 3, 2, [5, 5, 5]),
    "len_below_n_plus_1":
        ([6, 6, 0, 0, 0, 0, 0, 0, 0, 0], 2, 2, 2, [6, 6]),
    "len_zero":
        ([9, 9, 9, 9, 9, 9, 9, 9, 9, 9], 0, 3, 2, [0, 0, 0]),
    "unigram":
        ([5, 1, 5, 2, 5, 0, 0, 0, 0, 0], 5, 2, 1, [2, 5]),
    "len_clamped_to_row":
        ([1, 2, 3, 1, 2, 4, 1, 2, 5, 1], 99, 2, 1, [2, 5]),
}


class TestNgramDraft:
    @pytest.mark.parametrize("name", sorted(NGRAM_CASES))
    def test_case(self, name):
        hist, length, k, n, want = NGRAM_CASES[name]
        got = ops.ngram_draft(torch.tensor([hist], dtype=torch.int64),
                              _i32([length]), k, n=n)
        assert got.dtype == torch.int64 and got.shape == (1, k)
        assert got[0].tolist() == want

    def test_rows_are_independent(self):
        names = ["match_in_the_middle", "no_match", "len_zero"]
        hist = torch.tensor([NGRAM_CASES[n][0] for n in names],
                            dtype=torch.int64)
        lens = _i32([NGRAM_CASES[n][1] for n in names])
        got = ops.ngram_draft(hist, lens, 3, n=2)
        assert got.tolist() == [NGRAM_CASES[n][4] for n in names]

    def test_bad_arguments(self):
        hist = torch.zeros(1, 4, dtype=torch.int64)
        with pytest.raises(ValueError):
            ops.ngram_draft(hist, _i32([2]), 0)
        with pytest.raises(ValueError):
            ops.ngram_draft(hist, _i32([2]), 2, n=0)
        with pytest.raises(ValueError):
            ops.ngram_draft(hist.int(), _i32([2]), 2)


# ---------------------------------------------------------- verify_step

B, S, K = 3, 7, 3


def _prompts(seed=0):
    gen = torch.Generator().manual_seed(100 + seed)
    return torch.randint(0, 1024, (B, S), generator=gen)


def _engine(seed=0, **kwargs):
    return LlamaDecodeEngine(LlamaConfig.tiny(), B, device="cpu",
                             seed=seed, **kwargs)


@pytest.fixture(scope="module")
def truth():
    """Plain greedy continuation of _prompts(): [B, 12] tokens."""
    return _engine().generate(_prompts(), 12)


def _prefilled():
    """An engine right after prefill: buf_tokens is the first generated
    token, cache_lens == S."""
    engine = _engine()
    logits = engine.prefill(_prompts())
    engine.buf_tokens.copy_(logits.argmax(dim=-1))
    return engine


class TestVerifyStep:
    def test_perfect_drafts_are_all_accepted(self, truth):
        engine = _prefilled()
        assert torch.equal(engine.buf_tokens, truth[:, 0])
        pred, n_acc = engine.verify_step(truth[:, 1:1 + K])
        assert pred.shape == (B, K + 1) and n_acc.shape == (B,)
        assert n_acc.tolist() == [K] * B
        assert torch.equal(pred, truth[:, 1:K + 2])
        assert engine.cache_lens.tolist() == [S + K + 1] * B
        assert torch.equal(engine.buf_tokens, truth[:, K + 1])
        assert engine.buf_verify_logits.shape == (B, K + 1, 1024)

    def test_wrong_drafts_cost_nothing_but_the_step(self, truth):
        engine, plain = _prefilled(), _prefilled()
        wrong = (truth[:, 1:1 + K] + 1) % 1024
        pred, n_acc = engine.verify_step(wrong)
        plain.decode_step()
        assert n_acc.tolist() == [0] * B
        assert engine.cache_lens.tolist() == [S + 1] * B
        assert torch.equal(engine.buf_tokens, pred[:, 0])
        assert torch.equal(engine.buf_tokens, plain.buf_tokens)
        assert torch.equal(engine.buf_tokens, truth[:, 1])
        # the K/V rows of the rejected drafts lie beyond cache_lens:
        # the next plain step must not see them
        engine.decode_step()
        plain.decode_step()
        assert torch.equal(engine.buf_tokens, plain.buf_tokens)
        assert torch.equal(engine.buf_tokens, truth[:, 2])

    def test_first_draft_right_only(self, truth):
        engine = _prefilled()
        drafts = (truth[:, 1:1 + K] + 1) % 1024
        drafts[:, 0] = truth[:, 1]
        pred, n_acc = engine.verify_step(drafts)
        assert n_acc.tolist() == [1] * B
        assert engine.cache_lens.tolist() == [S + 2] * B
        assert torch.equal(pred[:, :2], truth[:, 1:3])
        assert torch.equal(engine.buf_tokens, truth[:, 2])

    def test_mixed_acceptance_per_row(self, truth):
        engine = _prefilled()
        drafts = truth[:, 1:1 + K].clone()
        drafts[1, 2] = (drafts[1, 2] + 1) % 1024   # row 1: 2 accepted
        drafts[2, 0] = (drafts[2, 0] + 1) % 1024   # row 2: 0 accepted
        pred, n_acc = engine.verify_step(drafts)
        assert n_acc.tolist() == [K, 2, 0]
        assert engine.cache_lens.tolist() == [S + K + 1, S + 3, S + 1]
        want = [truth[0, K + 1], truth[1, 3], truth[2, 1]]
        assert engine.buf_tokens.tolist() == [int(t) for t in want]

    def test_out_of_range_drafts_are_rejected(self, truth):
        engine = _prefilled()
        drafts = torch.tensor([[10 ** 9, 5, 5], [-7, 5, 5],
                               [1024, 5, 5]], dtype=torch.int64)
        pred, n_acc = engine.verify_step(drafts)
        assert n_acc.tolist() == [0] * B
        assert torch.equal(engine.buf_tokens, truth[:, 1])

    @pytest.mark.parametrize("k", [0, 8])
    def test_k_out_of_range(self, k):
        engine = _engine()
        with pytest.raises(ValueError, match="k must be"):
            engine.verify_step(torch.zeros(B, k, dtype=torch.int64))

    def test_restrictions(self):
        drafts = torch.zeros(B, K, dtype=torch.int64)
        with pytest.raises(ValueError, match="bf16 KV"):
            _engine(kv_dtype="fp8").verify_step(drafts)
        with pytest.raises(ValueError, match="greedy"):
            _engine(temperature=0.7).verify_step(drafts)
        with pytest.raises(ValueError, match="greedy"):
            _engine(temperature=-1.0).verify_step(drafts)
        engine = _engine()
        engine.weight_dtype = "fp8w"
        with pytest.raises(ValueError, match="bf16 weights"):
            engine.verify_step(drafts)
        engine = _engine()
        engine.tp_size = 2
        with pytest.raises(ValueError, match="tp_size"):
            engine.verify_step(drafts)
        with pytest.raises(ValueError, match="drafts must be"):
            _engine().verify_step(torch.zeros(B + 1, K, dtype=torch.int64))


# ------------------------------------------------- generate_speculative


class TestGenerateSpeculative:
    @pytest.mark.parametrize("seed", range(6))
    def test_equals_generate(self, seed):
        """Token for token, for k = 1, 3 and 7."""
        prompts = _prompts(seed)
        want = _engine(seed).generate(prompts, 20)
        for k in (1, 3, 7):
            engine = _engine(seed)
            got = engine.generate_speculative(prompts, 20, k=k)
            assert torch.equal(got, want), (seed, k)
            stats = engine.spec_stats
            assert 1 <= stats["steps"] <= 19
            assert 0 <= stats["accepted"] <= stats["drafted"]
            assert stats["drafted"] <= stats["steps"] * B * k

    def test_something_is_accepted(self):
        """The tiny model's greedy output repeats, so the n-gram drafter
        must land some drafts; with every draft rejected the loop would
        need max_new - 1 steps."""
        accepted = 0
        for seed in range(6):
            engine = _engine(seed)
            engine.generate_speculative(_prompts(seed), 20, k=3)
            accepted += engine.spec_stats["accepted"]
        assert accepted > 0

    def test_one_token(self):
        prompts = _prompts()
        got = _engine().generate_speculative(prompts, 1)
        assert torch.equal(got, _engine().generate(prompts, 1))

    def test_capacity(self):
        engine = _engine()
        smax = engine.cfg.max_seq_len
        with pytest.raises(AssertionError, match="room for k"):
            engine.generate_speculative(_prompts(), smax - S - 2, k=3)
        with pytest.raises(ValueError, match="k must be"):
            engine.generate_speculative(_prompts(), 4, k=8)

    def test_fills_the_cache_to_the_brim(self):
        """S + max_new + k == max_seq_len exactly: no row runs past the
        cache while slower rows catch up."""
        cfg = LlamaConfig.tiny(max_seq_len=32)
        prompts = _prompts()
        want = LlamaDecodeEngine(cfg, B, device="cpu", seed=0
                                 ).generate(prompts, 32 - S - 3)
        got = LlamaDecodeEngine(cfg, B, device="cpu", seed=0
                                ).generate_speculative(prompts, 32 - S - 3,
                                                       k=3)
        assert torch.equal(got, want)


# --------------------------------------------------------------- server


class _Ev:
    path = "/infer"
    id = "t"

    def __init__(self, inputs, max_tokens):
        self.body = {"inputs": inputs, "max_tokens": max_tokens}


def _server(**kwargs):
    server = LlamaServer(name="s", config=LlamaConfig.tiny(),
                         batch_size=4, max_new_tokens=6, use_graph=False,
                         device="cpu", **kwargs)
    server.load()
    return server


class TestServerSwitch:
    def test_same_outputs_as_plain_batch_mode(self):
        prompts = [[1, 2, 3, 9, 9, 9, 9, 9, 9], [4, 5, 6, 7], [8, 9]]
        outs = []
        for kwargs in ({}, {"speculative": 3}):
            server = _server(**kwargs)
            try:
                outs.append(server.do_event(_Ev(prompts, 12)
                                            ).body["outputs"])
                stats = server.stats()
            finally:
                server.shutdown()
        assert outs[0] == outs[1]
        assert [len(row) for row in outs[1]] == [12] * 3
        assert stats["speculative"]["steps"] >= 1

    def test_stop_token_trimming_unchanged(self):
        prompts = [[4, 5, 6, 7], [8, 9]]
        plain = _server()
        try:
            full = plain.do_event(_Ev(prompts, 10)).body["outputs"]
        finally:
            plain.shutdown()
        stop = full[0][3]
        outs = []
        for kwargs in ({}, {"speculative": 2}):
            server = _server(stop_token=stop, **kwargs)
            try:
                outs.append(server.do_event(_Ev(prompts, 10)
                                            ).body["outputs"])
            finally:
                server.shutdown()
        assert outs[0] == outs[1]
        assert outs[1][0][-1] == stop and len(outs[1][0]) <= 4

    def test_default_is_off(self):
        server = LlamaServer(name="s", config=LlamaConfig.tiny())
        assert server.speculative == 0
        assert server.stats() == {}

    @pytest.mark.parametrize("kwargs,match", [
        ({"scheduling": "continuous"}, "continuous"),
        ({"temperature": 0.8}, "temperature"),
        ({"kv_dtype": "fp8"}, "kv_dtype"),
        ({"weight_dtype": "fp8w"}, "weight_dtype"),
        ({"speculative": 8}, "outside"),
    ])
    def test_invalid_combinations(self, kwargs, match):
        args = {"speculative": 3, **kwargs}
        with pytest.raises(ValueError, match=match):
            LlamaServer(name="s", config=LlamaConfig.tiny(), **args)

    def test_conflict_set_after_init_fails_at_load(self):
        server = LlamaServer(name="s", config=LlamaConfig.tiny(),
                             batch_size=2, use_graph=False, device="cpu",
                             speculative=3)
        server.kv_dtype = "fp8"
        with pytest.raises(ValueError, match="kv_dtype"):
            server.load()

    def test_request_past_capacity_fails(self):
        server = _server(speculative=3)
        try:
            with pytest.raises(ValueError, match="max_seq_len"):
                server.do_event(_Ev([[1, 2, 3]], 252))
        finally:
            server.shutdown()
