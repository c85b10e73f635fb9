# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Prompt scoring, CPU tier: the reference branch of ops.lm_head_logprobs,
LlamaDecodeEngine.score_packed, their argument checks, and the server's
"prompt_logprobs" field."""

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import LlamaConfig, LlamaServer

from decode_refs import EPS32, f64
from lm_head_refs import PROMPTS, check_score_packed, engine


def operands(t=5, v=40, k=64):
    g = torch.Generator().manual_seed(3)
    h = torch.randn(t, k, generator=g).to(torch.bfloat16)
    w = torch.randn(v, k, generator=g).to(torch.bfloat16)
    return h, w, torch.tensor([0, v - 1, 7, -1, v], dtype=torch.int32)


def test_cpu_branch_against_float64():
    """The bf16 logits are the contract's; lse and the gather on them are
    fp32 torch code: a few roundings of values of at most |lse|."""
    h, w, targets = operands()
    logprob, lse = ops.lm_head_logprobs(h, w, targets)
    z = f64((h.float() @ w.float().t()).to(torch.bfloat16))
    ref_lse = torch.logsumexp(z, -1)
    ref = torch.stack([z[0, 0], z[1, 39], z[2, 7], z[3, 0] * 0,
                       z[4, 0] * 0]) - ref_lse
    bound = 8 * EPS32 * (ref_lse.abs() + z.abs().amax(-1))
    assert ((f64(lse) - ref_lse).abs() <= bound).all()
    assert ((f64(logprob) - ref).abs() <= bound).all()
    assert torch.equal(logprob[3:], -lse[3:])  # out of range: exactly -lse


def test_score_packed_on_cpu_against_prefix_prefills():
    check_score_packed("cpu")


@pytest.mark.parametrize("change, match", [
    (dict(h=torch.zeros(5, 48, dtype=torch.bfloat16),
          w=torch.zeros(40, 48, dtype=torch.bfloat16)), "K % 32"),
    (dict(targets=torch.zeros(5, dtype=torch.int64)), "targets"),
    (dict(targets=torch.zeros(4, dtype=torch.int32)), "targets"),
    (dict(h=torch.zeros(5, 64)), "bf16"),
    (dict(workspace=torch.zeros(3)), "workspace"),
    (dict(bn=32), "bn"),
])
def test_op_rejects(change, match):
    h, w, targets = operands()
    with pytest.raises(ValueError, match=match):
        ops.lm_head_logprobs(**{**dict(h=h, w=w, targets=targets), **change})


@pytest.mark.parametrize("kwargs, match", [
    (dict(kv_dtype="fp8"), "bf16 KV"),
    (dict(weight_dtype="fp8w"), "weight_dtype"),
])
def test_engine_rejects(kwargs, match):
    with pytest.raises(ValueError, match=match):
        engine("cpu", **kwargs).score_packed(PROMPTS, [0, 1])


class _Ev:
    id, path = "ev", ""

    def __init__(self, **body):
        self.body = body


def server(**kwargs):
    made = LlamaServer(name="s", config=LlamaConfig.tiny(), batch_size=4,
                       max_new_tokens=3, use_graph=False, device="cpu",
                       **kwargs)
    made.load()
    return made


def test_server_round_trip():
    inputs = [[1, 2, 3, 4], [9, 8, 7, 6, 5, 4], [11]]
    packed = server(scheduling="continuous", prefill="packed")
    exact = server(scheduling="continuous")
    try:
        plain = packed.do_event(_Ev(inputs=inputs, max_tokens=3)).body
        assert "prompt_logprobs" not in plain
        body = packed.do_event(_Ev(inputs=inputs, max_tokens=3,
                                   prompt_logprobs=[True, False, True])).body
        assert body["outputs"] == plain["outputs"]
        first, second, third = body["prompt_logprobs"]
        assert len(first) == 3 and second is None and third == []
        assert all(isinstance(x, float) and x < 0 for x in first)
        everyone = packed.do_event(_Ev(inputs=inputs, max_tokens=3,
                                       prompt_logprobs=True)).body
        assert [len(r) for r in everyone["prompt_logprobs"]] == [3, 5, 0]
        assert everyone["prompt_logprobs"][0] == first
        with pytest.raises(ValueError, match="prompt_logprobs"):
            exact.do_event(_Ev(inputs=inputs, prompt_logprobs=True))
        assert len(exact.do_event(_Ev(inputs=inputs, max_tokens=3)
                                  ).body["outputs"]) == 3  # still serving
    finally:
        packed.shutdown()
        exact.shutdown()
