# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""score_packed against its prefix reference, for the CPU and the GPU tier
of the prompt-scoring tests."""

import torch

from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

from decode_refs import R1, check, f64

TINY = dict(num_layers=2, num_heads=4, num_kv_heads=2, hidden_size=512,
            intermediate_size=1024, vocab_size=2048)
PROMPTS = [[5, 900, 17, 2000, 33], [1, 44, 1300, 8, 8, 250, 77, 1999, 3]]


def engine(device, batch_size=2, **kwargs):
    return LlamaDecodeEngine(LlamaConfig.tiny(**TINY), batch_size=batch_size,
                             device=device, use_graph=False, seed=41,
                             **kwargs)


def check_score_packed(device):
    """Reference: every proper prefix of each prompt through prefill_packed
    on a second engine of the same seed, log_softmax of its last-token
    logits at the next token.  The two sides differ in GEMM row counts
    only, so the tolerance is twice the spread of the reference against
    itself (prefixes packed in one call against one call each) plus
    2 R1 |ref|.  Returns (spread, largest error)."""
    scored = engine(device)
    logits, logprobs = scored.score_packed(PROMPTS, [0, 1])
    plain = engine(device)
    assert torch.equal(logits, plain.prefill_packed(PROMPTS, [0, 1]))
    for name in ("cache_lens", "buf_tokens"):
        assert torch.equal(getattr(scored, name), getattr(plain, name)), name

    prefixes = [p[:j] for p in PROMPTS for j in range(1, len(p))]
    nxt = torch.tensor([p[j] for p in PROMPTS for j in range(1, len(p))])
    ref_engine = engine(device, batch_size=len(prefixes))

    def at_next(rows):
        return torch.log_softmax(f64(rows), -1).gather(1, nxt[:, None])[:, 0]

    ref = at_next(ref_engine.prefill_packed(prefixes, range(len(prefixes))))
    ref_engine.reset()
    alone = at_next(torch.cat(
        [ref_engine.prefill_packed([q], [i]) for i, q in enumerate(prefixes)]))
    spread = (ref - alone).abs().max().item()
    assert [len(row) for row in logprobs] == [len(p) - 1 for p in PROMPTS]
    got = torch.cat(logprobs)
    assert got.dtype == torch.float32 and got.device.type == \
        torch.device(device).type
    err = (f64(got) - ref).abs().max().item()
    print(f"score_packed {device}: spread {spread:.4g}, largest error "
          f"{err:.4g}")
    check(got, ref, 2 * spread + 2 * R1 * ref.abs(),
          f"score_packed on {device} vs prefix prefills")
    return spread, err
