# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU checks of the logit processors: the logit_processors HIP kernel
against the CPU branch of the same op, bit for bit on logits and on the
token-state table, and the logit_processors=True engine on the tiny
config: against a teacher-forced engine without the flag, and under a
captured graph."""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

BATCHES = [1, 5, 64]
# one vector; one exact tile; a tile plus one vector; two tiles plus one
# vector; llama's vocabulary
VOCABS = [8, 2048, 2056, 4104, 128256]


def _edges(V):
    """Column 0, V - 1 and both sides of every multiple of LOGIT_TILE."""
    from mlrun_amd import ops

    cols = {0, V - 1}
    for start in range(ops.LOGIT_TILE, V + 1, ops.LOGIT_TILE):
        cols.update(c for c in (start - 1, start) if c < V)
    return sorted(cols)


_CASES = {}


def make_case(B, V, with_tokens=True):
    """Inputs of one (B, V) case and what the CPU branch makes of them,
    built once: (args, want_logits, want_state).  Row kinds cycle through
    everything on, bias only, neutral, repetition only and frequency /
    presence only; bias_n through 0, 1 and 64.  Counts, prompt bits and
    bias ids sit on every edge column; the pending tokens hit every edge
    of the small vocabularies and spread over all tiles of llama's,
    which has more edges than a launch has rows."""
    from mlrun_amd import ops

    key = (B, V, with_tokens)
    if key in _CASES:
        return _CASES[key]
    NB = ops.LOGIT_BIAS_MAX
    gen = torch.Generator().manual_seed(1000 * B + V)
    edges = _edges(V)
    S = B + 2
    logits = torch.randn(B, V, generator=gen) * 3
    state = torch.zeros(S, V, dtype=torch.int32)
    seen = torch.rand(S, V, generator=gen) < 0.05
    state[seen] = torch.randint(1, 9, (int(seen.sum()),), generator=gen,
                                dtype=torch.int32)
    penalties = torch.zeros(B, 3)
    bias_ids = torch.randint(0, V, (B, NB), generator=gen,
                             dtype=torch.int32)
    bias_val = torch.empty(B, NB).uniform_(-100, 100, generator=gen)
    bias_n = torch.zeros(B, dtype=torch.int32)
    tokens = torch.zeros(B, dtype=torch.int64)
    rows = (torch.randperm(B, generator=gen) + 1).to(torch.int32)
    if B > 1:
        rows[B // 2] = S if B % 2 else -1      # one entry out of range
    for b in range(B):
        kind = (b + 3) % 5
        penalties[b] = torch.tensor([
            [1.0, 0.0, 0.0], [1.3, 0.0, 0.0], [1.0, 0.5, 0.25],
            [0.7, -0.3, 1.1], [1.0, 0.0, 0.0]][kind])
        bias_n[b] = 0 if kind == 0 else (
            (1, NB)[b % 2] if kind == 4 else (0, 1, NB)[(b // 5 + b) % 3])
        # the edge columns, from a row-dependent offset, in every role
        mine = [edges[(37 * b + j) % len(edges)] for j in range(len(edges))]
        tokens[b] = mine[0]
        # distinct ids (of duplicates an unspecified one would apply):
        # edges first, then other columns, then ids to be ignored
        others = [c for c in torch.randperm(V, generator=gen)[:NB].tolist()
                  if c not in edges]
        ids = (mine + others)[:NB - 2]
        ids += [V, -1, V + 7, -2 ** 31, 2 ** 31 - 1] * NB
        bias_ids[b] = torch.tensor(ids[:NB], dtype=torch.int32)
        row = int(rows[b])
        if 0 <= row < S:
            for j, col in enumerate(mine):
                state[row, col] = (0, 1, 2, 7, 3)[j % 5]
        for j, col in enumerate(mine[:8]):      # large magnitudes
            logits[b, col] = (3e4, -3e4, 1e30, -1e30, 1e-30, 0.0, 250.0,
                              -0.0)[j]
    if B >= 5:
        tokens[3], tokens[4] = -1, V            # pending tokens to ignore
    if B == 1:
        bias_n[0] = NB
    args =[logits.to(torch.bfloat16), state, penalties, bias_ids, bias_val,
            bias_n, tokens if with_tokens else None, rows]
    want_logits, want_state = args[0].clone(), state.clone()
    ops.logit_processors(want_logits, want_state, *args[2:])
    _CASES[key] = (args, want_logits, want_state)
    return _CASES[key]


def run_gpu(args):
    from mlrun_amd import ops

    dev = [None if a is None else a.clone().cuda() for a in args]
    out = ops.logit_processors(*dev)
    assert out is dev[0]
    torch.cuda.synchronize()
    return dev[0].cpu(), dev[1].cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@requires_gpu
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("B", BATCHES)
def test_kernel_matches_the_cpu_branch(B, V):
    args, want_logits, want_state = make_case(B, V)
    # the case is no no-op: the reference changed logits and counts
    assert not torch.equal(want_state, args[1])
    assert not _same_bits(want_logits, args[0])
    logits, state = run_gpu(args)
    assert torch.equal(state, want_state)
    assert _same_bits(logits, want_logits)


@requires_gpu
@pytest.mark.parametrize("B, V", [(5, 2056), (64, 128256)])
def test_kernel_without_pending_tokens(B, V):
    args, want_logits, want_state = make_case(B, V, with_tokens=False)
    assert torch.equal(want_state, args[1])     # nothing is counted
    logits, state = run_gpu(args)
    assert torch.equal(state, want_state)
    assert _same_bits(logits, want_logits)


@requires_gpu
def test_rows_none_is_the_identity_mapping():
    from mlrun_amd import ops

    args, _, _ = make_case(5, 4104)
    args = list(args)
    args[7] = None
    want_logits, want_state = args[0].clone(), args[1].clone()
    ops.logit_processors(want_logits, want_state, *args[2:])
    logits, state = run_gpu(args)
    assert torch.equal(state, want_state)
    assert _same_bits(logits, want_logits)


@requires_gpu
def test_same_call_twice_is_bitwise_equal():
    args, _, _ = make_case(64, 128256)
    first = run_gpu(args)
    second = run_gpu(args)
    assert _same_bits(first[0], second[0])
    assert torch.equal(first[1], second[1])


@requires_gpu
def test_bad_arguments_raise_before_any_launch():
    from mlrun_amd import ops

    args, _, _ = make_case(5, 2056)
    dev = [a.clone().cuda() for a in args]
    with pytest.raises(ValueError, match="rows is on cpu"):
        ops.logit_processors(*dev[:7], args[7])
    flat = torch.zeros(5 * 2056 + 4, dtype=torch.bfloat16, device="cuda")
    view = flat[4:].view(5, 2056)
    assert view.is_contiguous() and view.data_ptr() % 16
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.logit_processors(view, *dev[1:])
    torch.cuda.synchronize()
    assert torch.equal(dev[1].cpu(), args[1])


# --------------------------------------------------------------- engine

PROMPTS = [[5, 9, 2, 77, 130], [400, 3, 3, 8, 1], [7, 7, 21, 4, 4],
           [1, 2, 3, 4, 5]]
# penalised, neutral, biased and sampled, everything at once
SLOT_PARAMS = [
    dict(repetition_penalty=1.5, presence_penalty=0.5),
    dict(),
    dict(temperature=0.8, top_p=0.9, seed=4, logit_bias={9: 3.0, 77: -2.0}),
    dict(temperature=5.0, seed=3, repetition_penalty=0.8,
         presence_penalty=-1.0, frequency_penalty=1.5,
         logit_bias={1023: 4.0})]


def _gpu_engine(use_graph, flag=True, weights=None):
    from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

    return LlamaDecodeEngine(LlamaConfig.tiny(), 4, device="cuda:0",
                             use_graph=use_graph, sampling="request",
                             logit_processors=flag, weights=weights)


def _reference(raw, prompts, generated, slot_params):
    """The CPU branch applied to raw logits [4, V] with the host-
    recounted state: prompt bits, and every generated token of the rows
    that count."""
    from mlrun_amd import ops
    from mlrun_amd.models.llama import SamplingParams

    B, V = raw.shape
    NB = ops.LOGIT_BIAS_MAX
    state = torch.zeros(B, V, dtype=torch.int32)
    penalties = torch.zeros(B, 3)
    ids = torch.zeros(B, NB, dtype=torch.int32)
    val = torch.zeros(B, NB)
    cnt = torch.zeros(B, dtype=torch.int32)
    for b, fields in enumerate(slot_params):
        params = SamplingParams(**fields)
        state[b, torch.tensor(prompts[b])] = 1
        if not params.neutral_processors():
            for token in generated[b]:
                state[b, token] += 2
        penalties[b] = torch.tensor([params.repetition_penalty,
                                     params.presence_penalty,
                                     params.frequency_penalty])
        for j, (key, value) in enumerate(params.bias_items()):
            ids[b, j], val[b, j] = key, value
        cnt[b] = len(params.bias_items())
    out = raw.clone()
    ops.logit_processors(out, state, penalties, ids, val, cnt)
    return out, state


@requires_gpu
def test_engine_logits_are_the_reference_on_the_raw_logits():
    """P runs the processors, N does not and is teacher-forced with P's
    tokens: N's logits are the raw logits P started from."""
    P = _gpu_engine(False)
    N = _gpu_engine(False, flag=False, weights=P.weights)
    for slot, fields in enumerate(SLOT_PARAMS):
        P.set_sampling(slot, **fields)
    tokens = torch.tensor(PROMPTS)
    got_first = P.prefill_slots(tokens, torch.arange(4))
    raw_first = N.prefill_slots(tokens, torch.arange(4))
    generated = [[] for _ in PROMPTS]
    want, _ = _reference(raw_first.cpu(), PROMPTS, generated, SLOT_PARAMS)
    assert _same_bits(got_first.cpu(), want)
    changed = 0
    for _ in range(6):
        N.buf_tokens.copy_(P.buf_tokens)
        for b, token in enumerate(P.buf_tokens.tolist()):
            generated[b].append(token)        # pending: counted this step
        P.decode_step()
        N.decode_step()
        torch.cuda.synchronize()
        raw = N.buf_logits.cpu()
        want, state = _reference(raw, PROMPTS, generated, SLOT_PARAMS)
        assert _same_bits(P.buf_logits.cpu(), want)
        assert torch.equal(P.buf_tok_state.cpu(), state)
        assert _same_bits(want[1], raw[1])    # the neutral row
        changed += int((want.view(torch.int16)
                        != raw.view(torch.int16)).sum())
    assert changed > 0


def _run_engine(engine, slot_params, steps=8, rewrite=None):
    """Prefill PROMPTS into slots 0..3 and decode; tokens per step
    [steps, 4] and the final state table, on the host.  ``rewrite`` =
    (step, slot, fields) rewrites one slot's parameters mid-run."""
    engine.reset()
    for slot, fields in enumerate(slot_params):
        engine.set_sampling(slot, **fields)
    engine.prefill_slots(torch.tensor(PROMPTS), torch.arange(4))
    if engine.use_graph:
        engine.capture_graph()
    out = [engine.buf_tokens.clone()]
    for step in range(steps):
        if rewrite is not None and step == rewrite[0]:
            engine.set_sampling(rewrite[1], **rewrite[2])
        engine.decode_step()
        out.append(engine.buf_tokens.clone())
    torch.cuda.synchronize()
    return torch.stack(out).cpu(), engine.buf_tok_state.cpu()


@requires_gpu
def test_engine_graph_matches_eager_and_follows_set_sampling():
    eager = _gpu_engine(False)
    graph = _gpu_engine(True, weights=eager.weights)
    want_tokens, want_state = _run_engine(eager, SLOT_PARAMS)
    got_tokens, got_state = _run_engine(graph, SLOT_PARAMS)
    assert graph._graph is not None
    assert torch.equal(got_tokens, want_tokens)
    # fails if the three warm-up steps of the capture leak into the counts
    assert torch.equal(got_state, want_state)
    V = want_state.shape[1]
    for b in (0, 2, 3):
        row = torch.zeros(V, dtype=torch.int32)
        row[torch.tensor(PROMPTS[b])] = 1
        for token in want_tokens[:-1, b].tolist():
            row[token] += 2
        assert torch.equal(want_state[b], row)
    # new parameters under the SAME captured graph, no recapture
    captured = graph._graph
    rewrite = (3, 1, dict(logit_bias={321: 100.0}))
    got2_tokens, got2_state = _run_engine(graph, SLOT_PARAMS,
                                          rewrite=rewrite)
    assert graph._graph is captured
    want2_tokens, want2_state = _run_engine(eager, SLOT_PARAMS,
                                            rewrite=rewrite)
    assert torch.equal(got2_tokens, want2_tokens)
    assert torch.equal(got2_state, want2_state)
    assert torch.equal(got2_tokens[:4], got_tokens[:4])
    assert got2_tokens[4:, 1].tolist() == [321] * 5
    assert torch.equal(got2_tokens[:, [0, 2, 3]], got_tokens[:, [0, 2, 3]])
