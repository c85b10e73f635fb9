# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU checks of per-request sampling: the fused sample_tokens HIP kernel
against the CPU reference of the same op (filters exactly, the draw up to
genuine near-ties), its determinism and row independence, and the
sampling="request" engine and server on the tiny config."""

import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

BATCHES = [1, 5, 64]
# one 16 B vector; the tiny vocabulary; one 256-lane x 8 sweep plus a
# tail; llama's vocabulary
VOCABS = [8, 1024, 2056, 128256]

# a draw may differ from the reference only on a near-tie of the f64
# scores: a few f32 ulps of z / T plus the two logf roundings
TIE_BAND = 2.0 ** -14
# an f32 tree sum over 128256 terms is good to ~1e-6 relative
LOGPROB_ATOL = 1e-4
# rows whose filter boundary lies this close are not decidable across
# two expf implementations: the generator draws them again
BOUNDARY = 2.0 ** -20


def _params(B, V, gen, shift):
    """Per-row (T, k, p, min_p): greedy rows, filter-off rows and a mix
    of k in {1, 50, V}, p in {0.5, 0.9, 1}, min_p in {0, 0.05}."""
    T = torch.empty(B).uniform_(0.3, 2.0, generator=gen)
    k = torch.tensor([1, 50, V, 0])[torch.randint(0, 4, (B,), generator=gen)]
    p = torch.tensor([0.5, 0.9, 1.0])[torch.randint(0, 3, (B,),
                                                    generator=gen)]
    mp = torch.tensor([0.0, 0.05])[torch.randint(0, 2, (B,), generator=gen)]
    for b in range(B):
        kind = (b + shift) % 6
        if kind == 0:       # greedy
            T[b] = 0.0
        elif kind == 1:     # sampled, every filter off
            k[b], p[b], mp[b] = 0, 1.0, 0.0
        elif kind == 2:     # every filter on
            k[b], p[b], mp[b] = 50, 0.9, 0.05
    return T, k.to(torch.int32), p, mp


def _undecidable(ref, p, mp):
    """Rows whose top_p cut or min_p bound is within BOUNDARY."""
    Q = ref["Q"].astype(np.float64)
    need = ref["need"].astype(np.float64)
    bad = np.zeros(len(Q), dtype=bool)
    p_on = p.numpy() < 1
    for tail in (ref["tail_cut"], ref["tail_above"]):
        bad |= p_on & (np.abs(tail.astype(np.float64) - need)
                       <= BOUNDARY * Q)
    bound = mp.numpy().astype(np.float64)[:, None] * 2.0 ** 32
    near = np.abs(ref["q"].astype(np.float64) - bound) <= BOUNDARY * 2.0 ** 32
    bad |= (mp.numpy() > 0) & near.any(axis=1)
    return bad


_CASES = {}


def make_case(B, V):
    """Logits, parameters and the CPU reference of one (B, V) case,
    built once.  Undecidable rows are drawn again (the next draw of the
    generator), never skipped."""
    from mlrun_amd import ops

    if (B, V) in _CASES:
        return _CASES[(B, V)]
    gen = torch.Generator().manual_seed(1000 * B + V)
    T, k, p, mp = _params(B, V, gen, shift=VOCABS.index(V))
    pos = torch.randint(0, 2048, (B,), generator=gen, dtype=torch.int32)
    seed = torch.randint(0, 2 ** 62, (B,), generator=gen, dtype=torch.int64)
    logits = (torch.randn(B, V, generator=gen) * 3).to(torch.bfloat16)
    args = (pos, T, k, p, mp, seed)
    ref = ops.sample_tokens_reference(logits, *args)
    for _ in range(50):
        bad = _undecidable(ref, p, mp) & (T.numpy() != 0)
        if not bad.any():
            break
        idx = torch.from_numpy(np.nonzero(bad)[0])
        logits[idx] = (torch.randn(len(idx), V, generator=gen) * 3
                       ).to(torch.bfloat16)
        ref = ops.sample_tokens_reference(logits, *args)
    else:
        raise AssertionError("case generator did not settle")
    _CASES[(B, V)] = (logits, args, ref)
    return _CASES[(B, V)]


def run_gpu(logits, args, fill=None):
    from mlrun_amd import ops

    B = logits.shape[0]
    tokens = torch.full((B,), -7 if fill else 0, dtype=torch.int64,
                        device="cuda")
    logprob = torch.full((B,), 123.0 if fill else 0.0, device="cuda")
    kept = torch.full((B,), -7 if fill else 0, dtype=torch.int32,
                      device="cuda")
    out = ops.sample_tokens(logits.cuda(), *[a.cuda() for a in args],
                            out_tokens=tokens, out_logprob=logprob,
                            out_kept=kept)
    assert out is tokens
    torch.cuda.synchronize()
    return tokens.cpu(), logprob.cpu(), kept.cpu()


def check_draw(logits, ref, tokens, logprob, rows=None, T=None):
    """Token equal to the reference's, or a near-tie of the f64 scores;
    logprob against f64 log_softmax at the GPU's token."""
    z = logits.double()
    lsm = torch.log_softmax(z, dim=-1)
    for b in (range(logits.shape[0]) if rows is None else rows):
        tok = int(tokens[b])
        assert 0 <= tok < logits.shape[1]
        want = float(lsm[b, tok])
        assert abs(float(logprob[b]) - want) <= LOGPROB_ATOL, \
            (b, float(logprob[b]), want)
        if tok == int(ref["tokens"][b]):
            continue
        assert T is not None and float(T[b]) != 0.0, \
            f"greedy row {b}: {tok} != {int(ref['tokens'][b])}"
        assert ref["keep"][b, tok], f"row {b}: token {tok} was filtered"
        u = ref["u"][b].astype(np.float64)
        score = ref["s"][b].astype(np.float64) - np.log(-np.log(u))
        best = score[ref["keep"][b]].max()
        assert score[tok] >= best - TIE_BAND * max(1.0, abs(best)), \
            (b, tok, score[tok], best)


@requires_gpu
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("B", BATCHES)
def test_kernel_matches_reference(B, V):
    logits, args, ref = make_case(B, V)
    tokens, logprob, kept = run_gpu(logits, args)
    print("kept gpu", kept.tolist()[:8], "ref", ref["kept"].tolist()[:8])
    assert kept.tolist() == ref["kept"].tolist()
    check_draw(logits, ref, tokens, logprob, T=args[1])
    mismatched = int((tokens.numpy() != ref["tokens"]).sum())
    print("tokens differing on a near-tie:", mismatched, "of", B)


@requires_gpu
def test_same_call_twice_is_bitwise_equal():
    logits, args, _ = make_case(64, 128256)
    first = run_gpu(logits, args)
    second = run_gpu(logits, args)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@requires_gpu
def test_row_does_not_depend_on_batch_or_neighbours():
    logits, args, _ = make_case(64, 128256)
    # a row with every filter on (kind 2 of _params at shift 3)
    row = next(b for b in range(64) if (b + 3) % 6 == 2)
    assert float(args[1][row]) != 0 and int(args[2][row]) == 50
    alone = run_gpu(logits[row:row + 1].contiguous(),
                    [a[row:row + 1].clone() for a in args])
    # slot 63 of a batch of different rows
    moved_logits = logits.clone()
    moved_logits[63] = logits[row]
    moved_logits[row] = logits[63]
    moved_args = [a.clone() for a in args]
    for a in moved_args:
        a[63], a[row] = a[row].clone(), a[63].clone()
    moved = run_gpu(moved_logits, moved_args)
    # the same slot among neighbours with other parameters
    other_args = [a.clone() for a in moved_args]
    other_args[1][:63] = 1.7           # temperature
    other_args[2][:63] = 3             # top_k
    other_args[3][:63] = 0.4           # top_p
    other_args[5][:63] += 11           # seed
    other = run_gpu(moved_logits, other_args)
    for got in (moved, other):
        for a, b in zip(alone, got):
            assert torch.equal(a[0], b[63])
    full = run_gpu(logits, args)
    for a, b in zip(alone, full):
        assert torch.equal(a[0], b[row])


@requires_gpu
def test_negative_pos_rows_are_untouched():
    logits, args, ref = make_case(5, 2056)
    args = [a.clone() for a in args]
    args[0][1] = -1
    args[0][3] = -5
    tokens, logprob, kept = run_gpu(logits, args, fill=True)
    for b in (1, 3):
        assert int(tokens[b]) == -7 and int(kept[b]) == -7
        assert float(logprob[b]) == 123.0
    live = [0, 2, 4]
    assert [int(kept[b]) for b in live] == [int(ref["kept"][b])
                                            for b in live]
    check_draw(logits, ref, tokens, logprob, rows=live, T=args[1])


@requires_gpu
def test_out_of_range_parameters_give_the_argmax():
    """The kernel is total: one row per parameter set outside the
    validated ranges (a temperature whose division overflows, with and
    without filters; negative and NaN temperatures; min_p > 1; top_p
    <= 0), plus an in-range row.  Each out-of-range row returns the
    argmax with kept = 1, like the reference, and every token is a
    valid index."""
    V = 2056
    gen = torch.Generator().manual_seed(7)
    rows = [(1.2e-38, 0, 1.0, 0.1), (1.2e-38, 0, 1.0, 0.0),
            (1.2e-38, 50, 0.5, 0.05), (-1.0, 0, 1.0, 0.0),
            (float("nan"), 3, 0.9, 0.1), (1.5, 0, 1.0, 2.0),
            (1.5, 0, 0.0, 0.0), (1.5, 0, -1.0, 0.0), (1.0, 0, 1.0, 0.0)]
    B = len(rows)
    logits = (torch.randn(B, V, generator=gen) * 3).to(torch.bfloat16)
    logits[:, 1999] = 30.0  # a unique maximum; 30 / 1.2e-38 overflows
    args = (torch.arange(B, dtype=torch.int32),
            torch.tensor([r[0] for r in rows]),
            torch.tensor([r[1] for r in rows], dtype=torch.int32),
            torch.tensor([r[2] for r in rows]),
            torch.tensor([r[3] for r in rows]),
            torch.arange(B, dtype=torch.int64) + 40)
    from mlrun_amd import ops
    ref = ops.sample_tokens_reference(logits, *args)
    tokens, logprob, kept = run_gpu(logits, args, fill=True)
    print("tokens", tokens.tolist(), "kept", kept.tolist())
    assert all(0 <= t < V for t in tokens.tolist())
    assert tokens[:-1].tolist() == [1999] * (B - 1)
    assert kept.tolist() == [1] * (B - 1) + [V]
    assert kept.tolist() == ref["kept"].tolist()
    want = torch.log_softmax(logits.double(), dim=-1)
    for b in range(B):
        assert abs(float(logprob[b]) - float(want[b, int(tokens[b])])) \
            <= LOGPROB_ATOL


@requires_gpu
def test_misaligned_logits_raise_value_error():
    """A contiguous [B, V] view that does not start on a 16-byte
    boundary is refused in Python, before any launch."""
    from mlrun_amd import ops

    B, V = 2, 16
    flat = torch.zeros(B * V + 4, dtype=torch.bfloat16, device="cuda")
    view = flat[4:].view(B, V)
    assert view.is_contiguous() and view.data_ptr() % 16
    tokens = torch.zeros(B, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.sample_tokens(
            view, torch.zeros(B, dtype=torch.int32, device="cuda"),
            torch.ones(B, device="cuda"),
            torch.zeros(B, dtype=torch.int32, device="cuda"),
            torch.ones(B, device="cuda"), torch.zeros(B, device="cuda"),
            torch.zeros(B, dtype=torch.int64, device="cuda"), tokens)


# --------------------------------------------------------------- engine

PROMPTS = [[5, 9, 2, 77, 130], [400, 3, 3, 8, 1], [7, 7, 21, 4, 4],
           [1, 2, 3, 4, 5]]
# mixed greedy and sampled slots
SLOT_PARAMS = [dict(), dict(temperature=5.0, seed=3),
               dict(temperature=0.8, top_k=40, top_p=0.9, min_p=0.01,
                    seed=4), dict()]


def _gpu_engine(use_graph, weights=None):
    from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

    return LlamaDecodeEngine(LlamaConfig.tiny(), 4, device="cuda:0",
                             use_graph=use_graph, sampling="request",
                             weights=weights)


def _run_engine(engine, slot_params, steps=12):
    """Prefill PROMPTS into slots 0..3 and decode; tokens, logprobs and
    kept counts per step as host tensors [steps, 4]."""
    engine.reset()
    for slot, params in enumerate(slot_params):
        engine.set_sampling(slot, **params)
    engine.prefill_slots(torch.tensor(PROMPTS), torch.arange(4))
    if engine.use_graph:
        engine.capture_graph()
    out = [(engine.buf_tokens.clone(), engine.buf_logprob.clone(),
            engine.buf_kept.clone())]
    for _ in range(steps - 1):
        engine.decode_step()
        out.append((engine.buf_tokens.clone(), engine.buf_logprob.clone(),
                    engine.buf_kept.clone()))
    torch.cuda.synchronize()
    return [torch.stack(part).cpu() for part in zip(*out)]


@requires_gpu
def test_engine_graph_matches_eager_and_follows_set_sampling():
    eager = _gpu_engine(False)
    graph = _gpu_engine(True, weights=eager.weights)
    want = _run_engine(eager, SLOT_PARAMS)
    got = _run_engine(graph, SLOT_PARAMS)
    assert graph._graph is not None
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert want[2][:, 0].tolist() == [1] * 12        # greedy slot
    assert want[2][:, 1].tolist() == [1024] * 12     # filters off
    assert 1 <= int(want[2][:, 2].max()) <= 40 + 8   # top_k (+ ties)
    # new parameters under the SAME captured graph, no recapture
    changed = [dict(temperature=5.0, seed=9)] + SLOT_PARAMS[1:]
    captured = graph._graph
    got2 = _run_engine(graph, changed)
    assert graph._graph is captured
    want2 = _run_engine(eager, changed)
    for a, b in zip(want2, got2):
        assert torch.equal(a, b)
    assert got2[0][:, 0].tolist() != got[0][:, 0].tolist()
    assert torch.equal(got2[0][:, 1:], got[0][:, 1:])  # others unmoved


@requires_gpu
def test_engine_first_step_matches_the_cpu_engine():
    from mlrun_amd import ops
    from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                        LlamaWeights)

    gpu = _gpu_engine(False)
    cfg = LlamaConfig.tiny()
    weights = LlamaWeights(cfg, torch.device("cpu"))
    weights.load_state_dict({key: value.cpu() for key, value
                             in gpu.weights.state_dict().items()})
    cpu = LlamaDecodeEngine(cfg, 4, device="cpu", sampling="request",
                            weights=weights)
    slot_params = [dict(), dict(temperature=5.0, seed=3),
                   dict(temperature=5.0, top_p=0.95, seed=4), dict()]
    for engine in (gpu, cpu):
        for slot, params in enumerate(slot_params):
            engine.set_sampling(slot, **params)
    slots = torch.arange(4)
    logits = gpu.prefill_slots(torch.tensor(PROMPTS), slots)
    cpu.prefill_slots(torch.tensor(PROMPTS), slots)
    torch.cuda.synchronize()
    got, want = gpu.buf_tokens.cpu(), cpu.buf_tokens
    # the reference draw on the GPU's own logits, for the tie band
    ref = ops.sample_tokens_reference(
        logits, gpu.cache_lens, gpu.buf_temp_r, gpu.buf_top_k,
        gpu.buf_top_p, gpu.buf_min_p, gpu.buf_seed)
    assert gpu.cache_lens.tolist() == [5] * 4
    for slot in (0, 3):  # greedy rows: token for token
        assert int(got[slot]) == int(want[slot])
    for slot in (1, 2):
        if int(got[slot]) == int(want[slot]):
            continue
        tok = int(want[slot])
        score = ref["s"][slot].astype(np.float64) - np.log(
            -np.log(ref["u"][slot].astype(np.float64)))
        best = score[ref["keep"][slot]].max()
        assert ref["keep"][slot, tok] and \
            score[tok] >= best - TIE_BAND * max(1.0, abs(best)), slot
    check_draw(logits.cpu(), ref, got, gpu.buf_logprob.cpu(),
               T=gpu.buf_temp_r.cpu())


# --------------------------------------------------------------- server


class _Ev:
    id = "ev"
    path = ""

    def __init__(self, inputs, max_tokens, **extra):
        self.body = {"inputs": inputs, "max_tokens": max_tokens, **extra}


@requires_gpu
def test_server_seeded_request_among_traffic():
    import concurrent.futures

    from mlrun_amd.models.llama import LlamaConfig, LlamaServer

    server = LlamaServer(name="s", config=LlamaConfig.tiny(), batch_size=4,
                         max_new_tokens=8, device="cuda:0",
                         scheduling="continuous", prefill="packed",
                         sampling="request")
    server.load()

    def ask(prompts, **fields):
        return server.do_event(_Ev(prompts, 8, **fields)).body

    mine = dict(temperature=5.0, top_p=0.95, seed=42, logprobs=True)
    try:
        with concurrent.futures.ThreadPoolExecutor(4) as pool:
            other = pool.submit(ask, [[400, 3, 3, 8, 1, 60, 14]],
                                temperature=1.0, seed=5)
            first = pool.submit(ask, [PROMPTS[0]], **mine).result(
                timeout=120)
            other.result(timeout=120)
        with concurrent.futures.ThreadPoolExecutor(4) as pool:
            others = [pool.submit(ask, [[7, 7, 21]]),
                      pool.submit(ask, [[1, 2], [9, 9, 9, 9]],
                                  temperature=2.0, top_k=10)]
            second = pool.submit(ask, [PROMPTS[0]], **mine).result(
                timeout=120)
            for future in others:
                future.result(timeout=120)
        lines = [json.loads(line) for line in server.do_event(
            _Ev([PROMPTS[0]], 8, stream=True, **mine)).body]
        stats = server.stats()
    finally:
        server.shutdown()
    assert len(first["outputs"][0]) == 8 and len(first["logprobs"][0]) == 8
    assert first["outputs"] == second["outputs"]
    assert first["logprobs"] == second["logprobs"]
    assert [line["token"] for line in lines] == first["outputs"][0]
    assert [line["logprob"] for line in lines] == first["logprobs"][0]
    assert stats["sampling"]["requests"] == 6
