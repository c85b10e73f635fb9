# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Per-request seeded sampling on the CPU path: the Philox generator and
the semantics of ops.sample_tokens (statistics, edge cases, argument
checks), then sampling="request" in LlamaDecodeEngine and LlamaServer —
a request's tokens and logprobs depend on its prompt, seed and parameters
only, whatever the scheduler, prefill mode, slot or co-arriving traffic."""

import concurrent.futures
import json

import numpy as np
import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaServer, SamplingParams)


def _call(logits, pos, T, k, p, mp, seed):
    """ops.sample_tokens on python lists / scalars per row."""
    B = logits.shape[0]

    def vec(value, dtype):
        if not isinstance(value, (list, tuple, torch.Tensor)):
            value = [value] * B
        return torch.as_tensor(value).to(dtype).contiguous()

    tokens = torch.zeros(B, dtype=torch.int64)
    logprob = torch.zeros(B, dtype=torch.float32)
    kept = torch.zeros(B, dtype=torch.int32)
    out = ops.sample_tokens(
        logits, vec(pos, torch.int32), vec(T, torch.float32),
        vec(k, torch.int32), vec(p, torch.float32), vec(mp, torch.float32),
        vec(seed, torch.int64), tokens, logprob, kept)
    assert out is tokens
    return tokens, logprob, kept


# --------------------------------------------------------------- philox


def test_philox_known_answers():
    """The three Philox4x32-10 known-answer vectors (Random123)."""
    ones = 0xFFFFFFFF
    cases = [
        ((0, 0, 0, 0), (0, 0),
         (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((ones,) * 4, (ones,) * 2,
         (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
         (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for counter, key, want in cases:
        got = ops.philox4x32(counter, key)
        assert tuple(int(word) for word in got) == want
    # vectorised over counters: the same blocks
    both = ops.philox4x32((np.array([0, ones]), np.array([0, ones]),
                           np.array([0, ones]), np.array([0, ones])),
                          (np.array([0, ones]), np.array([0, ones])))
    assert tuple(int(word) for word in both[0]) == cases[0][2]
    assert tuple(int(word) for word in both[1]) == cases[1][2]


# ----------------------------------------------------------- statistics

# one fixed bf16 row at V = 16 (every value exact in bf16, no ties)
STAT_ROW = [0.5, -2.5, 3.0, 1.25, -1.0, 2.0, 0.0, 1.75, -0.5, 2.5, 0.25,
            -2.0, 1.5, 0.75, -1.5, 1.0]
SETTINGS = [(1.0, 0, 1.0, 0.0), (0.7, 5, 1.0, 0.0), (1.3, 0, 0.8, 0.0),
            (1.0, 0, 1.0, 0.1), (0.9, 8, 0.9, 0.05)]


def _exact_kept_probs(z, T, k, p, mp):
    """f64 kept mask and renormalised probabilities, written out
    independently of the op (no setting here sits near a boundary)."""
    z = np.asarray(z, dtype=np.float64)
    prob = np.exp(z / T - (z / T).max())
    prob /= prob.sum()
    keep = np.ones(len(z), dtype=bool)
    order = np.argsort(-z)
    if 0 < k < len(z):
        keep &= z >= z[order[k - 1]]
    if p < 1:
        tail = np.cumsum(prob[order])
        keep &= z >= z[order[np.argmax(tail >= p)]]
    if mp > 0:
        keep &= prob >= mp * prob.max()
    kept_prob = np.where(keep, prob, 0.0)
    return keep, kept_prob / kept_prob.sum()


@pytest.mark.parametrize("T,k,p,mp", SETTINGS)
def test_draws_follow_the_filtered_distribution(T, k, p, mp):
    """20480 draws (seeds 1000..1063 x positions 0..319): none outside
    the kept set, chi-square against the exact renormalised kept
    probabilities below the 1e-6 critical value.  The draws are
    deterministic, so the outcome is fixed."""
    from scipy.stats import chi2

    logits = torch.tensor([STAT_ROW] * 64).to(torch.bfloat16)
    seeds = list(range(1000, 1064))
    keep, prob = _exact_kept_probs(STAT_ROW, T, k, p, mp)
    counts = np.zeros(16, dtype=np.int64)
    for position in range(320):
        tokens, _, kept = _call(logits, position, T, k, p, mp, seeds)
        assert kept.tolist() == [int(keep.sum())] * 64
        counts += np.bincount(tokens.numpy(), minlength=16)
    assert counts.sum() == 20480
    assert counts[~keep].sum() == 0, "a draw fell outside the kept set"
    expected = prob[keep] * 20480
    assert expected.min() >= 5
    stat = float(((counts[keep] - expected) ** 2 / expected).sum())
    critical = float(chi2.isf(1e-6, int(keep.sum()) - 1))
    print(f"chi2 {stat:.2f} (df {int(keep.sum()) - 1}), critical "
          f"{critical:.1f}, smallest expected count {expected.min():.1f}")
    assert stat < critical


# ----------------------------------------------------------- edge cases


def _rand_logits(B, V, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=gen) * 3).to(torch.bfloat16)


class TestEdgeCases:
    def test_degenerate_settings_give_the_argmax(self):
        logits = _rand_logits(6, 1024)
        logits[:, 77] = 30.0  # a unique maximum
        for T, k, p, mp in [(0.0, 7, 0.5, 0.2), (1.5, 1, 1.0, 0.0),
                            (1.5, 0, 1e-6, 0.0), (1.5, 0, 1.0, 0.999999)]:
            tokens, logprob, kept = _call(logits, list(range(6)), T, k, p,
                                          mp, list(range(6)))
            assert tokens.tolist() == [77] * 6, (T, k, p, mp)
            assert kept.tolist() == [1] * 6
            want = torch.log_softmax(logits.float(), dim=-1)[:, 77]
            assert torch.allclose(logprob, want, atol=1e-5)

    def test_greedy_takes_the_lowest_index_on_ties(self):
        logits = torch.zeros(2, 16, dtype=torch.bfloat16)
        logits[0, [3, 9]] = 2.0
        logits[1, [15, 4]] = 1.0
        tokens, _, kept = _call(logits, 0, 0.0, 0, 1.0, 0.0, 0)
        assert tokens.tolist() == [3, 4] and kept.tolist() == [1, 1]

    def test_ties_at_the_kth_value_are_all_kept(self):
        row = [5.0, 4.0, 3.0, 3.0, 3.0, 1.0, 0.0, -1.0]
        logits = torch.tensor([row] * 4).to(torch.bfloat16)
        seen = set()
        for position in range(40):
            tokens, _, kept = _call(logits, position, 3.0, 3, 1.0, 0.0,
                                    [1, 2, 3, 4])
            assert kept.tolist() == [5] * 4  # > k = 3
            seen.update(tokens.tolist())
        assert seen == {0, 1, 2, 3, 4}

    def test_filters_off_keep_the_whole_vocabulary(self):
        logits = _rand_logits(3, 8)  # V = 8: one 16-byte vector
        tokens, _, kept = _call(logits, 5, 1.0, 0, 1.0, 0.0, 9)
        assert kept.tolist() == [8] * 3
        assert all(0 <= t < 8 for t in tokens.tolist())
        _, _, kept = _call(logits, 5, 1.0, 8, 1.0, 0.0, 9)  # k = V: off
        assert kept.tolist() == [8] * 3

    def test_counter_is_seed_and_position(self):
        logits = _rand_logits(1, 1024).repeat(4, 1)
        tokens, _, _ = _call(logits, [3, 3, 4, 3], 2.0, 0, 1.0, 0.0,
                             [11, 11, 11, 12])
        assert tokens[0] == tokens[1]
        assert len({int(t) for t in tokens[1:]}) == 3

    def test_negative_pos_rows_are_untouched(self):
        logits = _rand_logits(3, 64)
        args = [torch.tensor([0, -1, 2], dtype=torch.int32),
                torch.ones(3), torch.zeros(3, dtype=torch.int32),
                torch.ones(3), torch.zeros(3),
                torch.zeros(3, dtype=torch.int64)]
        tokens = torch.full((3,), -7, dtype=torch.int64)
        logprob = torch.full((3,), 123.0)
        kept = torch.full((3,), -7, dtype=torch.int32)
        ops.sample_tokens(logits, *args, tokens, logprob, kept)
        assert int(tokens[1]) == -7 and int(kept[1]) == -7
        assert float(logprob[1]) == 123.0
        assert kept[[0, 2]].tolist() == [64, 64]

    def test_bad_arguments_raise_before_any_work(self):
        def args(B=2, V=16):
            return dict(
                logits=torch.zeros(B, V, dtype=torch.bfloat16),
                pos=torch.zeros(B, dtype=torch.int32),
                temperature=torch.ones(B), top_k=torch.zeros(
                    B, dtype=torch.int32),
                top_p=torch.ones(B), min_p=torch.zeros(B),
                seed=torch.zeros(B, dtype=torch.int64),
                out_tokens=torch.zeros(B, dtype=torch.int64),
                out_logprob=torch.zeros(B),
                out_kept=torch.zeros(B, dtype=torch.int32))

        ops.sample_tokens(**args())  # the baseline is fine
        bad = [
            ("logits", lambda a: a["logits"].float()),            # dtype
            ("logits", lambda a: torch.zeros(                     # layout
                16, 2, dtype=torch.bfloat16).t()),
            ("logits", lambda a: a["logits"][0]),                 # 1-d
            ("V", lambda a: torch.zeros(2, 12, dtype=torch.bfloat16)),
            ("pos", lambda a: a["pos"].long()),
            ("pos", lambda a: torch.zeros(3, dtype=torch.int32)),
            ("temperature", lambda a: a["temperature"].double()),
            ("top_k", lambda a: a["top_k"].long()),
            ("top_p", lambda a: torch.ones(4)[::2]),
            ("min_p", lambda a: a["min_p"].half()),
            ("seed", lambda a: a["seed"].int()),
            ("out_tokens", lambda a: a["out_tokens"].int()),
            ("out_logprob", lambda a: torch.zeros(1)),
            ("out_kept", lambda a: a["out_kept"].long()),
        ]
        for name, make in bad:
            call = args()
            call["logits" if name == "V" else name] = make(call)
            with pytest.raises(ValueError, match=name):
                ops.sample_tokens(**call)
        with pytest.raises(ValueError, match="B must be <= 64"):
            ops.sample_tokens(**args(B=65))

    def test_out_of_range_parameters_give_the_argmax(self):
        """The op is total: a temperature whose division overflows
        (1.2e-38 is a normal f32, and 30 / 1.2e-38 is inf), a negative
        or NaN temperature, and min_p > 1 (nothing kept) all return the
        argmax with kept = 1, never an invalid token; top_p <= 0 keeps
        the maximum alone, as top_p -> 0+ does."""
        logits = _rand_logits(4, 1024)
        logits[:, 77] = 30.0  # a unique maximum
        want = torch.log_softmax(logits.float(), dim=-1)[:, 77]
        for T, k, p, mp in [(1.2e-38, 0, 1.0, 0.1), (1.2e-38, 0, 1.0, 0.0),
                            (1.2e-38, 5, 0.5, 0.1), (-1.0, 0, 1.0, 0.0),
                            (float("nan"), 3, 0.9, 0.1),
                            (1.5, 0, 1.0, 2.0), (1.5, 0, 0.0, 0.0),
                            (1.5, 0, -1.0, 0.0)]:
            tokens, logprob, kept = _call(logits, [0, 1, 2, 3], T, k, p,
                                          mp, [5, 6, 7, 8])
            assert tokens.tolist() == [77] * 4, (T, k, p, mp)
            assert kept.tolist() == [1] * 4, (T, k, p, mp)
            assert torch.allclose(logprob, want, atol=1e-5)

    def test_tiny_temperature_with_a_negative_maximum(self):
        """zmax / T = -inf is not finite either: greedy, lowest index."""
        logits = torch.full((1, 16), -9.0, dtype=torch.bfloat16)
        logits[0, [6, 11]] = -7.0
        tokens, _, kept = _call(logits, 0, 1.2e-38, 0, 1.0, 0.1, 1)
        assert tokens.tolist() == [6] and kept.tolist() == [1]


# --------------------------------------------------------------- engine


def _engine(B=4, **kwargs):
    return LlamaDecodeEngine(LlamaConfig.tiny(), B, device="cpu",
                             sampling="request", **kwargs)


class TestEngine:
    def test_defaults_are_greedy_and_match_the_engine_mode(self):
        tokens = torch.tensor([[5, 9, 2, 77], [400, 3, 3, 8]])
        want = LlamaDecodeEngine(LlamaConfig.tiny(), 2, device="cpu"
                                 ).generate(tokens, max_new_tokens=6)
        engine = _engine(2)
        got = engine.generate(tokens, max_new_tokens=6)
        assert torch.equal(got, want)
        assert engine.buf_kept.tolist() == [1, 1]

    def test_logprob_is_log_softmax_of_the_logits(self):
        engine = _engine(4)
        engine.set_sampling(1, temperature=5.0, seed=3)
        engine.set_sampling(2, temperature=0.8, top_k=20, top_p=0.9,
                            min_p=0.01, seed=4)
        tokens = torch.tensor([[5, 9, 2], [7, 7, 21], [1, 60, 14]])
        slots = torch.tensor([0, 1, 2])
        logits = engine.prefill_slots(tokens, slots)
        chosen = engine.buf_tokens[slots]
        want = torch.log_softmax(logits.float(), dim=-1).gather(
            1, chosen.view(3, 1)).view(3)
        assert torch.allclose(engine.buf_logprob[slots], want, atol=1e-5)
        for _ in range(3):
            engine.decode_step()
            want = torch.log_softmax(engine.buf_logits.float(), dim=-1
                                     ).gather(1, engine.buf_tokens.view(4, 1))
            assert torch.allclose(engine.buf_logprob, want.view(4),
                                  atol=1e-5)
        assert int(engine.buf_kept[0]) == 1
        assert int(engine.buf_kept[1]) == 1024

    def test_tokens_do_not_depend_on_slot_or_prefill_mode(self):
        """Same tokens and logprobs in any slot and after either
        prefill call."""
        prompt = [5, 9, 2, 77, 130]
        params = dict(temperature=5.0, top_p=0.95, seed=42)
        runs = []
        for slot, packed in [(0, False), (3, False), (2, True)]:
            engine = _engine(4)
            engine.set_sampling(slot, **params)
            other = (slot + 1) % 4
            engine.set_sampling(other, temperature=2.0, seed=slot)
            if packed:
                engine.prefill_packed([prompt, [8, 1]], [slot, other])
            else:
                engine.prefill_slots(torch.tensor([prompt]),
                                     torch.tensor([slot]))
            out = [(int(engine.buf_tokens[slot]),
                    float(engine.buf_logprob[slot]))]
            for _ in range(5):
                engine.decode_step()
                out.append((int(engine.buf_tokens[slot]),
                            float(engine.buf_logprob[slot])))
            runs.append(out)
        assert runs[0] == runs[1] == runs[2]

    def test_tiny_temperature_is_floored_and_gives_the_argmax(self):
        """A request may send any temperature >= 0: (0, 1e-4) is raised
        to 1e-4, and with min_p on the draw is the greedy token."""
        SamplingParams(temperature=1.2e-38, min_p=0.1).validate()
        tokens = torch.tensor([[5, 9, 2, 77], [400, 3, 3, 8]])
        want = _engine(2).generate(tokens, max_new_tokens=5)
        engine = _engine(2)
        engine.set_sampling(0, temperature=1.2e-38, min_p=0.1, seed=7)
        engine.set_sampling(1, temperature=5e-5, top_k=0, seed=8)
        assert engine.buf_temp_r.tolist() == pytest.approx([1e-4, 1e-4])
        got = engine.generate(tokens, max_new_tokens=5)
        assert torch.equal(got, want)
        engine.set_sampling(0, temperature=0.0)
        assert float(engine.buf_temp_r[0]) == 0.0

    def test_prompt_ids_outside_the_vocabulary_are_refused(self):
        """Checked on the host in every prefill call, so that no
        embedding gather reads outside the table on the device."""
        for engine in (_engine(2), LlamaDecodeEngine(
                LlamaConfig.tiny(), 2, device="cpu")):
            for bad in (1024, 10 ** 9, -1):
                tokens = torch.tensor([[5, bad, 2]])
                with pytest.raises(ValueError, match="token id outside"):
                    engine.prefill_slots(tokens, torch.tensor([1]))
                with pytest.raises(ValueError, match="token id outside"):
                    engine.prefill(tokens.repeat(2, 1))
                with pytest.raises(ValueError, match="token id outside"):
                    engine.prefill_packed(tokens.tolist(), [0])

    def test_refusals(self):
        cfg = LlamaConfig.tiny()
        with pytest.raises(ValueError, match="tp_size"):
            LlamaDecodeEngine(cfg, 2, device="cpu", tp_size=2,
                              sampling="request")
        with pytest.raises(ValueError, match="sampling"):
            LlamaDecodeEngine(cfg, 2, device="cpu", sampling="maybe")
        with pytest.raises(ValueError, match="batch_size"):
            LlamaDecodeEngine(cfg, 65, device="cpu", sampling="request")
        engine = _engine(2)
        with pytest.raises(ValueError, match='sampling="request"'):
            engine.generate_speculative(
                torch.zeros(2, 4, dtype=torch.int64), max_new_tokens=4)
        with pytest.raises(ValueError, match="top_p"):
            engine.set_sampling(0, top_p=0.0)
        with pytest.raises(ValueError, match="slot"):
            engine.set_sampling(2)
        plain = LlamaDecodeEngine(cfg, 2, device="cpu")
        with pytest.raises(ValueError, match="sampling"):
            plain.set_sampling(0, temperature=1.0)
        assert not hasattr(plain, "buf_logprob")


# --------------------------------------------------------------- server


class _Ev:
    id = "ev"
    path = ""

    def __init__(self, inputs, max_tokens, **extra):
        self.body = {"inputs": inputs, "max_tokens": max_tokens, **extra}


def _server(sampling="request", **kwargs):
    server = LlamaServer(name="s", config=LlamaConfig.tiny(), batch_size=4,
                         max_new_tokens=6, use_graph=False, device="cpu",
                         sampling=sampling, **kwargs)
    server.load()
    return server


def _ask(server, prompts, max_tokens=6, **fields):
    return server.do_event(_Ev(prompts, max_tokens, **fields)).body


SERVER_MODES = {
    "batch": dict(),
    "batcher": dict(batch_window_ms=20),
    "continuous": dict(scheduling="continuous"),
    "packed": dict(scheduling="continuous", prefill="packed"),
}

PROMPT = [5, 9, 2, 77, 130]
SAMPLED = dict(temperature=5.0, top_p=0.95, seed=42, logprobs=True)
FILTERED = dict(temperature=0.8, top_k=40, top_p=0.9, min_p=0.01, seed=7,
                logprobs=True)
# co-arriving traffic of other lengths: greedy and sampled
TRAFFIC = [([[400, 3, 3, 8, 1, 60, 14]], dict(temperature=1.0, seed=5)),
           ([[7, 7, 21]], dict()),
           ([[1, 2, 3, 4, 5]], dict(temperature=2.0, top_k=10, seed=9))]


@pytest.fixture(scope="module")
def mode_results():
    """The two seeded requests in every scheduling mode, alone and among
    concurrent traffic: {mode: [(alone, together), ...]}."""
    results = {}
    for mode, kwargs in SERVER_MODES.items():
        server = _server(**kwargs)
        try:
            pairs = []
            for fields in (SAMPLED, FILTERED):
                alone = _ask(server, [PROMPT], **fields)
                with concurrent.futures.ThreadPoolExecutor(8) as pool:
                    others = [pool.submit(_ask, server, prompts, **extra)
                              for prompts, extra in TRAFFIC[:2]]
                    mine = pool.submit(_ask, server, [PROMPT], **fields)
                    others.append(pool.submit(_ask, server, *TRAFFIC[2][:1],
                                              **TRAFFIC[2][1]))
                    together = mine.result(timeout=120)
                    for other in others:
                        other.result(timeout=120)
                pairs.append((alone, together))
            results[mode] = pairs
        finally:
            server.shutdown()
    return results


class TestServer:
    @pytest.mark.parametrize("mode", list(SERVER_MODES))
    def test_request_does_not_depend_on_traffic(self, mode_results, mode):
        for alone, together in mode_results[mode]:
            assert len(alone["outputs"][0]) == 6
            assert len(alone["logprobs"][0]) == 6
            assert alone["outputs"] == together["outputs"]
            assert alone["logprobs"] == together["logprobs"]

    def test_every_mode_serves_the_same_tokens(self, mode_results):
        first = mode_results["batch"]
        for mode, pairs in mode_results.items():
            for (want, _), (got, _) in zip(first, pairs):
                assert got["outputs"] == want["outputs"], mode

    def test_schedulers_serve_the_same_logprobs(self, mode_results):
        first = mode_results["batch"]
        for mode in ("batcher", "continuous"):
            for (want, _), (got, _) in zip(first, mode_results[mode]):
                assert got["logprobs"] == want["logprobs"], mode

    def test_prefill_modes_serve_the_same_logprobs(self, mode_results):
        """prefill="exact" against "packed": identical logprobs.  A
        sampling="request" engine prefills both ways through ONE
        attention code path (prefill_slots delegates to prefill_packed);
        two paths that agree only within the prefill bound
        (PREFILL_MAX_ERR in test_prefill_packed.py) gave logprobs up to
        3.9e-3 apart here."""
        worst = 0.0
        for (want, _), (got, _) in zip(mode_results["continuous"],
                                       mode_results["packed"]):
            for a, b in zip(want["logprobs"][0], got["logprobs"][0]):
                worst = max(worst, abs(a - b))
        print(f"largest |logprob difference| exact vs packed: {worst:.2e}")
        for (want, _), (got, _) in zip(mode_results["continuous"],
                                       mode_results["packed"]):
            assert got["logprobs"] == want["logprobs"]

    def test_greedy_request_matches_the_engine_mode(self):
        prompts = [PROMPT, [7, 7, 21]]
        plain = _server(sampling="engine")
        try:
            want = _ask(plain, prompts)["outputs"]
        finally:
            plain.shutdown()
        server = _server()
        try:
            body = _ask(server, prompts, temperature=0)
            assert body["outputs"] == want
            assert "logprobs" not in body
            assert _ask(server, prompts)["outputs"] == want  # defaults
        finally:
            server.shutdown()

    def test_seeds(self):
        server = _server()
        try:
            hot = dict(temperature=5, logprobs=True)
            one = _ask(server, [PROMPT], seed=1, **hot)
            two = _ask(server, [PROMPT], seed=2, **hot)
            assert one["outputs"] != two["outputs"]
            assert one == _ask(server, [PROMPT], seed=1, **hot)
            # prompt j draws with seed + j
            both = _ask(server, [PROMPT, PROMPT], seed=1, **hot)
            assert both["outputs"] == [one["outputs"][0], two["outputs"][0]]
            assert both["logprobs"] == [one["logprobs"][0],
                                        two["logprobs"][0]]
            # no seed: drawn per request
            free = [_ask(server, [PROMPT], temperature=5)["outputs"]
                    for _ in range(3)]
            assert free[0] != free[1] or free[1] != free[2]
        finally:
            server.shutdown()

    def test_constructor_values_are_the_defaults(self):
        server = _server(temperature=5.0, top_k=30, top_p=0.9, min_p=0.01)
        try:
            implicit = _ask(server, [PROMPT], seed=3, logprobs=True)
            explicit = _ask(server, [PROMPT], seed=3, logprobs=True,
                            temperature=5.0, top_k=30, top_p=0.9,
                            min_p=0.01)
            greedy = _ask(server, [PROMPT], seed=3, temperature=0)
        finally:
            server.shutdown()
        assert implicit == explicit
        assert implicit["outputs"] != greedy["outputs"]

    @pytest.mark.parametrize("mode", ["batch", "continuous"])
    def test_logprobs_are_trimmed_at_the_stop_token(self, mode):
        fields = dict(temperature=5, seed=11, logprobs=True)
        server = _server(**SERVER_MODES[mode])
        try:
            full = _ask(server, [PROMPT, [7, 7, 21]], **fields)
        finally:
            server.shutdown()
        stop = full["outputs"][0][2]
        cut = full["outputs"][0].index(stop) + 1
        server = _server(stop_token=stop, **SERVER_MODES[mode])
        try:
            body = _ask(server, [PROMPT, [7, 7, 21]], **fields)
        finally:
            server.shutdown()
        assert body["outputs"][0] == full["outputs"][0][:cut]
        assert body["logprobs"][0] == full["logprobs"][0][:cut]
        for row, logprobs in zip(body["outputs"], body["logprobs"]):
            assert len(row) == len(logprobs)
            assert all(value <= 0 for value in logprobs)

    def test_streaming_lines_carry_the_logprob(self):
        server = _server(scheduling="continuous")
        try:
            whole = _ask(server, [PROMPT], **SAMPLED)
            lines = [json.loads(line) for line in server.do_event(
                _Ev([PROMPT], 6, stream=True, **SAMPLED)).body]
            bare = [json.loads(line) for line in server.do_event(
                _Ev([PROMPT], 6, stream=True, temperature=5.0,
                    seed=42, top_p=0.95)).body]
        finally:
            server.shutdown()
        assert [line["token"] for line in lines] == whole["outputs"][0]
        assert [line["logprob"] for line in lines] == whole["logprobs"][0]
        assert [line["token"] for line in bare] == whole["outputs"][0]
        assert all("logprob" not in line for line in bare)

    def test_validation_names_the_field_and_fails_one_request(self):
        server = _server()
        try:
            bad = [("temperature", -0.5), ("temperature", "hot"),
                   ("top_k", -1), ("top_k", 2.5), ("top_p", 0),
                   ("top_p", 1.5), ("min_p", 1.0), ("min_p", -0.1),
                   ("seed", -1), ("seed", 2 ** 63), ("seed", 1.5),
                   ("logprobs", "yes")]
            for name, value in bad:
                with pytest.raises(ValueError, match=name):
                    _ask(server, [PROMPT], **{name: value})
            assert len(_ask(server, [PROMPT])["outputs"][0]) == 6
            stats = server.stats()
        finally:
            server.shutdown()
        assert stats == {"sampling": {"requests": 1, "sampled": 0,
                                      "greedy": 1}}

    def test_stats_count_requests(self):
        server = _server()
        try:
            _ask(server, [PROMPT, PROMPT], temperature=1.0)
            _ask(server, [PROMPT], temperature=0.5, top_k=5)
            _ask(server, [PROMPT])
            assert server.stats() == {"sampling": {
                "requests": 3, "sampled": 2, "greedy": 1}}
        finally:
            server.shutdown()

    def test_refused_combinations(self):
        cfg = LlamaConfig.tiny()
        with pytest.raises(ValueError, match="speculative"):
            LlamaServer(name="s", config=cfg, sampling="request",
                        speculative=2)
        with pytest.raises(ValueError, match="temperature"):
            LlamaServer(name="s", config=cfg, sampling="request",
                        temperature=-1)
        with pytest.raises(ValueError, match="top_p"):
            LlamaServer(name="s", config=cfg, sampling="request", top_p=0)
        with pytest.raises(ValueError, match="sampling"):
            LlamaServer(name="s", config=cfg, sampling="never")
        server = LlamaServer(name="s", config=cfg, batch_size=2,
                             device="cpu", use_graph=False,
                             sampling="request")
        server.speculative = 2
        with pytest.raises(ValueError, match="speculative"):
            server.load()

    def test_engine_mode_rejects_nothing_it_accepted(self):
        server = _server(sampling="engine")
        try:
            want = _ask(server, [PROMPT])
            odd = _ask(server, [PROMPT], temperature=-3, top_k="many",
                       top_p=7, min_p=-1, seed="x", logprobs="yes")
            assert server.stats() == {}
        finally:
            server.shutdown()
        assert odd == want and "logprobs" not in odd

    @pytest.mark.parametrize("prefill", ["exact", "packed"])
    def test_failed_admission_leaves_its_slots_greedy(self, prefill):
        """A prompt that fails at prefill (token id out of range) frees
        its slot with the sampling parameters back at the defaults."""
        server = _server(scheduling="continuous", prefill=prefill)
        try:
            with pytest.raises(Exception):
                _ask(server, [[10 ** 9]], temperature=2.0, top_p=0.5,
                     seed=3)
            engine = server.engines[0]
            assert engine.buf_temp_r.tolist() == [0.0] * 4
            assert engine.buf_top_p.tolist() == [1.0] * 4
            assert engine.buf_seed.tolist() == [0] * 4
            good = _ask(server, [PROMPT], **SAMPLED)
            assert len(good["outputs"][0]) == 6
        finally:
            server.shutdown()


def test_sampling_params_defaults():
    params = SamplingParams()
    assert (params.temperature, params.top_k, params.top_p, params.min_p,
            params.seed, params.logprobs) == (0.0, 0, 1.0, 0.0, 0, False)
    assert params.validate() is params
