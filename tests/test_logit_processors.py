# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""CPU checks of the logit processors: the reference branch of
ops.logit_processors rule by rule on hand-computed rows, its argument
checks, the new SamplingParams fields, and the logit_processors=True
engine and server on the tiny config."""

import concurrent.futures

import pytest
import torch

from mlrun_amd import ops
from mlrun_amd.models.llama import (LlamaConfig, LlamaDecodeEngine,
                                    LlamaServer, SamplingParams)

NB = ops.LOGIT_BIAS_MAX


def _bf16(values):
    return torch.tensor(values, dtype=torch.float32).to(torch.bfloat16)


def _apply(logits, state, penalties, bias=None, tokens=None, rows=None):
    """Run the op on copies; ``bias`` is one {id: value} per row.
    Returns (logits as f32 lists, state)."""
    logits = _bf16(logits).clone()
    B = logits.shape[0]
    state = torch.tensor(state, dtype=torch.int32)
    ids = torch.zeros(B, NB, dtype=torch.int32)
    val = torch.zeros(B, NB, dtype=torch.float32)
    cnt = torch.zeros(B, dtype=torch.int32)
    for b, entries in enumerate(bias or []):
        for j, (key, value) in enumerate(entries.items()):
            ids[b, j], val[b, j] = key, value
        cnt[b] = len(entries)
    out = ops.logit_processors(
        logits, state, torch.tensor(penalties, dtype=torch.float32), ids,
        val, cnt,
        None if tokens is None else torch.tensor(tokens, dtype=torch.int64),
        None if rows is None else torch.tensor(rows, dtype=torch.int32))
    assert out is logits
    return logits.float().tolist(), state


# state words: 0 = unseen, 1 = prompt only, 2 = generated once,
# 7 = generated three times and in the prompt
ROW = [2.0, -2.0, 0.0, 4.0, 4.0, -1.0, 3.0, 0.5]
SEEN = [2, 2, 2, 0, 1, 1, 7, 0]


class TestRules:
    def test_repetition_divides_positive_and_multiplies_the_rest(self):
        got, _ = _apply([ROW], [SEEN], [[2.0, 0.0, 0.0]])
        # z > 0: z / r; z <= 0 (zero included): z * r; unseen: untouched;
        # prompt-only tokens are penalised like generated ones
        assert got == [[1.0, -4.0, 0.0, 4.0, 2.0, -2.0, 1.5, 0.5]]

    def test_prompt_only_token_gets_no_presence_or_frequency(self):
        got, _ = _apply([ROW], [SEEN], [[1.0, 0.5, 0.25]])
        # n = 1: z - 0.25 - 0.5; n = 3: z - 0.75 - 0.5; n = 0: untouched
        assert got == [[1.25, -2.75, -0.75, 4.0, 4.0, -1.0, 1.75, 0.5]]

    def test_frequency_alone_and_presence_alone(self):
        got, _ = _apply([ROW, ROW], [SEEN, SEEN],
                        [[1.0, 0.0, 0.5], [1.0, 1.5, 0.0]])
        assert got[0] == [1.5, -2.5, -0.5, 4.0, 4.0, -1.0, 1.5, 0.5]
        assert got[1] == [0.5, -3.5, -1.5, 4.0, 4.0, -1.0, 1.5, 0.5]

    def test_bias_alone(self):
        got, state = _apply([ROW], [SEEN], [[1.0, 0.0, 0.0]],
                            bias=[{3: -100.0, 7: 2.5, 0: 0.25}])
        assert got == [[2.25, -2.0, 0.0, -96.0, 4.0, -1.0, 3.0, 3.0]]
        assert state.tolist() == [SEEN]

    def test_all_three_in_the_stated_order(self):
        got, _ = _apply([ROW], [SEEN], [[2.0, 0.5, 0.25]],
                        bias=[{6: 1.0, 1: -1.0, 3: 1.0}])
        # column 6: ((3 / 2) - 0.25 * 3) - 0.5 + 1 = 1.25
        # column 1: ((-2 * 2) - 0.25) - 0.5 - 1 = -5.75
        # column 0: (2 / 2) - 0.25 - 0.5 = 0.25; column 4: 4 / 2
        assert got == [[0.25, -5.75, -0.75, 5.0, 2.0, -2.0, 1.25, 0.5]]

    def test_results_round_to_nearest_even_at_bf16(self):
        # bf16 keeps 8 significant bits: near 1 the step is 2^-7
        up, tie_even, tie_odd = 2.0 ** -8 + 2.0 ** -10, 2.0 ** -8, 2.0 ** -8
        row = [1.0, 1.0, 1.0 + 2.0 ** -7, 3.0, 0, 0, 0, 0]
        got, _ = _apply([row], [[0] * 8], [[1.0, 0.0, 0.0]],
                        bias=[{0: up, 1: tie_even, 2: tie_odd}])
        assert got[0][0] == 1.0 + 2.0 ** -7      # above the tie: up
        assert got[0][1] == 1.0                  # tie: to the even 1.0
        assert got[0][2] == 1.0 + 2.0 ** -6      # tie: up to the even
        # 3 / 1.5 is exact; 1 / 3 rounds in f32, then in bf16
        got, _ = _apply([[1.0] * 8], [[1] * 8], [[3.0, 0.0, 0.0]])
        third = torch.tensor(1.0) / torch.tensor(3.0)
        assert got[0][0] == float(third.to(torch.bfloat16))

    def test_pending_token_is_counted_before_its_column(self):
        got, state = _apply([ROW], [SEEN], [[1.0, 0.0, 1.0]], tokens=[3])
        assert state.tolist() == [[2, 2, 2, 2, 1, 1, 7, 0]]
        assert got[0][3] == 3.0          # n = 1 in this very call
        got, state = _apply([ROW], [SEEN], [[1.0, 0.0, 1.0]], tokens=[6])
        assert state.tolist()[0][6] == 9 and got[0][6] == -1.0

    @pytest.mark.parametrize("token", [-1, 8, 2 ** 40])
    def test_pending_token_outside_the_vocabulary_is_ignored(self, token):
        got, state = _apply([ROW], [SEEN], [[2.0, 0.0, 0.0]],
                            tokens=[token])
        assert state.tolist() == [SEEN]
        assert got == [[1.0, -4.0, 0.0, 4.0, 2.0, -2.0, 1.5, 0.5]]

    def test_neutral_and_out_of_range_rows_are_left_alone(self):
        logits = [ROW, ROW, ROW, ROW]
        state = [SEEN, SEEN, SEEN]
        # row 0 neutral, rows 1 and 2 out of range,
        # row 3 live on state row 1
        penalties = [[1.0, 0.0, 0.0], [2.0, 1.0, 1.0], [2.0, 1.0, 1.0],
                     [1.0, 0.0, 1.0]]
        got, after = _apply(logits, state, penalties, tokens=[3, 3, 3, 3],
                            rows=[0, 3, -1, 1])
        assert got[:3] == [ROW, ROW, ROW]
        assert after.tolist() == [SEEN, [2, 2, 2, 2, 1, 1, 7, 0], SEEN]
        assert got[3] == [1.0, -3.0, -1.0, 3.0, 4.0, -1.0, 0.0, 0.5]

    def test_bias_count_is_clamped_and_bad_ids_are_ignored(self):
        logits = _bf16([ROW, ROW])
        state = torch.zeros(2, 8, dtype=torch.int32)
        ids = torch.full((2, NB), 5, dtype=torch.int32)
        ids[1, :3] = torch.tensor([-1, 8, 2])
        val = torch.full((2, NB), 1.0)
        ops.logit_processors(
            logits, state, torch.tensor([[1.0, 0.0, 0.0]] * 2), ids, val,
            torch.tensor([-5, 1000], dtype=torch.int32))
        assert logits[0].float().tolist() == ROW      # n < 0: neutral
        want = list(ROW)
        want[2] += 1.0
        want[5] += 1.0      # 61 duplicates of one id and value: applied once
        assert logits[1].float().tolist() == want


class TestArgumentChecks:
    def _args(self, B=2, V=16, S=2):
        return dict(
            logits=torch.zeros(B, V, dtype=torch.bfloat16),
            state=torch.zeros(S, V, dtype=torch.int32),
            penalties=torch.tensor([[1.0, 0.0, 0.0]] * B),
            bias_ids=torch.zeros(B, NB, dtype=torch.int32),
            bias_val=torch.zeros(B, NB),
            bias_n=torch.zeros(B, dtype=torch.int32),
            tokens=torch.zeros(B, dtype=torch.int64),
            rows=torch.zeros(B, dtype=torch.int32))

    @pytest.mark.parametrize("name, bad", [
        ("logits", torch.zeros(2, 16)),
        ("logits", torch.zeros(2, 12, dtype=torch.bfloat16)),
        ("logits", torch.zeros(16, dtype=torch.bfloat16)),
        ("logits", torch.zeros(2, 32, dtype=torch.bfloat16)[:, ::2]),
        ("state", torch.zeros(2, 16, dtype=torch.int64)),
        ("state", torch.zeros(2, 24, dtype=torch.int32)),
        ("penalties", torch.zeros(2, 2)),
        ("penalties", torch.zeros(2, 3, dtype=torch.float64)),
        ("bias_ids", torch.zeros(2, 32, dtype=torch.int32)),
        ("bias_val", torch.zeros(2, NB, dtype=torch.bfloat16)),
        ("bias_n", torch.zeros(3, dtype=torch.int32)),
        ("tokens", torch.zeros(2, dtype=torch.int32)),
        ("rows", torch.zeros(2, dtype=torch.int64)),
        ("rows", [0, 1]),
    ])
    def test_bad_arguments_are_value_errors(self, name, bad):
        args = self._args()
        args[name] = bad
        before = args["state"].clone()
        with pytest.raises(ValueError, match=name):
            ops.logit_processors(**args)
        if name != "state":
            assert torch.equal(args["state"], before)

    def test_too_many_rows(self):
        with pytest.raises(ValueError, match="B must be <= 64"):
            ops.logit_processors(**self._args(B=65))

    def test_constants(self):
        assert ops.LOGIT_BIAS_MAX == 64 and ops.LOGIT_TILE == 2048


class TestSamplingParams:
    def test_defaults_are_neutral_and_appended(self):
        params = SamplingParams()
        assert (params.repetition_penalty, params.presence_penalty,
                params.frequency_penalty, params.logit_bias) == \
            (1.0, 0.0, 0.0, None)
        assert params.validate() is params and params.neutral_processors()
        # positional construction of the earlier fields keeps working
        assert SamplingParams(0.5, 3, 0.9, 0.1, 7, True).logprobs is True

    @pytest.mark.parametrize("field, value", [
        ("repetition_penalty", 0.05), ("repetition_penalty", 10.5),
        ("repetition_penalty", "2"), ("repetition_penalty", float("nan")),
        ("presence_penalty", -2.5), ("presence_penalty", 3),
        ("presence_penalty", None), ("frequency_penalty", 2.01),
        ("frequency_penalty", True), ("logit_bias", [1, 2]),
        ("logit_bias", {"x": 1.0}), ("logit_bias", {-1: 1.0}),
        ("logit_bias", {1.5: 1.0}), ("logit_bias", {3: 101}),
        ("logit_bias", {3: "1"}), ("logit_bias", {3: float("nan")}),
        ("logit_bias", {3: 1.0, "3": 2.0}),
        ("logit_bias", {i: 0.0 for i in range(65)}),
    ])
    def test_validate_names_the_field(self, field, value):
        with pytest.raises(ValueError, match=field):
            SamplingParams(**{field: value}).validate()

    def test_accepted_values(self):
        params = SamplingParams(
            repetition_penalty=10, presence_penalty=-2,
            frequency_penalty=2.0,
            logit_bias={"17": -100, 5: 100.0, **{i: 0 for i in range(100,
                                                                      162)}})
        params.validate()
        assert params.bias_items()[:2] == [(17, -100.0), (5, 100.0)]
        assert not params.neutral_processors()


# --------------------------------------------------------------- engine

PROMPTS = torch.tensor([[5, 9, 2, 77], [400, 3, 3, 8], [7, 7, 7, 7]])


def _engine(B=3, flag=True, **kwargs):
    return LlamaDecodeEngine(LlamaConfig.tiny(), B, device="cpu",
                             use_graph=False, sampling="request",
                             logit_processors=flag, **kwargs)


def _recount(V, prompt, generated, counted=True):
    """The state row of one sequence: prompt bits, plus 2 per generated
    token while the row is counted."""
    row = torch.zeros(V, dtype=torch.int32)
    row[torch.tensor(prompt)] = 1
    for token in generated if counted else []:
        row[token] += 2
    return row


class TestEngine:
    def test_flag_needs_request_sampling(self):
        cfg = LlamaConfig.tiny()
        with pytest.raises(ValueError, match="logit_processors.*sampling"):
            LlamaDecodeEngine(cfg, 2, device="cpu", logit_processors=True)
        plain = _engine(2, flag=False)
        assert not hasattr(plain, "buf_tok_state")
        engine = _engine(2)
        assert engine.buf_tok_state.shape == (2, cfg.vocab_size)
        assert engine.buf_tok_state.dtype == torch.int32
        assert engine.buf_penalties.tolist() == [[1.0, 0.0, 0.0]] * 2
        assert engine.buf_bias_ids.shape == engine.buf_bias_val.shape == \
            (2, 64)
        assert engine.buf_bias_n.tolist() == [0, 0]

    @pytest.mark.parametrize("fields, name", [
        (dict(repetition_penalty=1.5), "repetition_penalty"),
        (dict(presence_penalty=0.5), "presence_penalty"),
        (dict(frequency_penalty=-0.5), "frequency_penalty"),
        (dict(logit_bias={3: 1.0}), "logit_bias"),
    ])
    def test_flag_off_engine_refuses_the_new_fields(self, fields, name):
        engine = _engine(2, flag=False)
        with pytest.raises(ValueError, match=name):
            engine.set_sampling_slots([0], [SamplingParams(**fields)])
        with pytest.raises(ValueError, match=name):
            engine.set_sampling(1, **fields)
        # neutral values pass, as before
        engine.set_sampling_slots([0], [SamplingParams(
            temperature=1.0, repetition_penalty=1.0, logit_bias={})])

    def test_set_sampling_writes_and_resets_the_buffers(self):
        engine = _engine(3)
        with pytest.raises(ValueError, match="logit_bias.*vocabulary"):
            engine.set_sampling(0, logit_bias={1024: 1.0})
        engine.set_sampling(1, repetition_penalty=1.5, presence_penalty=-1,
                            frequency_penalty=0.25,
                            logit_bias={"9": 2.0, 1023: -3.0})
        assert engine.buf_penalties.tolist() == [
            [1.0, 0.0, 0.0], [1.5, -1.0, 0.25], [1.0, 0.0, 0.0]]
        assert engine.buf_bias_n.tolist() == [0, 2, 0]
        assert engine.buf_bias_ids[1, :2].tolist() == [9, 1023]
        assert engine.buf_bias_val[1, :2].tolist() == [2.0, -3.0]
        engine.set_sampling_slots([1], [None])
        assert engine.buf_penalties.tolist() == [[1.0, 0.0, 0.0]] * 3
        assert engine.buf_bias_n.tolist() == [0, 0, 0]

    def test_a_bias_of_100_forces_the_token(self):
        engine = _engine(3)
        engine.set_sampling(0, logit_bias={321: 100})
        engine.set_sampling(2, temperature=1.0, seed=5,
                            logit_bias={"17": 100.0})
        out = engine.generate(PROMPTS, max_new_tokens=5)
        assert out[0].tolist() == [321] * 5
        assert out[2].tolist() == [17] * 5
        plain = _engine(3, flag=False).generate(PROMPTS, max_new_tokens=5)
        assert torch.equal(out[1], plain[1])

    def test_state_table_is_the_host_recount(self):
        engine = _engine(3)
        engine.set_sampling(0, repetition_penalty=1.3, presence_penalty=0.5)
        engine.set_sampling(1, temperature=1.5, seed=11,
                            frequency_penalty=1.0, logit_bias={8: -5.0})
        out = engine.generate(PROMPTS, max_new_tokens=6)
        V = engine.cfg.vocab_size
        # the last sampled token is pending: not counted yet
        for b in (0, 1):
            want = _recount(V, PROMPTS[b].tolist(), out[b, :-1].tolist())
            assert torch.equal(engine.buf_tok_state[b], want)
        # the neutral row holds its prompt bits and counts nothing
        assert torch.equal(engine.buf_tok_state[2], _recount(
            V, PROMPTS[2].tolist(), [], counted=False))
        # a new sequence in a slot starts from its own prompt alone
        engine.prefill_slots(torch.tensor([[1, 2, 3]]), torch.tensor([1]))
        assert torch.equal(engine.buf_tok_state[1],
                           _recount(V, [1, 2, 3], []))
        assert torch.equal(engine.buf_tok_state[0], _recount(
            V, PROMPTS[0].tolist(), out[0, :-1].tolist()))

    def test_penalties_change_what_greedy_decoding_repeats(self):
        engine = _engine(3)
        for slot in range(3):
            engine.set_sampling(slot, presence_penalty=2.0,
                                frequency_penalty=2.0,
                                repetition_penalty=10.0)
        out = engine.generate(PROMPTS, max_new_tokens=8)
        for b in range(3):
            row = out[b].tolist()
            assert len(set(row)) == len(row)
            assert not set(row) & set(PROMPTS[b].tolist())

    def test_neutral_engine_matches_an_engine_without_the_flag(self):
        runs = []
        for flag in (False, True):
            engine = _engine(3, flag=flag)
            engine.set_sampling(1, temperature=2.0, top_p=0.9, seed=3)
            tokens, logprobs = [], []
            engine.prefill(PROMPTS)
            for _ in range(5):
                tokens.append(engine.buf_tokens.clone())
                logprobs.append(engine.buf_logprob.clone())
                engine.decode_step()
            runs.append((torch.stack(tokens), torch.stack(logprobs)))
        assert torch.equal(runs[0][0], runs[1][0])
        assert torch.equal(runs[0][1], runs[1][1])

    def test_logprob_is_that_of_the_processed_logits(self):
        engine = _engine(3)
        engine.set_sampling(0, logit_bias={50: 6.0, 51: 6.0})
        engine.set_sampling(1, repetition_penalty=2.0)
        engine.prefill(PROMPTS)
        for _ in range(3):
            engine.decode_step()
            want = torch.log_softmax(engine.buf_logits.float(), dim=-1
                                     ).gather(1, engine.buf_tokens.view(3, 1))
            assert torch.allclose(engine.buf_logprob, want.view(3),
                                  atol=1e-5)

    def test_packed_continuation_keeps_the_earlier_prompt_bits(self):
        engine = _engine(3)
        V = engine.cfg.vocab_size
        engine.set_sampling(0, repetition_penalty=2.0)
        engine.set_sampling(2, repetition_penalty=2.0)
        engine.prefill_packed([[5, 9, 2], [30, 31]], [0, 2])
        assert torch.equal(engine.buf_tok_state[0], _recount(V, [5, 9, 2], []))
        # slot 0 continues its prefix, slot 2 starts a new sequence
        engine.prefill_packed([[77, 9], [40]], [0, 2], starts=[3, 0])
        assert torch.equal(engine.buf_tok_state[0],
                           _recount(V, [5, 9, 2, 77], []))
        assert torch.equal(engine.buf_tok_state[2], _recount(V, [40], []))
        assert int(engine.buf_tok_state[1].sum()) == 0


# --------------------------------------------------------------- server


class _Ev:
    id = "ev"
    path = ""

    def __init__(self, inputs, max_tokens, **extra):
        self.body = {"inputs": inputs, "max_tokens": max_tokens, **extra}


def _ask(server, prompts, max_tokens=5, **fields):
    return server.do_event(_Ev(prompts, max_tokens, **fields)).body


def _server(**kwargs):
    server = LlamaServer(name="s", config=LlamaConfig.tiny(), batch_size=4,
                         max_new_tokens=5, use_graph=False, device="cpu",
                         sampling="request", **kwargs)
    server.load()
    return server


SERVER_MODES = {"batch": dict(), "continuous": dict(scheduling="continuous")}


class TestServer:
    @pytest.mark.parametrize("mode", list(SERVER_MODES))
    def test_bias_forces_the_token_and_bad_bias_fails_alone(self, mode):
        server = _server(logit_processors=True, **SERVER_MODES[mode])
        try:
            assert server.engine.logit_processors
            plain = _ask(server, [[7, 7, 21]])["outputs"]
            with concurrent.futures.ThreadPoolExecutor(4) as pool:
                good = pool.submit(_ask, server, [[5, 9, 2, 77]],
                                   logit_bias={"321": 100})
                bad = [pool.submit(_ask, server, [[1, 2, 3]], **fields)
                       for fields in (dict(logit_bias={"1024": 1.0}),
                                      dict(logit_bias={"3": 1000}),
                                      dict(repetition_penalty=0.0))]
                other = pool.submit(_ask, server, [[7, 7, 21]])
                assert good.result(timeout=120)["outputs"] == [[321] * 5]
                assert other.result(timeout=120)["outputs"] == plain
                for future, name in zip(bad, ("logit_bias", "logit_bias",
                                              "repetition_penalty")):
                    with pytest.raises(ValueError, match=name):
                        future.result(timeout=120)
            # the freed slots are neutral again
            penalised = _ask(server, [[7, 7, 21]], presence_penalty=2.0,
                             frequency_penalty=2.0)["outputs"][0]
            assert len(set(penalised)) == 5
            assert _ask(server, [[7, 7, 21]])["outputs"] == plain
        finally:
            server.shutdown()

    def test_server_without_the_flag_does_not_read_the_fields(self):
        server = _server()
        try:
            plain = _ask(server, [[7, 7, 21]])["outputs"]
            got = _ask(server, [[7, 7, 21]], logit_bias={"321": 100},
                       repetition_penalty=99)["outputs"]
            assert got == plain
        finally:
            server.shutdown()

    def test_flag_needs_request_sampling(self):
        with pytest.raises(ValueError, match="logit_processors.*sampling"):
            LlamaServer(name="s", config=LlamaConfig.tiny(),
                        logit_processors=True)
