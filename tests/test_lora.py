# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Multi-LoRA serving on the CPU reference path: the lora_shrink /
lora_expand references, per-row adapters in LlamaDecodeEngine against an
engine with merged weights, LlamaServer(adapters=...) in every
scheduling mode, and LoRA fine-tuning in LlamaTrainer."""

import concurrent.futures

import pytest
import torch

import mlrun_amd
from mlrun_amd import ops
from mlrun_amd.models.llama import (LORA_PROJECTIONS, LlamaConfig,
                                    LlamaDecodeEngine, LlamaServer)
from mlrun_amd.models.llama_train import LlamaTrainer

# ----------------------------------------------------------------- ops


def lora_ids(B, NA):
    """Adapter ids of a B-row batch: the last slot, base (-1), a
    repeated id and NA itself (out of range: the row stays untouched)."""
    base = [NA - 1, -1, 0, 0, NA]
    return torch.tensor([base[b % len(base)] for b in range(B)],
                        dtype=torch.int32)


def int_case(B, R, K, N, NA=3, seed=0):
    """Integer-valued inputs whose products and sums are exact in bf16
    and f32, and the expected t and y written out from indexing alone.

    A is one-hot, A[a, j, (j * stride + a) % K] = 1, so
    t[b, j] = x[b, (j * stride + idx[b]) % K]; x in {-2..2}, Bm in
    {-1, 0, 1}, y0 in [-100, 100]: |y| <= 100 + 2 R <= 228 < 256."""
    gen = torch.Generator().manual_seed(seed)
    stride = max(K // R, 1)
    x = torch.randint(-2, 3, (B, K), generator=gen)
    Bm = torch.randint(-1, 2, (NA, N, R), generator=gen)
    y0 = torch.randint(-100, 101, (B, N), generator=gen)
    A = torch.zeros(NA, R, K)
    for a in range(NA):
        for j in range(R):
            A[a, j, (j * stride + a) % K] = 1
    idx = lora_ids(B, NA)
    t_exp = torch.zeros(B, R, dtype=torch.int64)
    y_exp = y0.clone()
    touched = []
    for b, a in enumerate(idx.tolist()):
        if not 0 <= a < NA:
            continue
        touched.append(b)
        for j in range(R):
            t_exp[b, j] = x[b, (j * stride + a) % K]
        y_exp[b] = y0[b] + (Bm[a] * t_exp[b].view(1, R)).sum(dim=1)
    return dict(x=x.to(torch.bfloat16), A=A.to(torch.bfloat16),
                Bm=Bm.to(torch.bfloat16), y0=y0.to(torch.bfloat16),
                idx=idx, t_exp=t_exp.float(),
                y_exp=y_exp.to(torch.bfloat16), touched=touched)


class TestLoraOpsReference:
    @pytest.mark.parametrize("R,K,N", [(8, 64, 40), (16, 8, 8),
                                       (64, 520, 264)])
    def test_integer_exact(self, R, K, N):
        case = int_case(5, R, K, N)
        sentinel = 12345.0
        t = torch.full((5, R), sentinel)
        out = ops.lora_shrink(case["x"], case["A"], case["idx"], out=t)
        assert out is t
        rows = case["touched"]
        assert rows == [0, 2, 3]
        assert torch.equal(t[rows], case["t_exp"][rows])
        skipped = [b for b in range(5) if b not in rows]
        assert (t[skipped] == sentinel).all()  # ids -1 and NA: no write
        y = case["y0"].clone()
        out = ops.lora_expand(y, t, case["Bm"], case["idx"])
        assert out is y
        assert torch.equal(y, case["y_exp"])
        assert torch.equal(y[skipped], case["y0"][skipped])
        assert not torch.equal(y[rows], case["y0"][rows])

    def test_shrink_allocates_f32(self):
        case = int_case(5, 8, 64, 40)
        t = ops.lora_shrink(case["x"], case["A"], case["idx"])
        assert t.dtype == torch.float32 and t.shape == (5, 8)
        rows = case["touched"]
        assert torch.equal(t[rows], case["t_exp"][rows])

    def test_one_rounding(self):
        """y + delta is rounded ONCE: 256 + 1 + 1 in f32 is 258, a bf16
        value; rounding after each term would leave 256."""
        x = torch.ones(1, 8, dtype=torch.bfloat16)
        A = torch.zeros(1, 8, 8, dtype=torch.bfloat16)
        A[0, 0, 0] = A[0, 1, 1] = 1
        Bm = torch.zeros(1, 8, 8, dtype=torch.bfloat16)
        Bm[0, 0, 0] = Bm[0, 0, 1] = 1
        idx = torch.zeros(1, dtype=torch.int32)
        y = torch.full((1, 8), 256.0, dtype=torch.bfloat16)
        ops.lora_expand(y, ops.lora_shrink(x, A, idx), Bm, idx)
        assert y[0, 0].item() == 258.0 and y[0, 1].item() == 256.0

    def test_value_errors(self):
        c = int_case(5, 8, 64, 40)
        x, A, Bm, idx, y = c["x"], c["A"], c["Bm"], c["idx"], c["y0"]
        t = torch.zeros(5, 8)
        bf16, f32 = torch.bfloat16, torch.float32
        bad_shrink = [
            (x.t().contiguous().t(), A, idx),           # non-contiguous
            (x.float(), A, idx),                        # dtype
            (x, A.float(), idx),
            (x, A, idx.long()),
            (torch.zeros(5, 12, dtype=bf16),            # K % 8
             torch.zeros(3, 8, 12, dtype=bf16), idx),
            (x, torch.zeros(3, 12, 64, dtype=bf16), idx),   # R
            (torch.zeros(65, 64, dtype=bf16), A,        # B > 64
             torch.zeros(65, dtype=torch.int32)),
        ]
        for args in bad_shrink:
            with pytest.raises(ValueError):
                ops.lora_shrink(*args)
        with pytest.raises(ValueError):
            ops.lora_shrink(x, A, idx, out=torch.zeros(5, 8, dtype=bf16))
        bad_expand = [
            (y.t().contiguous().t(), t, Bm, idx),
            (y.float(), t, Bm, idx),
            (y, t.to(bf16), Bm, idx),
            (y, t, Bm.float(), idx),
            (y, t, Bm, idx.long()),
            (torch.zeros(5, 12, dtype=bf16), t,         # N % 8
             torch.zeros(3, 12, 8, dtype=bf16), idx),
            (y, torch.zeros(5, 12, dtype=f32),          # R
             torch.zeros(3, 40, 12, dtype=bf16), idx),
            (torch.zeros(65, 40, dtype=bf16), torch.zeros(65, 8), Bm,
             torch.zeros(65, dtype=torch.int32)),
            (y, t, torch.zeros(3, 48, 8, dtype=bf16), idx),  # N mismatch
        ]
        for args in bad_expand:
            with pytest.raises(ValueError):
                ops.lora_expand(*args)


# -------------------------------------------------------------- engine

# Merged-vs-unmerged error of the recipe below, measured with this code
# on the CPU path for the two adapters: 0.0117 and 0.0098 after prefill
# (last-token logits), 0.0093 and 0.0100 after one decode step; the
# adapters move the logits by 1.37 to 1.63.  The bound is 4 x the largest
# error: the margin covers the merged weights' own bf16 rounding under
# another seed.
MERGED_ERR_MEASURED = 0.0117
MERGED_BOUND = 4 * MERGED_ERR_MEASURED

B_ENG, S_ENG, R_ENG = 4, 9, 8


def make_adapter(weights, r, gen, alpha=None, projs=LORA_PROJECTIONS,
                 layers=None, std_a=0.05, std_b=0.1):
    """A random adapter state for ``weights``: A ~ N(0, std_a),
    B ~ N(0, std_b), bf16, alpha = r unless given."""
    state = {"alpha": float(r if alpha is None else alpha)}
    layers = range(len(weights.layers)) if layers is None else layers
    for li in layers:
        for proj in projs:
            n, k = weights.layers[li][proj].shape
            state[f"layers.{li}.{proj}.lora_A"] = (
                torch.randn(r, k, generator=gen) * std_a
            ).to(torch.bfloat16)
            state[f"layers.{li}.{proj}.lora_B"] = (
                torch.randn(n, r, generator=gen) * std_b
            ).to(torch.bfloat16)
    return state


def merge_adapter(engine, source, slot):
    """engine.weights <- W + Bm A of ``source``'s table slot, in f32,
    rounded to bf16."""
    for li, layer in enumerate(engine.weights.layers):
        for proj in LORA_PROJECTIONS:
            a_tab, b_tab = source.lora.layers[li][proj]
            merged = layer[proj].float() + \
                b_tab[slot].float() @ a_tab[slot].float()
            layer[proj].copy_(merged.to(torch.bfloat16))


class _EngineRuns:
    """The engine recipe, run once and shared: tiny config, B = 4,
    S = 9, seed 7, two rank-8 adapters over all projections of both
    layers; prefill logits and the next decode step's buf_logits for
    homogeneous, all-base and mixed ids, and for merged engines."""

    def __init__(self, device="cpu", cfg=None, use_graph=False):
        gen = torch.Generator().manual_seed(7)
        cfg = cfg or LlamaConfig.tiny()
        self.cfg = cfg
        self.tokens = torch.randint(0, cfg.vocab_size, (B_ENG, S_ENG),
                                    generator=gen)
        self.engine = LlamaDecodeEngine(cfg, B_ENG, device=device,
                                        use_graph=use_graph,
                                        max_adapters=2, lora_rank=R_ENG)
        self.states = [make_adapter(self.engine.weights, R_ENG, gen)
                       for _ in range(2)]
        for slot, state in enumerate(self.states):
            self.engine.load_adapter(slot, state)
        self.runs = {}
        for name, ids in (("base", [-1] * 4), ("a0", [0] * 4),
                          ("a1", [1] * 4), ("mixed", [0, -1, 1, 0])):
            self.runs[name] = self.run(self.engine, ids)
        for slot in (0, 1):
            merged = LlamaDecodeEngine(cfg, B_ENG, device=device,
                                       use_graph=False)
            merge_adapter(merged, self.engine, slot)
            self.runs[f"merged{slot}"] = self.run(merged, None)

    def run(self, engine, ids):
        engine.reset()
        kwargs = {} if ids is None else {"adapters": ids}
        logits = engine.prefill(self.tokens, **kwargs)
        engine.buf_tokens.copy_(logits.argmax(dim=-1))
        engine.decode_step()
        return (logits.float().cpu().clone(),
                engine.buf_logits.float().cpu().clone())


@pytest.fixture(scope="module")
def engine_runs():
    return _EngineRuns()


def check_parity(runs):
    """Adapter vs merged engine within MERGED_BOUND, and far enough
    from the base model that a no-op implementation fails; prefill
    logits (stage 0) and the next decode step's buf_logits (stage 1)."""
    figures = {}
    for slot in (0, 1):
        for stage in (0, 1):
            got = runs[f"a{slot}"][stage]
            err = (got - runs[f"merged{slot}"][stage]).abs().max().item()
            moved = (got - runs["base"][stage]).abs().max().item()
            figures[(slot, stage)] = (err, moved)
            print(f"adapter {slot} stage {stage}: merged err {err:.5f} "
                  f"moved {moved:.4f}")
    for (slot, stage), (err, moved) in figures.items():
        assert err <= MERGED_BOUND, (slot, stage, err)
        assert moved >= 20 * MERGED_BOUND, (slot, stage, moved)
    return figures


def check_row_independence(runs):
    """ids [0, -1, 1, 0]: every row equals, bit for bit, the same row
    of its adapter's homogeneous run (or of the all-base run)."""
    for row, name in enumerate(["a0", "base", "a1", "a0"]):
        for stage in (0, 1):
            assert torch.equal(runs["mixed"][stage][row],
                               runs[name][stage][row]), (row, name, stage)


class TestEngineLora:
    def test_matches_merged_weights(self, engine_runs):
        check_parity(engine_runs.runs)

    def test_adapter_changes_argmax(self, engine_runs):
        runs = engine_runs.runs
        changed = runs["a0"][0].argmax(-1) != runs["base"][0].argmax(-1)
        assert changed.any()

    def test_row_independence(self, engine_runs):
        check_row_independence(engine_runs.runs)

    def test_prefill_variants_agree(self, engine_runs):
        """prefill_slots and prefill_packed with adapters= agree with
        prefill within the merged bound, and leave the same ids."""
        er = engine_runs
        ids = [0, -1, 1, 0]
        ref = er.runs["mixed"][0]
        er.engine.reset()
        got = er.engine.prefill_slots(er.tokens, torch.arange(B_ENG),
                                      adapters=ids)
        assert (got.float() - ref).abs().max().item() <= MERGED_BOUND
        assert er.engine.buf_adapter.tolist() == ids
        er.engine.reset()
        er.engine.buf_adapter.fill_(-1)
        # packed: slots in another order, the ids follow their prompts
        order = [2, 0, 3, 1]
        got = er.engine.prefill_packed(
            [er.tokens[i].tolist() for i in order], order,
            adapters=[ids[i] for i in order])
        err = (got.float() - ref[order]).abs().max().item()
        assert err <= MERGED_BOUND, err
        assert er.engine.buf_adapter.tolist() == ids
        moved = (got.float() - er.runs["base"][0][order]).abs().max()
        assert moved.item() >= 20 * MERGED_BOUND

    def test_no_adapters_means_no_buffers(self):
        engine = LlamaDecodeEngine(LlamaConfig.tiny(), 2, device="cpu")
        assert engine.lora is None and engine.max_adapters == 0
        assert not hasattr(engine, "buf_adapter")
        assert not hasattr(engine, "buf_lora_t")
        with pytest.raises(ValueError, match="max_adapters"):
            engine.load_adapter(0, {"alpha": 1.0})
        with pytest.raises(ValueError, match="max_adapters"):
            engine.prefill(torch.zeros(2, 4, dtype=torch.int64),
                           adapters=[0, -1])

    def test_buffers_and_sharing(self):
        cfg = LlamaConfig.tiny()
        first = LlamaDecodeEngine(cfg, 3, device="cpu", max_adapters=2,
                                  lora_rank=8)
        assert first.buf_adapter.dtype == torch.int32
        assert first.buf_adapter.tolist() == [-1, -1, -1]
        assert first.buf_lora_t.shape == (3, 8)
        assert first.buf_lora_t.dtype == torch.float32
        a_tab, b_tab = first.lora.layers[1]["wgu"]
        assert a_tab.shape == (2, 8, cfg.hidden_size)
        assert b_tab.shape == (2, 2 * cfg.intermediate_size, 8)
        assert not a_tab.any() and not b_tab.any()
        replica = LlamaDecodeEngine(cfg, 3, device="cpu",
                                    weights=first.weights, lora=first.lora)
        assert replica.lora is first.lora and replica.max_adapters == 2
        assert replica.buf_adapter is not first.buf_adapter

    def test_load_adapter_padding_partial_unload(self):
        cfg = LlamaConfig.tiny()
        engine = LlamaDecodeEngine(cfg, 2, device="cpu", max_adapters=2,
                                   lora_rank=8)
        gen = torch.Generator().manual_seed(3)
        # rank 4 in a rank-8 table, only wo and wdown of layer 1
        state = make_adapter(engine.weights, 4, gen, alpha=6.0,
                             projs=("wo", "wdown"), layers=[1])
        engine.load_adapter(1, state)
        a_tab, b_tab = engine.lora.layers[1]["wo"]
        assert torch.equal(a_tab[1, :4], state["layers.1.wo.lora_A"])
        assert not a_tab[1, 4:].any() and not a_tab[0].any()
        scaled = (state["layers.1.wo.lora_B"].float() * (6.0 / 4)
                  ).to(torch.bfloat16)
        assert torch.equal(b_tab[1, :, :4], scaled)
        assert not b_tab[1, :, 4:].any()
        for li, proj in ((0, "wo"), (1, "wqkv"), (1, "wgu")):
            a_tab, b_tab = engine.lora.layers[li][proj]
            assert not a_tab.any() and not b_tab.any()
        # the padded adapter equals its merged weights too
        tokens = torch.randint(0, cfg.vocab_size, (2, 5), generator=gen)
        got = engine.prefill(tokens, adapters=[1, 1]).float()
        base = engine.prefill(tokens).float()
        assert engine.buf_adapter.tolist() == [-1, -1]
        merged = LlamaDecodeEngine(cfg, 2, device="cpu")
        merge_adapter(merged, engine, 1)
        ref = merged.prefill(tokens).float()
        assert (got - ref).abs().max().item() <= MERGED_BOUND
        assert not torch.equal(got, base)
        engine.unload_adapter(1)
        for tables in engine.lora.layers:
            for a_tab, b_tab in tables.values():
                assert not a_tab.any() and not b_tab.any()
        again = engine.prefill(tokens, adapters=[1, 1]).float()
        assert torch.equal(again, base)

    def test_load_adapter_errors(self):
        cfg = LlamaConfig.tiny()
        engine = LlamaDecodeEngine(cfg, 2, device="cpu", max_adapters=1,
                                   lora_rank=8)
        gen = torch.Generator().manual_seed(4)
        good = make_adapter(engine.weights, 8, gen)
        bad = dict(good)
        bad["layers.1.wgu.lora_B"] = torch.zeros(7, 8)
        with pytest.raises(ValueError, match="layers.1.wgu.lora_B"):
            engine.load_adapter(0, bad)
        bad = dict(good)
        bad["layers.0.wo.lora_A"] = torch.zeros(8, 3)
        with pytest.raises(ValueError, match="layers.0.wo.lora_A"):
            engine.load_adapter(0, bad)
        # a failed load leaves the slot as it was
        assert not engine.lora.layers[0]["wo"][0].any()
        too_big = make_adapter(engine.weights, 16, gen)
        with pytest.raises(ValueError, match="rank 16"):
            engine.load_adapter(0, too_big)
        with pytest.raises(ValueError, match="slot"):
            engine.load_adapter(1, good)
        with pytest.raises(ValueError, match="alpha"):
            engine.load_adapter(0, {k: v for k, v in good.items()
                                    if k != "alpha"})
        with pytest.raises(ValueError, match="adapter id"):
            engine.prefill(torch.zeros(2, 4, dtype=torch.int64),
                           adapters=[0, 1])

    def test_refusals(self):
        cfg = LlamaConfig.tiny()
        with pytest.raises(ValueError, match="tp_size"):
            LlamaDecodeEngine(cfg, 2, device="cpu", tp_size=2,
                              max_adapters=1)
        with pytest.raises(ValueError, match="lora_rank"):
            LlamaDecodeEngine(cfg, 2, device="cpu", max_adapters=1,
                              lora_rank=12)
        engine = LlamaDecodeEngine(cfg, 2, device="cpu", max_adapters=1,
                                   lora_rank=8)
        engine.prefill(torch.zeros(2, 4, dtype=torch.int64))
        with pytest.raises(ValueError, match="max_adapters"):
            engine.verify_step(torch.zeros(2, 3, dtype=torch.int64))
        with pytest.raises(ValueError, match="max_adapters"):
            engine.generate_speculative(
                torch.zeros(2, 4, dtype=torch.int64), max_new_tokens=4)


# -------------------------------------------------------------- server


class _Ev:
    id = "ev"
    path = ""

    def __init__(self, inputs, max_tokens, **extra):
        self.body = {"inputs": inputs, "max_tokens": max_tokens, **extra}


def save_adapters(tmp_path, n=2, r=8, seed=21):
    """n random adapter state files for the tiny config."""
    weights = LlamaDecodeEngine(LlamaConfig.tiny(), 1,
                                device="cpu").weights
    gen = torch.Generator().manual_seed(seed)
    paths = {}
    for i in range(n):
        path = tmp_path / f"adapter{i}.pt"
        torch.save(make_adapter(weights, r, gen), str(path))
        paths[f"ad{i}"] = str(path)
    return paths


def _lora_server(adapters, device="cpu", use_graph=False, **kwargs):
    server = LlamaServer(name="s", config=LlamaConfig.tiny(),
                         batch_size=4, max_new_tokens=6,
                         use_graph=use_graph, device=device,
                         adapters=adapters, lora_rank=8, **kwargs)
    server.load()
    return server


# three requests of different prompt lengths: adapter 0, adapter 1, base
REQUESTS = [([[5, 9, 2, 77, 130]], "ad0"),
            ([[400, 3, 3, 8, 1, 60, 14]], "ad1"),
            ([[7, 7, 21]], None),
            ([[5, 9, 2, 77, 130]], "ad1")]


def _ask(server, prompts, name, **extra):
    if name is not None:
        extra["adapter"] = name
    return server.do_event(_Ev(prompts, 6, **extra)).body["outputs"]


def check_server_mixes_adapters(server):
    """Concurrent requests that mix both adapters and the base return
    what each returns alone; an unknown name fails only itself."""
    alone = [_ask(server, prompts, name) for prompts, name in REQUESTS]
    # the adapters matter: same prompt, different adapter or base
    base = _ask(server, REQUESTS[0][0], None)
    assert alone[0] != base and alone[3] != base and alone[0] != alone[3]
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        futures = [pool.submit(_ask, server, prompts, name)
                   for prompts, name in REQUESTS]
        bad = pool.submit(_ask, server, [[1, 2, 3]], "nope")
        together = [f.result(timeout=120) for f in futures]
        with pytest.raises(ValueError, match="ad0.*ad1"):
            bad.result(timeout=120)
    assert together == alone
    return alone


SERVER_MODES = {
    "batch": {},
    "batcher": {"batch_window_ms": 30},
    "continuous-exact": {"scheduling": "continuous"},
    "continuous-packed": {"scheduling": "continuous", "prefill": "packed"},
}


class TestServerLora:
    @pytest.mark.parametrize("mode", list(SERVER_MODES))
    def test_mixed_requests(self, tmp_path, mode):
        server = _lora_server(save_adapters(tmp_path), **SERVER_MODES[mode])
        try:
            check_server_mixes_adapters(server)
            stats = server.stats()
        finally:
            server.shutdown()
        assert stats["lora"]["adapters"] == ["ad0", "ad1"]
        # alone + together: ad0 twice, ad1 four times; the base and
        # the unknown name are not counted
        assert stats["lora"]["requests"] == {"ad0": 2, "ad1": 4}

    def test_modes_agree(self, tmp_path):
        """Every scheduling mode serves the same tokens."""
        paths = save_adapters(tmp_path)
        outs = []
        for kwargs in SERVER_MODES.values():
            server = _lora_server(paths, **kwargs)
            try:
                outs.append([_ask(server, prompts, name)
                             for prompts, name in REQUESTS])
            finally:
                server.shutdown()
        assert all(out == outs[0] for out in outs[1:])

    def test_streaming(self, tmp_path):
        import json

        server = _lora_server(save_adapters(tmp_path),
                              scheduling="continuous")
        try:
            prompts, name = REQUESTS[1]
            whole = _ask(server, prompts, name)
            lines = list(server.do_event(
                _Ev(prompts, 6, adapter=name, stream=True)).body)
        finally:
            server.shutdown()
        assert [json.loads(line)["token"] for line in lines] == whole[0]

    def test_matches_engine(self, tmp_path):
        """The server's tokens are the engine's with the same adapter."""
        paths = save_adapters(tmp_path)
        server = _lora_server(paths)
        try:
            got = _ask(server, REQUESTS[1][0], "ad1")
        finally:
            server.shutdown()
        engine = LlamaDecodeEngine(LlamaConfig.tiny(), 1, device="cpu",
                                   max_adapters=2, lora_rank=8)
        engine.load_adapter(1, torch.load(paths["ad1"],
                                          weights_only=True))
        want = engine.generate(torch.tensor(REQUESTS[1][0]),
                               max_new_tokens=6, adapters=[1])
        assert got == want.tolist()

    def test_speculative_conflict(self, tmp_path):
        paths = save_adapters(tmp_path, n=1)
        with pytest.raises(ValueError, match="speculative"):
            LlamaServer(name="s", config=LlamaConfig.tiny(),
                        adapters=paths, speculative=2)
        server = LlamaServer(name="s", config=LlamaConfig.tiny(),
                             batch_size=2, use_graph=False, device="cpu",
                             adapters=paths, lora_rank=8)
        server.speculative = 2
        with pytest.raises(ValueError, match="speculative"):
            server.load()

    def test_defaults(self, tmp_path):
        server = LlamaServer(name="s", config=LlamaConfig.tiny())
        assert server.adapters == {} and server.max_adapters == 0
        assert server.stats() == {}
        paths = save_adapters(tmp_path, n=2)
        server = LlamaServer(name="s", config=LlamaConfig.tiny(),
                             adapters=paths)
        assert server.max_adapters == 2
        with pytest.raises(ValueError, match="max_adapters"):
            LlamaServer(name="s", config=LlamaConfig.tiny(),
                        adapters=paths, max_adapters=1)

    def test_old_queue_items(self, tmp_path):
        """Queue items of the lengths used before adapters existed are
        still accepted, and run the base model."""
        for kwargs, item in (
                ({}, lambda f: ([[7, 7, 21]], 6, f)),
                ({"scheduling": "continuous"},
                 lambda f: ([7, 7, 21], 6, f)),
                ({"scheduling": "continuous"},
                 lambda f: ([7, 7, 21], 6, f, None, None))):
            server = _lora_server(save_adapters(tmp_path), **kwargs)
            try:
                want = _ask(server, [[7, 7, 21]], None)
                future = concurrent.futures.Future()
                server._tasks.put(item(future))
                got = future.result(timeout=120)
            finally:
                server.shutdown()
            assert got in (want, want[0])


# ------------------------------------------------------------- trainer


class TestTrainerLora:
    def test_trains_only_the_adapter(self):
        torch.manual_seed(5)
        cfg = LlamaConfig.tiny(vocab_size=256, max_seq_len=32)
        trainer = LlamaTrainer(cfg, device="cpu", lr=1e-2, lora_rank=4)
        assert trainer.lora_alpha == 8.0
        named = dict(trainer.model.named_parameters())
        lora_names = {n for n in named if ".lora_" in n}
        assert len(lora_names) == 2 * 4 * cfg.num_layers
        base_before = {n: p.detach().clone() for n, p in named.items()
                       if n not in lora_names}
        assert all(not named[n].requires_grad for n in base_before)
        opt_params = {id(p) for group in trainer.optimizer.param_groups
                      for p in group["params"]}
        assert opt_params == {id(named[n]) for n in lora_names}
        for name in lora_names:
            if name.endswith("lora_B"):
                assert not named[name].any()
            else:
                assert named[name].any()
        batch = torch.randint(0, 256, (2, 16),
                              generator=torch.Generator().manual_seed(6))
        losses = [trainer.train_step(batch) for _ in range(3)]
        assert losses[2] < losses[0], losses
        for name, before in base_before.items():
            assert torch.equal(named[name], before), name
        assert all(named[n].any() for n in lora_names
                   if n.endswith("lora_B"))
        state = trainer.adapter_state()
        assert state["alpha"] == 8.0
        assert state["layers.1.wgu.lora_A"].shape == (4, cfg.hidden_size)
        assert state["layers.1.wgu.lora_B"].shape == \
            (2 * cfg.intermediate_size, 4)

    def test_rank_zero_is_unchanged(self):
        cfg = LlamaConfig.tiny(vocab_size=128)
        trainer = LlamaTrainer(cfg, device="cpu")
        assert not any(".lora_" in n
                       for n, _ in trainer.model.named_parameters())
        assert all(p.requires_grad for p in trainer.model.parameters())
        with pytest.raises(ValueError, match="lora_rank"):
            trainer.adapter_state()

    def test_targets(self):
        cfg = LlamaConfig.tiny(vocab_size=128)
        trainer = LlamaTrainer(cfg, device="cpu", lora_rank=4,
                               lora_alpha=4, lora_targets=("wo",))
        keys = [k for k in trainer.adapter_state() if k.startswith("l")]
        assert sorted(keys) == ["layers.0.wo.lora_A", "layers.0.wo.lora_B",
                                "layers.1.wo.lora_A", "layers.1.wo.lora_B"]
        with pytest.raises(ValueError, match="lora_targets"):
            LlamaTrainer(cfg, device="cpu", lora_rank=4,
                         lora_targets=("q_proj",))

    def test_train_to_serve_round_trip(self, rundb):
        """save_adapter -> LlamaServer(adapters={"ft": uri}): the first
        served token is the argmax of the training model's logits.
        Rows whose top-1 margin is within the bf16 serving error cannot
        be compared token for token and are left out (not all of them
        may be)."""
        torch.manual_seed(11)
        cfg = LlamaConfig.tiny(vocab_size=512, max_seq_len=64)
        ctx = mlrun_amd.get_or_create_ctx("lora-ft")
        trainer = LlamaTrainer(cfg, device="cpu", lr=2e-2, lora_rank=4,
                               context=ctx)
        batch = torch.randint(0, 512, (2, 24))
        for _ in range(3):
            trainer.train_step(batch)
        base_art = trainer.save_checkpoint("base")
        adapter_art = trainer.save_adapter("ft")
        assert adapter_art.parameters["kind"] == "lora"
        assert adapter_art.parameters["rank"] == 4
        assert adapter_art.parameters["alpha"] == 8.0
        assert adapter_art.parameters["config"] == cfg.name

        prompts = torch.randint(0, 512, (4, 8),
                                generator=torch.Generator().manual_seed(2))
        with torch.no_grad():
            logits = trainer.model.eval()(prompts)[:, -1].float()
        top2 = logits.topk(2, dim=-1).values
        sure = (top2[:, 0] - top2[:, 1]) > 2 * MERGED_BOUND
        assert sure.any()
        server = LlamaServer(name="s", config=cfg, batch_size=4,
                             use_graph=False, device="cpu",
                             model_path=base_art.uri,
                             adapters={"ft": adapter_art.uri}, lora_rank=8)
        server.load()
        try:
            tuned = server.do_event(_Ev(prompts.tolist(), 1, adapter="ft")
                                    ).body["outputs"]
        finally:
            server.shutdown()
        want = logits.argmax(dim=-1).tolist()
        for row in range(4):
            if sure[row]:
                assert tuned[row][0] == want[row], row
        assert server.engines[0].lora.loaded == {0}
