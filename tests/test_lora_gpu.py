# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""GPU numerics of multi-LoRA serving: the lora_shrink / lora_expand HIP
kernels against the CPU references of the same ops, per-row adapters in
LlamaDecodeEngine (eager and under the captured graph) and one
LlamaServer run under continuous scheduling."""

import pytest
import torch

from test_lora import (MERGED_BOUND, _EngineRuns, check_parity,
                       check_row_independence, check_server_mixes_adapters,
                       int_case, lora_ids, save_adapters, _lora_server)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# bf16 result vs the fp32 reference (TestAttnDecode's bound)
ATOL = RTOL = 3e-2

BATCHES = [1, 5, 64]
RANKS = [8, 64]
# one lane, exactly one 64-lane x 8 sweep, a sweep plus a tail, one
# whole 256-lane workgroup sweep plus a tail, llama's longest
KS = [8, 512, 520, 2056, 14336]
# below, at and across a workgroup's 256-wide tile edge, llama's qkv
NS = [8, 256, 264, 6144]
NA = 3


def _rand_bf16(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16)


def _shrink_gpu(x, A, idx, fill=0.0):
    from mlrun_amd import ops

    t = torch.full((x.shape[0], A.shape[1]), fill, device="cuda")
    ops.lora_shrink(x.cuda(), A.cuda(), idx.cuda(), out=t)
    torch.cuda.synchronize()
    return t.cpu()


def _expand_gpu(y, t, Bm, idx):
    from mlrun_amd import ops

    out = ops.lora_expand(y.cuda(), t.cuda(), Bm.cuda(), idx.cuda())
    torch.cuda.synchronize()
    return out.cpu()


def _rows(idx, na):
    touched = [b for b, a in enumerate(idx.tolist()) if 0 <= a < na]
    skipped = [b for b in range(idx.numel()) if b not in touched]
    return touched, skipped


@requires_gpu
class TestLoraShrink:
    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("R", RANKS)
    def test_integer_exact(self, R, K):
        for B in BATCHES:
            case = int_case(B, R, K, 8, NA)
            got = _shrink_gpu(case["x"], case["A"], case["idx"], fill=7.5)
            touched, skipped = _rows(case["idx"], NA)
            assert torch.equal(got[touched], case["t_exp"][touched]), B
            assert (got[skipped] == 7.5).all(), B  # never written

    @pytest.mark.parametrize("K", KS)
    @pytest.mark.parametrize("R", RANKS)
    def test_random_within_f32_sum_bound(self, R, K):
        """|t_gpu - t_ref| <= 2 K 2^-24 sum_k |x_k a_jk| (sum in f64):
        the worst case of an f32 sum in any order."""
        from mlrun_amd import ops

        gen = torch.Generator().manual_seed(100 * R + K)
        A = _rand_bf16(NA, R, K, gen=gen)
        for B in BATCHES:
            x = _rand_bf16(B, K, gen=gen)
            idx = lora_ids(B, NA)
            ref = ops.lora_shrink(x, A, idx)
            got = _shrink_gpu(x, A, idx)
            touched, skipped = _rows(idx, NA)
            assert not got[skipped].any()
            for b in touched:
                a = int(idx[b])
                mag = A[a].double().abs() @ x[b].double().abs()
                bound = 2 * K * 2.0 ** -24 * mag
                err = (got[b].double() - ref[b].double()).abs()
                assert (err <= bound).all(), (B, b, err.max().item())

    def test_all_base_writes_nothing(self):
        case = int_case(5, 8, 512, 8, NA)
        idx = torch.full((5,), -1, dtype=torch.int32)
        got = _shrink_gpu(case["x"], case["A"], idx, fill=3.25)
        assert (got == 3.25).all()


@requires_gpu
class TestLoraExpand:
    @pytest.mark.parametrize("N", NS)
    @pytest.mark.parametrize("R", RANKS)
    def test_integer_exact(self, R, N):
        for B in BATCHES:
            case = int_case(B, R, 64, N, NA)
            t = case["t_exp"].clone()
            touched, skipped = _rows(case["idx"], NA)
            t[skipped] = float("nan")  # a skipped row's t is never read
            got = _expand_gpu(case["y0"], t, case["Bm"], case["idx"])
            assert torch.equal(got, case["y_exp"]), B
            assert torch.equal(got[skipped], case["y0"][skipped]), B

    @pytest.mark.parametrize("N", NS)
    @pytest.mark.parametrize("R", RANKS)
    def test_random_vs_reference(self, R, N):
        from mlrun_amd import ops

        gen = torch.Generator().manual_seed(100 * R + N)
        Bm = _rand_bf16(NA, N, R, scale=0.3, gen=gen)
        for B in BATCHES:
            y0 = _rand_bf16(B, N, gen=gen)
            t = torch.randn(B, R, generator=gen)
            idx = lora_ids(B, NA)
            ref = ops.lora_expand(y0.clone(), t, Bm, idx)
            got = _expand_gpu(y0, t, Bm, idx)
            touched, skipped = _rows(idx, NA)
            assert torch.isfinite(got.float()).all()
            assert torch.allclose(got.float(), ref.float(), atol=ATOL,
                                  rtol=RTOL), \
                (B, (got.float() - ref.float()).abs().max().item())
            # ids -1 and NA: bit-identical to the input
            assert torch.equal(got[skipped], y0[skipped])

    def test_all_base_leaves_y(self):
        case = int_case(5, 8, 64, 264, NA)
        idx = torch.full((5,), -1, dtype=torch.int32)
        got = _expand_gpu(case["y0"], case["t_exp"], case["Bm"], idx)
        assert torch.equal(got, case["y0"])


@requires_gpu
def test_unreferenced_nan_slots_stay_out():
    """Table slots that no row names may hold anything, NaN included."""
    from mlrun_amd import ops

    case = int_case(5, 8, 520, 264, NA)
    idx = torch.tensor([0, -1, 0, NA, 0], dtype=torch.int32)
    A, Bm = case["A"].clone(), case["Bm"].clone()
    A[1:] = float("nan")
    Bm[1:] = float("nan")
    t_ref = ops.lora_shrink(case["x"], case["A"], idx)
    y_ref = ops.lora_expand(case["y0"].clone(), t_ref, case["Bm"], idx)
    t = _shrink_gpu(case["x"], A, idx)
    y = _expand_gpu(case["y0"], t, Bm, idx)
    assert torch.isfinite(t).all() and torch.isfinite(y.float()).all()
    assert torch.equal(t, t_ref) and torch.equal(y, y_ref)


# -------------------------------------------------------------- engine


def _gpu_cfg():
    from mlrun_amd.models.llama import LlamaConfig

    return LlamaConfig.tiny(num_layers=2, num_heads=4, num_kv_heads=2,
                            hidden_size=512, intermediate_size=1024,
                            vocab_size=2048)


@pytest.fixture(scope="module")
def gpu_runs():
    return _EngineRuns(device="cuda:0", cfg=_gpu_cfg())


@requires_gpu
class TestEngineLoraGPU:
    def test_matches_merged_weights(self, gpu_runs):
        """The CPU recipe and bound on the GPU path (eager decode step
        on the HIP kernels).  Measured on an MI355X (profiles/README.md):
        0.0215 / 0.0234 after prefill, 0.0195 / 0.0221 after the decode
        step, against the bound of 0.0469."""
        check_parity(gpu_runs.runs)

    def test_row_independence(self, gpu_runs):
        check_row_independence(gpu_runs.runs)

    def test_graph_follows_buf_adapter(self, gpu_runs):
        """One captured graph, ids [0, -1, 1, 0]: same tokens as eager;
        then other ids WITHOUT recapturing: the replay follows them."""
        from mlrun_amd.models.llama import LlamaDecodeEngine

        eager = gpu_runs.engine
        graphed = LlamaDecodeEngine(gpu_runs.cfg, 4, device="cuda:0",
                                    use_graph=True, weights=eager.weights,
                                    lora=eager.lora)
        results = {}
        for ids in ([0, -1, 1, 0], [1, 1, -1, -1]):
            for name, engine in (("eager", eager), ("graph", graphed)):
                engine.reset()
                logits = engine.prefill(gpu_runs.tokens, adapters=ids)
                engine.buf_tokens.copy_(logits.argmax(dim=-1))
                if engine.use_graph:
                    engine.capture_graph()  # the first time only
                engine.decode_step()
                torch.cuda.synchronize()
                results[(name, tuple(ids))] = (
                    engine.buf_tokens.cpu().clone(),
                    engine.buf_logits.float().cpu().clone())
        assert graphed._graph is not None
        first, second = (0, -1, 1, 0), (1, 1, -1, -1)
        for ids in (first, second):
            tok_e, log_e = results[("eager", ids)]
            tok_g, log_g = results[("graph", ids)]
            assert torch.equal(tok_e, tok_g), ids
            assert (log_e - log_g).abs().max().item() <= MERGED_BOUND
        # every row changed its id, and the replay moved with each of
        # them: further than the two paths may differ, so a replay that
        # kept the captured ids could not have passed the check above
        moved = (results[("graph", second)][1] -
                 results[("graph", first)][1]).abs().amax(dim=-1)
        assert (moved > 2 * MERGED_BOUND).all(), moved
        assert moved.max().item() >= 20 * MERGED_BOUND, moved


@requires_gpu
def test_server_continuous_graph(tmp_path):
    server = _lora_server(save_adapters(tmp_path), device="cuda:0",
                          use_graph=True, scheduling="continuous")
    try:
        assert server.engines[0]._graph is not None
        check_server_mixes_adapters(server)
    finally:
        server.shutdown()
