# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""The two bit-exact decode fusions against the kernel pairs they
replace, compared with `torch.equal` on the GPU:

- `fused_add_rmsnorm_fold` (split-K slabs -> new residual + normed row)
  against `ops.skinny_gemm` (whose reduce_cast folds and rounds the same
  slabs) followed by `ops.fused_add_rmsnorm`;
- `skinny_gemm_swiglu` (variant-4 gate|up GEMM with the SwiGLU epilogue)
  against `ops.skinny_gemm(variant=4, ksplit=1)` + `ops.swiglu_fused`;
- a two-layer llama-3-8b-shaped engine stepping with
  MLRUN_DECODE_FUSE=none and with both fusions on the same weights.

Operands are interior slices of NaN-fenced buffers and outputs start as
NaN, so a row fetched from outside a tensor or an element left unwritten
shows, and the fences must come back untouched.

The ring of the variant-4 kernel is chosen by MLRUN_GEMM_LDS_RING, which
the extension reads once per process, so `test_swiglu_all_rings` re-runs
the SwiGLU cases in one child process per ring."""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = ("64x2", "64x3", "128x2")
PAD = 64        # fence elements on either side: keeps 16-byte alignment
EPS = 1e-5


class Fenced:
    """`values` (or NaN of `shape`) on the GPU inside a flat buffer that
    is NaN everywhere else: PAD elements on both sides, and `spare`
    elements of NaN capacity behind the values that belong to `.all`."""

    def __init__(self, values=None, shape=None, dtype=torch.bfloat16,
                 spare=0):
        if values is None:
            values = torch.full(shape, float("nan"), dtype=dtype)
        n = values.numel()
        flat = torch.full((PAD + n + spare + PAD,), float("nan"),
                          dtype=values.dtype)
        flat[PAD:PAD + n] = values.reshape(-1)
        self.buf = flat.cuda()
        self.n = n
        self.t = self.buf[PAD:PAD + n].view(values.shape)
        self.all = self.buf[PAD:PAD + n + spare]
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def intact(self):
        outside = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]])
        return bool(torch.isnan(outside).all())


def _randn(rows, cols, seed, std=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * std).to(torch.bfloat16)


def _ext():
    import mlrun_amd._hip_ops as ext

    return ext


# ------------------------------------------------------------- fold-norm

NORM_K = 512
ROWS = (1, 17, 32)
# 64 threads: 64 and 512; 256 threads: 2048 and 4096 (two chunks per
# thread, the decode shape); 2112 leaves 248 threads without a second
# chunk; 4160 is past two chunks per thread (the re-reading loop)
HIDDENS = (64, 512, 2048, 2112, 4096, 4160)
KSPLITS = (1, 2, 4)
# ksplit 3 and 8 run the instantiation with a run-time slab count
EXTRA = [(17, 2112, 3), (32, 4160, 8)]

_NORM_W = {}


def _norm_weights(hidden):
    """(GEMM weight [hidden, K], norm weight [hidden]), fenced, once."""
    if hidden not in _NORM_W:
        _NORM_W[hidden] = (Fenced(_randn(hidden, NORM_K, 5000 + hidden)),
                           Fenced(1 + _randn(1, hidden, 6000 + hidden,
                                             0.25).view(hidden)))
    return _NORM_W[hidden]


def _check_fold_norm(rows, hidden, ksplit):
    from mlrun_amd import ops

    w, nw = _norm_weights(hidden)
    a = Fenced(_randn(rows, NORM_K, 7000 + rows))
    residual = _randn(rows, hidden, 8000 + rows + hidden, 1.0)
    what = f"rows {rows} hidden {hidden} ksplit {ksplit}"

    # the unfused pair
    x = ops.skinny_gemm(a.t, w.t, ksplit=ksplit, variant=4)
    ref_res = residual.clone().cuda()
    ref_out = ops.fused_add_rmsnorm(x, nw.t, residual=ref_res, eps=EPS)

    slabs = Fenced(shape=(ksplit * rows * hidden,), dtype=torch.float32,
                   spare=hidden + 8)
    _ext().skinny_gemm_slabs(slabs.all, a.t, w.t, ksplit, 4)
    res = Fenced(residual)
    out = Fenced(shape=(rows, hidden))
    _ext().fused_add_rmsnorm_fold(out.t, res.t, slabs.all, nw.t, ksplit, EPS)
    torch.cuda.synchronize()
    assert not torch.isnan(out.t).any(), f"NaN left in out: {what}"
    assert torch.equal(res.t, ref_res), f"residual differs: {what}"
    assert torch.equal(out.t, ref_out), f"normed row differs: {what}"
    assert out.intact() and res.intact() and slabs.intact()
    assert torch.isnan(slabs.all[ksplit * rows * hidden:]).all()


@requires_gpu
@pytest.mark.parametrize("ksplit", KSPLITS)
@pytest.mark.parametrize("hidden", HIDDENS)
@pytest.mark.parametrize("rows", ROWS)
def test_fold_norm_bit_identical(rows, hidden, ksplit):
    _check_fold_norm(rows, hidden, ksplit)


@requires_gpu
@pytest.mark.parametrize("rows,hidden,ksplit", EXTRA)
def test_fold_norm_other_ksplits(rows, hidden, ksplit):
    _check_fold_norm(rows, hidden, ksplit)


def _raises(match, fn, *args):
    with pytest.raises(ValueError, match=match):
        fn(*args)


@requires_gpu
def test_fold_norm_bad_arguments_raise_before_any_launch():
    rows, hidden, ksplit = 3, 64, 2
    residual = _randn(rows, hidden, 1)
    out = torch.full((rows, hidden), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    res = residual.cuda()
    slabs = torch.ones(ksplit * rows * hidden, device="cuda")
    weight = torch.ones(hidden, dtype=torch.bfloat16, device="cuda")
    fn = _ext().fused_add_rmsnorm_fold
    good = [out, res, slabs, weight, ksplit, EPS]

    def bad(match, index, value):
        args = list(good)
        args[index] = value
        _raises(match, fn, *args)

    bad("out must be on GPU", 0, out.cpu())
    bad("out must be bf16", 0, out.float())
    bad("out must have 2 dimensions", 0, out.view(-1))
    bad("residual not contiguous", 1,
        residual.t().contiguous().cuda().t())
    bad("residual size", 1, res[:2].contiguous())
    bad("slabs must be f32", 2, slabs.double())
    bad("slabs too small", 2, slabs[:-1])
    bad("weight size", 3, torch.cat([weight, weight[:8]]))
    bad("weight must be bf16", 3, weight.float())
    bad("ksplit must be", 4, 0)
    bad("slabs too small", 4, ksplit + 1)
    _raises("rows must be", fn, out.new_empty(65, hidden),
            res.new_empty(65, hidden), slabs.new_empty(2 * 65 * hidden),
            weight, ksplit, EPS)
    _raises("hidden must be a multiple of 8", fn, out.new_empty(rows, 60),
            res.new_empty(rows, 60), slabs, weight[:60], ksplit, EPS)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert torch.equal(res.cpu(), residual)


# -------------------------------------------------------- SwiGLU epilogue

# K = 160: waves get 64/64/32/0 k, wave 3 is empty; 256: exactly one
# 64-k stage per wave; 1056: whole stages and a 32-k tail (288 per wave).
# inter 40 ends in a partial tile: its last workgroup has 8 live columns.
SWIGLU_CASES = [(m, inter, k) for m in (17, 32) for inter in (48, 40)
                for k in (160, 256, 1056)]


def _check_swiglu(m, inter, k):
    from mlrun_amd import ops

    a = Fenced(_randn(m, k, 1000 + m + k))
    wgu = Fenced(_randn(2 * inter, k, 2000 + inter + k))
    gu = ops.skinny_gemm(a.t, wgu.t, ksplit=1, variant=4)
    ref = ops.swiglu_fused(gu)
    act = Fenced(shape=(m, inter))
    _ext().skinny_gemm_swiglu(act.t, a.t, wgu.t)
    torch.cuda.synchronize()
    what = f"M {m} inter {inter} K {k}"
    assert not torch.isnan(act.t).any(), f"NaN left in act: {what}"
    assert torch.equal(act.t, ref), \
        f"epilogue != GEMM + swiglu_fused at {what}: " \
        f"{(act.t.float() - ref.float()).abs().max().item()}"
    assert act.intact()


@requires_gpu
@pytest.mark.parametrize("m,inter,k", SWIGLU_CASES)
def test_swiglu_epilogue_bit_identical(m, inter, k):
    _check_swiglu(m, inter, k)


@requires_gpu
def test_swiglu_epilogue_bad_arguments_raise_before_any_launch():
    inter, k = 48, 256
    wgu = _randn(2 * inter, k, 3).cuda()
    fn = _ext().skinny_gemm_swiglu
    acts = []

    def args(m):
        acts.append(torch.full((m, inter), float("nan"),
                               dtype=torch.bfloat16, device="cuda"))
        return [acts[-1], _randn(m, k, 4).cuda(), wgu]

    for m in (16, 33):
        _raises("16 < M <= 32", fn, *args(m))

    def bad(match, index, value):
        call = args(32)
        call[index] = value(call[index]) if callable(value) else value
        _raises(match, fn, *call)

    bad("act must be on GPU", 0, lambda t: t.cpu())
    bad("act must be bf16", 0, lambda t: t.float())
    bad("act rows", 0, lambda t: t[:31].contiguous())
    bad("2 \\* inter rows", 0, lambda t: t[:, :40].contiguous())
    bad("a must be bf16", 1, lambda t: t.float())
    bad("a not contiguous", 1, lambda t: t.t().contiguous().t())
    bad("K mismatch", 1, lambda t: t[:, :k - 32].contiguous())
    bad("wgu must be on GPU", 2, lambda t: t.cpu())
    bad("wgu must have 2 dimensions", 2, lambda t: t.view(-1))
    _raises("inter must be a multiple of 8", fn,
            torch.empty(32, 44, dtype=torch.bfloat16, device="cuda"),
            _randn(32, k, 4).cuda(), wgu[:88].contiguous())
    _raises("K must be a multiple of 32", fn,
            torch.empty(32, inter, dtype=torch.bfloat16, device="cuda"),
            _randn(32, 48, 4).cuda(), wgu[:, :48].contiguous())
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in acts)


def _run_swiglu_cases():
    for case in SWIGLU_CASES:
        _check_swiglu(*case)


@requires_gpu
@pytest.mark.parametrize("ring", RINGS)
def test_swiglu_all_rings(ring):
    """Every SwiGLU case with the ring fixed by the environment knob."""
    env = dict(os.environ, MLRUN_GEMM_LDS_RING=ring)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__)],
                          cwd=REPO, env=env, capture_output=True, text=True,
                          timeout=300)
    assert proc.returncode == 0 and f"ring ok {ring}" in proc.stdout, \
        f"ring {ring}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"


# ----------------------------------------------------------------- engine

@requires_gpu
def test_engine_steps_do_not_depend_on_the_knob(monkeypatch):
    """Two engines on one set of llama-3-8b-shaped weights (two layers:
    the projections' plans are the measured ones, wo / down split and
    gate|up on variant 4) step side by side without a graph, one with
    MLRUN_DECODE_FUSE=none and one with both fusions."""
    from mlrun_amd.models.llama import LlamaConfig, LlamaDecodeEngine

    monkeypatch.delenv("MLRUN_SLAB_MODE", raising=False)
    B, steps = 32, 4
    cfg = LlamaConfig.llama3_8b(num_layers=2, vocab_size=2048,
                                max_seq_len=64)
    plain = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                              use_graph=False)
    fused = LlamaDecodeEngine(cfg, batch_size=B, device="cuda:0",
                              use_graph=False, weights=plain.weights)
    layer = plain.weights.layers[0]
    assert fused._plan(layer["wgu"]) == (1, 4)
    assert fused._plan(layer["wo"])[0] > 1
    assert fused._plan(layer["wdown"])[0] > 1
    prompt = torch.randint(0, cfg.vocab_size, (B, 9),
                           generator=torch.Generator().manual_seed(0))
    for engine in (plain, fused):
        logits = engine.prefill(prompt)
        engine.buf_tokens.copy_(logits.argmax(dim=-1))
    assert torch.equal(plain.buf_tokens, fused.buf_tokens)

    calls = {"fused_add_rmsnorm_fold": 0, "skinny_gemm_swiglu": 0}
    ext = _ext()
    for name in calls:
        real = getattr(ext, name)

        def counted(*args, _real=real, _name=name):
            calls[_name] += 1
            return _real(*args)

        monkeypatch.setattr(ext, name, counted)

    for step in range(steps):
        monkeypatch.setenv("MLRUN_DECODE_FUSE", "none")
        plain.decode_step()
        assert not any(calls.values())
        # the default is both fusions
        monkeypatch.delenv("MLRUN_DECODE_FUSE")
        fused.decode_step()
        torch.cuda.synchronize()
        # per layer: fold-norm after wo and after down, one gate|up GEMM
        assert calls == {"fused_add_rmsnorm_fold": 4,
                         "skinny_gemm_swiglu": 2}
        calls.update(dict.fromkeys(calls, 0))
        for name in ("buf_logits", "buf_tokens", "buf_residual",
                     "cache_lens"):
            assert torch.equal(getattr(plain, name), getattr(fused, name)), \
                f"{name} differs after step {step}"
        for li in range(cfg.num_layers):
            assert torch.equal(plain.k_cache[li], fused.k_cache[li])
            assert torch.equal(plain.v_cache[li], fused.v_cache[li])
    assert not torch.isnan(fused.buf_logits.float()).any()
    monkeypatch.setenv("MLRUN_DECODE_FUSE", "bogus")
    with pytest.raises(ValueError, match="MLRUN_DECODE_FUSE"):
        fused.decode_step()


if __name__ == "__main__":
    _run_swiglu_cases()
    print("ring ok", os.environ.get("MLRUN_GEMM_LDS_RING"))
