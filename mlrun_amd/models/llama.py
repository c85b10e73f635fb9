# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Llama-family generative engine, decode-optimized for MI355X.

Design (MI355X-first, not a port — the reference has no model code):
- weights live as raw bf16 [N, K] tensors resident in HBM (288 GB:
  an 8B model + caches is ~6% of one GPU)
- the decode step runs entirely on hand-written CDNA4 kernels
  (mlrun_amd/ops: MFMA skinny GEMM, fused add+RMSNorm, RoPE, GQA
  decode attention, SwiGLU) with every buffer preallocated and the
  whole token step captured in ONE hipGraph (torch.cuda.CUDAGraph is
  hipGraph on ROCm) — per-token CPU cost is a single graph replay
- prefill batches through hipBLASLt (torch.matmul) + SDPA: it is
  compute-bound and library GEMMs are the right tool there
  (guide: hand-write the fused hot ops, use hipBLASLt for plain GEMMs)
- tensor parallelism (Llama-70B): row/col sharded projections with
  one RCCL all-reduce after attn-out and after mlp-down, over xGMI
"""

import math
import os
import typing
from dataclasses import dataclass

import torch

from .. import ops
from ..utils import logger
from .prefix_cache import PrefixIndex


@dataclass
class LlamaConfig:
    name: str = "llama-3-8b"
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    vocab_size: int = 128256
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    max_seq_len: int = 2048

    @classmethod
    def llama3_8b(cls, **over):
        return cls(**{**dict(name="llama-3-8b"), **over})

    @classmethod
    def llama3_70b(cls, **over):
        return cls(**{**dict(
            name="llama-3-70b", hidden_size=8192, intermediate_size=28672,
            num_layers=80, num_heads=64, num_kv_heads=8), **over})

    @classmethod
    def tiny(cls, **over):
        """Small config for CPU tests."""
        return cls(**{**dict(
            name="llama-tiny", hidden_size=256, intermediate_size=512,
            num_layers=2, num_heads=2, num_kv_heads=2, head_dim=128,
            vocab_size=1024, max_seq_len=256), **over})


class LlamaWeights:
    """Per-layer raw bf16 weight tensors ([N, K] row-major, matching
    the skinny-GEMM W layout).  TP sharding slices head/intermediate
    dims; each rank holds 1/tp of qkv+o+mlp weights."""

    def __init__(self, cfg: LlamaConfig, device, tp_rank=0, tp_size=1,
                 seed=1234):
        self.cfg = cfg
        self.device = device
        self.tp_rank = tp_rank
        self.tp_size = tp_size
        hq = cfg.num_heads // tp_size
        hkv = max(cfg.num_kv_heads // tp_size, 1)
        inter = cfg.intermediate_size // tp_size
        d, h = cfg.head_dim, cfg.hidden_size
        gen = torch.Generator(device="cpu").manual_seed(seed)

        def w(n, k, std=0.02):
            t = torch.empty(n, k, dtype=torch.bfloat16, device=device)
            t.normal_(0.0, std)
            return t

        # random-init on device (no network for checkpoints; see
        # BASELINE.md — synthetic data / random weights)
        torch.manual_seed(seed + tp_rank)
        self.embed = w(cfg.vocab_size, h)
        self.layers = []
        for _ in range(cfg.num_layers):
            self.layers.append({
                "attn_norm": torch.ones(h, dtype=torch.bfloat16,
                                        device=device),
                "wqkv": w((hq + 2 * hkv) * d, h),
                "wo": w(h, hq * d),
                "ffn_norm": torch.ones(h, dtype=torch.bfloat16,
                                       device=device),
                # fused gate|up: one [2*inter, h] GEMM per mlp
                "wgu": w(2 * inter, h),
                "wdown": w(h, inter),
            })
        self.final_norm = torch.ones(h, dtype=torch.bfloat16, device=device)
        self.lm_head = w(cfg.vocab_size, h)
        self.hq, self.hkv, self.inter = hq, hkv, inter

    def load_state_dict(self, state: dict):
        """Load a checkpoint saved by state_dict() — or a TRAINING
        checkpoint (LlamaForCausalLM.state_dict(), keys like
        "embed.weight"/"blocks.N..."), converted in place: artifacts
        logged by LlamaTrainer.save_checkpoint serve directly."""
        if "embed" not in state and "embed.weight" in state:
            state = _training_state_to_decode(state)
        self.embed.copy_(state["embed"])
        for i, layer in enumerate(self.layers):
            for key in layer:
                layer[key].copy_(state[f"layers.{i}.{key}"])
        self.final_norm.copy_(state["final_norm"])
        self.lm_head.copy_(state["lm_head"])

    def state_dict(self) -> dict:
        out = {"embed": self.embed, "final_norm": self.final_norm,
               "lm_head": self.lm_head}
        for i, layer in enumerate(self.layers):
            for key, value in layer.items():
                out[f"layers.{i}.{key}"] = value
        return out


def _training_state_to_decode(state: dict) -> dict:
    """Map a LlamaForCausalLM (training) state dict onto the decode
    weight layout (same mapping as llama_train.export_decode_state,
    duplicated here so serving never imports the training stack)."""
    out = {
        "embed": state["embed.weight"],
        "final_norm": state["final_norm.weight"],
        "lm_head": state["lm_head.weight"],
    }
    i = 0
    while f"blocks.{i}.attn_norm.weight" in state:
        prefix = f"blocks.{i}."
        out[f"layers.{i}.attn_norm"] = state[prefix + "attn_norm.weight"]
        out[f"layers.{i}.wqkv"] = state[prefix + "attn.wqkv.weight"]
        out[f"layers.{i}.wo"] = state[prefix + "attn.wo.weight"]
        out[f"layers.{i}.ffn_norm"] = state[prefix + "ffn_norm.weight"]
        out[f"layers.{i}.wgu"] = state[prefix + "mlp.wgu.weight"]
        out[f"layers.{i}.wdown"] = state[prefix + "mlp.wdown.weight"]
        i += 1
    return {k: v.to(torch.bfloat16) for k, v in out.items()}


LORA_PROJECTIONS = ("wqkv", "wo", "wgu", "wdown")


@dataclass
class SamplingParams:
    """How one prompt's tokens are chosen under ``sampling="request"``:
    the defaults are greedy with every filter off.  ``logprobs`` asks
    the server to return the chosen tokens' log-probabilities.

    The last four fields change the distribution a row samples from and
    need an engine built with ``logit_processors=True``; their defaults
    are neutral.  ``repetition_penalty`` r in [0.1, 10] divides the
    positive and multiplies the other logits of every token the prompt
    or the output holds; ``frequency_penalty`` f and ``presence_penalty``
    p in [-2, 2] subtract ``f * n + p`` from a token generated n > 0
    times; ``logit_bias`` maps at most 64 token ids (ints or decimal
    strings) to an addend in [-100, 100].  Applied in that order."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    seed: int = 0
    logprobs: bool = False
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: typing.Optional[dict] = None

    def bias_items(self):
        """logit_bias as [(token id, value)] with int ids; ValueError
        naming the field."""
        if self.logit_bias is None:
            return []
        if not isinstance(self.logit_bias, dict):
            raise ValueError("logit_bias must map token ids to numbers, "
                             f"got {self.logit_bias!r}")
        if len(self.logit_bias) > ops.LOGIT_BIAS_MAX:
            raise ValueError(f"logit_bias holds {len(self.logit_bias)} "
                             f"entries, at most {ops.LOGIT_BIAS_MAX}")
        items = {}
        for key, value in self.logit_bias.items():
            if isinstance(key, str) and key.isascii() and key.isdigit():
                key = int(key)
            if isinstance(key, bool) or not isinstance(key, int) or key < 0:
                raise ValueError("logit_bias keys must be token ids >= 0 "
                                 f"(ints or decimal strings), got {key!r}")
            if key in items:
                raise ValueError(f"logit_bias names token {key} twice")
            if isinstance(value, bool) or \
                    not isinstance(value, (int, float)) or \
                    not -100 <= value <= 100:
                raise ValueError("logit_bias values must be numbers in "
                                 f"[-100, 100], got {value!r} for token "
                                 f"{key}")
            items[key] = float(value)
        return list(items.items())

    def neutral_processors(self) -> bool:
        """Whether the four logit-processor fields leave logits alone."""
        return self.repetition_penalty == 1 and \
            self.presence_penalty == 0 and self.frequency_penalty == 0 \
            and not self.logit_bias

    def validate(self):
        """ValueError naming the field that is out of range."""
        def number(name, value):
            if isinstance(value, bool) or \
                    not isinstance(value, (int, float)) or \
                    value != value:
                raise ValueError(f"{name} must be a number, got {value!r}")

        def integer(name, value):
            if isinstance(value, bool) or not isinstance(value, int):
                raise ValueError(f"{name} must be an integer, got "
                                 f"{value!r}")

        number("temperature", self.temperature)
        if not 0 <= self.temperature < float("inf"):
            raise ValueError(f"temperature must be >= 0 and finite, got "
                             f"{self.temperature}")
        integer("top_k", self.top_k)
        if not 0 <= self.top_k < 2 ** 31:
            raise ValueError(f"top_k must be an integer >= 0, got "
                             f"{self.top_k}")
        number("top_p", self.top_p)
        if not 0 < self.top_p <= 1:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}")
        number("min_p", self.min_p)
        if not 0 <= self.min_p < 1:
            raise ValueError(f"min_p must be in [0, 1), got {self.min_p}")
        integer("seed", self.seed)
        if not 0 <= self.seed < 2 ** 63:
            raise ValueError(f"seed must be an integer in [0, 2^63), got "
                             f"{self.seed}")
        if not isinstance(self.logprobs, bool):
            raise ValueError(f"logprobs must be true or false, got "
                             f"{self.logprobs!r}")
        number("repetition_penalty", self.repetition_penalty)
        if not 0.1 <= self.repetition_penalty <= 10:
            raise ValueError("repetition_penalty must be in [0.1, 10], "
                             f"got {self.repetition_penalty}")
        for name in ("presence_penalty", "frequency_penalty"):
            number(name, getattr(self, name))
            if not -2 <= getattr(self, name) <= 2:
                raise ValueError(f"{name} must be in [-2, 2], got "
                                 f"{getattr(self, name)}")
        self.bias_items()
        return self


class LoraTables:
    """Adapter tables of a multi-LoRA engine: per layer and projection
    ``A [NA, R, K]`` and ``Bm [NA, N, R]`` bf16, zero-initialised and
    allocated once (a captured decode graph keeps their pointers).
    A slot holds one adapter; adapters of a smaller rank are zero-padded
    to R and ``alpha / r`` is folded into Bm.  Replica engines share one
    instance, like they share the weights."""

    def __init__(self, weights: LlamaWeights, max_adapters: int,
                 rank: int = 16):
        if rank not in ops.LORA_RANKS:
            raise ValueError(f"lora_rank must be one of {ops.LORA_RANKS}, "
                             f"got {rank}")
        if max_adapters < 1:
            raise ValueError("LoraTables needs max_adapters >= 1")
        self.max_adapters = int(max_adapters)
        self.rank = int(rank)
        self.weights = weights
        self.loaded = set()  # slots holding an adapter
        bf16 = dict(dtype=torch.bfloat16, device=weights.device)
        self.layers = []
        for layer in weights.layers:
            tables = {}
            for proj in LORA_PROJECTIONS:
                n, k = layer[proj].shape
                tables[proj] = (
                    torch.zeros(self.max_adapters, self.rank, k, **bf16),
                    torch.zeros(self.max_adapters, n, self.rank, **bf16))
            self.layers.append(tables)

    def _check_slot(self, slot):
        if not 0 <= int(slot) < self.max_adapters:
            raise ValueError(f"adapter slot {slot} outside "
                             f"[0, {self.max_adapters})")
        return int(slot)

    def unload(self, slot: int):
        slot = self._check_slot(slot)
        for tables in self.layers:
            for a_tab, b_tab in tables.values():
                a_tab[slot].zero_()
                b_tab[slot].zero_()
        self.loaded.discard(slot)

    @torch.no_grad()
    def load(self, slot: int, state: dict):
        """Validate the whole state first, then overwrite the slot."""
        slot = self._check_slot(slot)
        if "alpha" not in state:
            raise ValueError("adapter state has no 'alpha'")
        alpha = float(state["alpha"])
        pending = []
        seen = set()
        for key in state:
            if not key.startswith("layers."):
                continue
            parts = key.split(".")
            if len(parts) != 4 or not parts[1].isdigit() or \
                    parts[2] not in LORA_PROJECTIONS or \
                    parts[3] not in ("lora_A", "lora_B") or \
                    int(parts[1]) >= len(self.layers):
                raise ValueError(f"unexpected adapter key {key!r}")
            seen.add((int(parts[1]), parts[2]))
        for li, proj in sorted(seen):
            key_a = f"layers.{li}.{proj}.lora_A"
            key_b = f"layers.{li}.{proj}.lora_B"
            for key in (key_a, key_b):
                if key not in state:
                    raise ValueError(f"adapter state lacks {key!r}")
            mat_a, mat_b = state[key_a], state[key_b]
            n, k = self.weights.layers[li][proj].shape
            if mat_a.dim() != 2 or mat_a.shape[1] != k:
                raise ValueError(f"{key_a}: expected [r, {k}], got "
                                 f"{tuple(mat_a.shape)}")
            r = mat_a.shape[0]
            if not 1 <= r <= self.rank:
                raise ValueError(f"{key_a}: rank {r} outside "
                                 f"[1, lora_rank={self.rank}]")
            if tuple(mat_b.shape) != (n, r):
                raise ValueError(f"{key_b}: expected [{n}, {r}], got "
                                 f"{tuple(mat_b.shape)}")
            pending.append((li, proj, r, mat_a, mat_b))
        self.unload(slot)
        for li, proj, r, mat_a, mat_b in pending:
            a_tab, b_tab = self.layers[li][proj]
            a_tab[slot, :r].copy_(mat_a)
            # B * alpha / r in f32, ONE rounding to bf16
            scaled = mat_b.to(device=b_tab.device, dtype=torch.float32) \
                * (alpha / r)
            b_tab[slot, :, :r].copy_(scaled)
        self.loaded.add(slot)


class LlamaDecodeEngine:
    """Batched generation engine: prefill (hipBLASLt+SDPA) + hipGraph-
    captured decode step on the custom kernel chain.

    Multi-LoRA (``max_adapters > 0``): every cache slot carries an
    adapter id in ``buf_adapter`` (-1 = base model); the decode step adds
    each row's low-rank delta after the four projection GEMMs with the
    batched ``ops.lora_shrink`` / ``ops.lora_expand`` pair, so ONE
    captured graph serves rows of different adapters.  Single GPU, no
    speculative decoding."""

    def __init__(self, cfg: LlamaConfig, batch_size: int, device=None,
                 tp_group=None, tp_rank=0, tp_size=1, use_graph=True,
                 seed=1234, weights: "LlamaWeights" = None,
                 weight_dtype: str = "bf16", kv_dtype: str = "bf16",
                 temperature: float = 0.0, top_k: int = 0,
                 max_adapters: int = 0, lora_rank: int = 16,
                 lora: "LoraTables" = None, sampling: str = "engine",
                 logit_processors: bool = False,
                 prefix_cache_blocks: int = 0):
        if sampling not in ("engine", "request"):
            raise ValueError(f"unknown sampling mode {sampling!r} "
                             "(expected 'engine' or 'request')")
        if prefix_cache_blocks < 0:
            raise ValueError(
                f"prefix_cache_blocks={prefix_cache_blocks} is negative")
        if prefix_cache_blocks > 0 and kv_dtype == "fp8":
            raise ValueError(
                f"prefix_cache_blocks={prefix_cache_blocks} conflicts with "
                'kv_dtype="fp8": the cache fills slots through packed '
                "prefill, which needs a bf16 KV cache")
        if prefix_cache_blocks > 0 and tp_size > 1:
            raise ValueError(
                f"prefix_cache_blocks={prefix_cache_blocks} conflicts with "
                f"tp_size={tp_size}: the block pool is not sharded")
        if logit_processors and sampling != "request":
            raise ValueError(
                f"logit_processors=True needs sampling=\"request\", got "
                f"sampling={sampling!r}: penalties and logit bias are "
                "per-request parameters")
        if sampling == "request" and tp_size > 1:
            raise ValueError(
                f'sampling="request" conflicts with tp_size={tp_size}: '
                "per-request sampling runs on a single GPU")
        if sampling == "request" and batch_size > ops.SAMPLE_MAX_ROWS:
            raise ValueError(
                f'sampling="request" needs batch_size <= '
                f"{ops.SAMPLE_MAX_ROWS}, got {batch_size}")
        if (max_adapters > 0 or lora is not None) and tp_size > 1:
            raise ValueError(
                f"max_adapters={max_adapters} conflicts with tp_size="
                f"{tp_size}: LoRA adapters are not sharded")
        if (max_adapters > 0 or lora is not None) and \
                batch_size > ops.LORA_MAX_ROWS:
            raise ValueError(
                f"max_adapters > 0 needs batch_size <= "
                f"{ops.LORA_MAX_ROWS}, got {batch_size}")
        self.cfg = cfg
        self.B = batch_size
        self.device = torch.device(
            device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
        self.on_gpu = self.device.type == "cuda"
        self.tp_group = tp_group
        self.tp_rank = tp_rank
        self.tp_size = tp_size
        self.use_graph = use_graph and self.on_gpu
        # sampling: 0 = greedy argmax; otherwise Gumbel-max over
        # logits/T (graph-safe: torch captures RNG ops so every
        # replay draws fresh noise), optionally top-k restricted.
        # temperature < 0 enables PER-SLOT temperatures via buf_temp
        # (one graph serves mixed greedy/sampled requests: greedy
        # slots get a tiny T so the scaled logit gap swamps the noise)
        self.temperature = float(temperature)
        self.top_k = int(top_k)
        self.per_slot_temp = self.temperature < 0
        self.buf_temp = torch.full((batch_size, 1), 1e-4,
                                   dtype=torch.float32,
                                   device=self.device) \
            if self.per_slot_temp else None
        # weights are read-only at serving time: replica engines on the
        # same GPU share one copy (16 GB for 8B) and keep private
        # KV caches / buffers / streams
        self.weights = weights if weights is not None else \
            LlamaWeights(cfg, self.device, tp_rank, tp_size, seed)
        w = self.weights
        d, h = cfg.head_dim, cfg.hidden_size
        B, smax = batch_size, cfg.max_seq_len
        bf16 = dict(dtype=torch.bfloat16, device=self.device)

        # per-layer KV caches (per-rank kv heads): [L, B, Hkv, Smax, D].
        # kv_dtype="fp8": OCP e4m3 bytes + per-row f32 scales — halves
        # KV memory AND decode-attention HBM traffic (dequant happens
        # while staging chunks through LDS).
        self.kv_dtype = kv_dtype
        if kv_dtype == "fp8":
            u8 = dict(dtype=torch.uint8, device=self.device)
            self.k_cache = torch.zeros(cfg.num_layers, B, w.hkv, smax, d,
                                       **u8)
            self.v_cache = torch.zeros(cfg.num_layers, B, w.hkv, smax, d,
                                       **u8)
            f32 = dict(dtype=torch.float32, device=self.device)
            self.k_scale = torch.ones(cfg.num_layers, B, w.hkv, smax,
                                      **f32)
            self.v_scale = torch.ones(cfg.num_layers, B, w.hkv, smax,
                                      **f32)
        else:
            self.k_cache = torch.zeros(cfg.num_layers, B, w.hkv, smax, d,
                                       **bf16)
            self.v_cache = torch.zeros(cfg.num_layers, B, w.hkv, smax, d,
                                       **bf16)
            self.k_scale = self.v_scale = None
        self.cache_lens = torch.zeros(B, dtype=torch.int32,
                                      device=self.device)
        self.buf_positions = torch.zeros(B, dtype=torch.int32,
                                         device=self.device)
        self.cos_sin = ops.build_rope_cos_sin(smax, d, cfg.rope_theta,
                                              self.device)

        # preallocated decode buffers (graph-capture requirement)
        qkv_n = (w.hq + 2 * w.hkv) * d
        # split-K scratch: ksplit * B * N f32 for the largest case
        gemm_shapes = [(qkv_n, h), (h, w.hq * d), (2 * w.inter, h),
                       (h, w.inter), (cfg.vocab_size, h)]
        scratch = max(ops.pick_gemm_plan(B, n, k)[0] * n
                      for n, k in gemm_shapes)
        self.buf_tokens = torch.zeros(B, dtype=torch.int64,
                                      device=self.device)
        self.buf_hidden = torch.zeros(B, h, **bf16)
        self.buf_residual = torch.zeros(B, h, **bf16)
        self.buf_qkv = torch.zeros(B, qkv_n, **bf16)
        self.buf_attn_out = torch.zeros(B, w.hq * d, **bf16)
        self.buf_proj = torch.zeros(B, h, **bf16)
        self.buf_gu = torch.zeros(B, 2 * w.inter, **bf16)
        self.buf_act = torch.zeros(B, w.inter, **bf16)
        self.buf_down = torch.zeros(B, h, **bf16)
        self.buf_logits = torch.zeros(B, cfg.vocab_size, **bf16)
        # flat f32 split-K scratch (shared across all decode GEMMs)
        self.buf_c32 = torch.empty(B * scratch, dtype=torch.float32,
                                   device=self.device)
        self.scale = 1.0 / math.sqrt(d)
        self._capture_stream_ctx = None
        # opt-in fp8-weight decode: per-row e4m3 packs keyed by the
        # bf16 master tensor (prefill stays bf16/hipBLASLt; ~7.5 GB
        # extra for the packs on 8B — 288 GB HBM absorbs it)
        self.weight_dtype = weight_dtype
        self._fp8_packs = {}
        if weight_dtype == "fp8w" and self.on_gpu and tp_size == 1:
            max_k = max(h, w.inter, w.hq * d)
            self.buf_a8 = torch.empty(B * max_k, dtype=torch.uint8,
                                      device=self.device)
            self.buf_a_scale = torch.empty(B, dtype=torch.float32,
                                           device=self.device)
            # hidden quantized as a sidecar of the rmsnorm kernels —
            # qkv/gate-up/lm_head consume it without a quant launch
            self.buf_h8 = torch.empty(B, h, dtype=torch.uint8,
                                      device=self.device)
            self.buf_h8_scale = torch.empty(B, dtype=torch.float32,
                                            device=self.device)
            self.rebuild_fp8_packs()
        # fill-based (ns4 at B=32): the graph bakes ONE nsplit for all
        # context lengths, and decode mostly runs at S << max_seq_len —
        # measured (scripts/bench_attn_longctx.py): chunk-aware ns16
        # wins >=10% only at S>=1024 but costs 2.4% on the headline
        # (S~160).  Long-context deployments: pass seq_len to
        # pick_attn_nsplit / set MLRUN_ATTN_NSPLIT.
        _ns = os.environ.get("MLRUN_ATTN_NSPLIT")
        self.attn_nsplit = int(_ns) if _ns else \
            ops.pick_attn_nsplit(B, w.hkv)
        self.buf_attn_ws = torch.empty(
            B * w.hq * self.attn_nsplit * (d + 2), dtype=torch.float32,
            device=self.device) if self.on_gpu else None
        self._graph = None
        self._ksplits = {}
        # multi-LoRA (opt-in): shared adapter tables + per-slot ids.
        # With max_adapters == 0 nothing is allocated and the decode
        # step takes exactly the path it takes without this feature.
        if lora is None and max_adapters > 0:
            lora = LoraTables(w, max_adapters, lora_rank)
        self.lora = lora
        self.max_adapters = lora.max_adapters if lora is not None else 0
        if lora is not None:
            self.buf_adapter = torch.full((B,), -1, dtype=torch.int32,
                                          device=self.device)
            self.buf_lora_t = torch.zeros(B, lora.rank,
                                          dtype=torch.float32,
                                          device=self.device)
        # per-request sampling (opt-in): every slot carries its own
        # parameters in device buffers read by ops.sample_tokens, so one
        # captured graph serves rows that sample differently.  Defaults:
        # greedy, filters off.  With sampling == "engine" nothing is
        # allocated and _select_tokens picks the tokens as before.
        self.sampling = sampling
        if sampling == "request":
            dev = self.device
            self.buf_temp_r = torch.zeros(B, dtype=torch.float32, device=dev)
            self.buf_top_k = torch.zeros(B, dtype=torch.int32, device=dev)
            self.buf_top_p = torch.ones(B, dtype=torch.float32, device=dev)
            self.buf_min_p = torch.zeros(B, dtype=torch.float32, device=dev)
            self.buf_seed = torch.zeros(B, dtype=torch.int64, device=dev)
            self.buf_logprob = torch.zeros(B, dtype=torch.float32,
                                           device=dev)
            self.buf_kept = torch.zeros(B, dtype=torch.int32, device=dev)
        # logit processors (opt-in, on top of sampling="request"): per
        # slot the penalties, the bias entries and the token-state row
        # (2 * times generated + in prompt) that ops.logit_processors
        # reads and maintains between the lm_head GEMM and the sampler.
        # All neutral: such a row costs a workgroup exit.  With the flag
        # off nothing is allocated and the step launches what it did.
        self.logit_processors = bool(logit_processors)
        if self.logit_processors:
            dev, NB = self.device, ops.LOGIT_BIAS_MAX
            self.buf_tok_state = torch.zeros(B, cfg.vocab_size,
                                             dtype=torch.int32, device=dev)
            self.buf_penalties = torch.tensor(
                [[1.0, 0.0, 0.0]] * B, dtype=torch.float32).to(dev)
            self.buf_bias_ids = torch.zeros(B, NB, dtype=torch.int32,
                                            device=dev)
            self.buf_bias_val = torch.zeros(B, NB, dtype=torch.float32,
                                            device=dev)
            self.buf_bias_n = torch.zeros(B, dtype=torch.int32, device=dev)
        # speculative decoding (opt-in): running acceptance counters
        self.spec_stats = {"steps": 0, "drafted": 0, "accepted": 0}
        # prefix cache (opt-in): a pool of 32-token KV blocks
        # [L, N, Hkv, 32, D] kept between requests, and the host index
        # that names their content.  prefill_cached copies hit blocks
        # into the slot and prefills the rest.  At 0 nothing is allocated.
        self.prefix_index = None
        self.pc_k = self.pc_v = None
        if prefix_cache_blocks > 0:
            if not self._packed_prefill_serves():
                raise ValueError(
                    f"prefix_cache_blocks={prefix_cache_blocks} conflicts "
                    f"with head_dim={d} and {w.hq}/{w.hkv} q/kv heads: "
                    "packed prefill serves head_dim 128 and at most 8 "
                    "q-heads per KV head")
            self.prefix_index = PrefixIndex(prefix_cache_blocks)
            self.pc_k = torch.zeros(cfg.num_layers, prefix_cache_blocks,
                                    w.hkv, ops.KV_BLOCK_TOKENS, d, **bf16)
            self.pc_v = torch.zeros_like(self.pc_k)

    # ---------------------------------------------------- prefix cache
    def clear_prefix_cache(self):
        """Forget every cached prefix (the pool's memory stays)."""
        if self.prefix_index is not None:
            self.prefix_index.clear()

    @property
    def prefix_stats(self) -> dict:
        """Counters of the prefix cache: lookups, prompt_tokens,
        hit_tokens, inserted, evicted, blocks_in_use, capacity."""
        if self.prefix_index is None:
            raise ValueError("engine built with prefix_cache_blocks=0 "
                             "holds no prefix cache")
        return self.prefix_index.stats()

    # -------------------------------------------------------- sampling
    def set_sampling(self, slot: int, temperature: float = 0.0,
                     top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
                     seed: int = 0, repetition_penalty: float = 1.0,
                     presence_penalty: float = 0.0,
                     frequency_penalty: float = 0.0,
                     logit_bias: dict = None):
        """Write one slot's sampling parameters (sampling="request"
        engines).  The captured graph reads them on the device, so the
        change holds from the next step on without a recapture.  The
        last four need ``logit_processors=True``; a slot counts its
        generated tokens only while its parameters are not neutral."""
        self.set_sampling_slots([slot], [SamplingParams(
            temperature, top_k, top_p, min_p, seed, False,
            repetition_penalty, presence_penalty, frequency_penalty,
            logit_bias)])

    def set_sampling_slots(self, slots, params):
        """set_sampling for several slots at once: ``params`` holds one
        SamplingParams (None = the defaults) per slot; one host-to-
        device copy per parameter.  A temperature in (0, 1e-4) is
        raised to 1e-4, the floor of the ``temperature=-1`` path: below
        it the draw is the argmax anyway."""
        if self.sampling != "request":
            raise ValueError('set_sampling needs an engine built with '
                             'sampling="request"')
        slots = [int(slot) for slot in slots]
        params = [SamplingParams() if item is None else item
                  for item in params]
        if len(slots) != len(params):
            raise ValueError(f"{len(params)} parameter sets for "
                             f"{len(slots)} slots")
        for slot in slots:
            if not 0 <= slot < self.B:
                raise ValueError(f"slot {slot} outside [0, {self.B})")
        for item in params:
            item.validate()
            self._check_processors(item)
        if not slots:
            return
        index = torch.tensor(slots, dtype=torch.long).to(self.device)
        if self.logit_processors:
            NB = ops.LOGIT_BIAS_MAX
            biases = [item.bias_items() for item in params]
            self.buf_penalties[index] = torch.tensor(
                [[item.repetition_penalty, item.presence_penalty,
                  item.frequency_penalty] for item in params],
                dtype=torch.float32).to(self.device)
            self.buf_bias_ids[index] = torch.tensor(
                [[key for key, _ in bias] + [0] * (NB - len(bias))
                 for bias in biases], dtype=torch.int32).to(self.device)
            self.buf_bias_val[index] = torch.tensor(
                [[value for _, value in bias] + [0.0] * (NB - len(bias))
                 for bias in biases], dtype=torch.float32).to(self.device)
            self.buf_bias_n[index] = torch.tensor(
                [len(bias) for bias in biases],
                dtype=torch.int32).to(self.device)
        for buf, name in ((self.buf_temp_r, "temperature"),
                          (self.buf_top_k, "top_k"),
                          (self.buf_top_p, "top_p"),
                          (self.buf_min_p, "min_p"),
                          (self.buf_seed, "seed")):
            values = [getattr(item, name) for item in params]
            if name == "temperature":
                # like buf_temp: z / T stays finite for any real logit
                values = [max(value, 1e-4) if value > 0 else value
                          for value in values]
            values = torch.tensor(values, dtype=buf.dtype)
            buf[index] = values.to(self.device)

    def _check_processors(self, item: SamplingParams):
        """ValueError naming the logit-processor field that this engine
        cannot serve: any non-neutral one without the flag, a bias id
        outside the vocabulary with it."""
        if not self.logit_processors:
            for name, neutral in (("repetition_penalty", 1),
                                  ("presence_penalty", 0),
                                  ("frequency_penalty", 0)):
                if getattr(item, name) != neutral:
                    raise ValueError(
                        f"{name}={getattr(item, name)} needs an engine "
                        "built with logit_processors=True")
            if item.logit_bias:
                raise ValueError("logit_bias needs an engine built with "
                                 "logit_processors=True")
            return
        for key, _ in item.bias_items():
            if key >= self.cfg.vocab_size:
                raise ValueError(
                    f"logit_bias names token {key}, outside the "
                    f"vocabulary [0, {self.cfg.vocab_size})")

    def _prepare_tok_state(self, slots, tok_slot, tokens, fresh=None):
        """Before a first token is sampled: zero the state rows of the
        freshly prefilled ``slots`` (a long tensor; ``fresh`` masks
        those that start a sequence, None = all) and set the in-prompt
        bit of ``tokens`` [T] in rows ``tok_slot`` [T].  A prefix
        continuation is not fresh: it ORs its tokens into the row."""
        state = self.buf_tok_state
        tok_slot, tokens = tok_slot.long(), tokens.long()
        state[slots if fresh is None else slots[fresh]] = 0
        # duplicates write one value: every pair reads the same word
        state[tok_slot, tokens] = state[tok_slot, tokens] | 1

    def _packed_prefill_serves(self) -> bool:
        """Whether prefill_packed (ops.attn_prefill) handles this
        engine: bf16 KV, head_dim 128, group size <= 8."""
        w = self.weights
        return self.kv_dtype == "bf16" and self.cfg.head_dim == 128 \
            and w.hq % w.hkv == 0 and w.hq // w.hkv <= 8

    def _sample_slots(self, logits, slots, prompt):
        """First token of freshly prefilled ``slots`` (a long tensor or
        a slice of rows) from their last-token logits [n, vocab], by
        each slot's own parameters; pos = the prompt length.  ``prompt``
        is (tok_slot [T], tokens [T], fresh [n] bool or None): the
        prompts' tokens with the slot of each, for the token-state rows
        of a logit_processors engine, whose penalties and bias are
        applied to the logits, in place, before the draw."""
        logits = logits.contiguous()
        n = logits.shape[0]
        if self.logit_processors:
            if isinstance(slots, slice):
                slots = torch.arange(self.B, device=self.device)[slots]
            self._prepare_tok_state(slots, *prompt)
            ops.logit_processors(
                logits, self.buf_tok_state,
                self.buf_penalties[slots].contiguous(),
                self.buf_bias_ids[slots].contiguous(),
                self.buf_bias_val[slots].contiguous(),
                self.buf_bias_n[slots].contiguous(),
                tokens=None, rows=slots.to(torch.int32))
        tokens = torch.empty(n, dtype=torch.int64, device=self.device)
        logprob = torch.empty(n, dtype=torch.float32, device=self.device)
        kept = torch.empty(n, dtype=torch.int32, device=self.device)
        ops.sample_tokens(
            logits, self.cache_lens[slots].contiguous(),
            self.buf_temp_r[slots].contiguous(),
            self.buf_top_k[slots].contiguous(),
            self.buf_top_p[slots].contiguous(),
            self.buf_min_p[slots].contiguous(),
            self.buf_seed[slots].contiguous(), tokens, logprob, kept)
        self.buf_tokens[slots] = tokens
        self.buf_logprob[slots] = logprob
        self.buf_kept[slots] = kept
        return tokens

    # ------------------------------------------------------------ gemm
    def _plan(self, w_):
        key = (w_.shape[0], w_.shape[1])
        if key not in self._ksplits:
            self._ksplits[key] = ops.pick_gemm_plan(self.B, *key)
        return self._ksplits[key]

    def _gemm(self, a, w_, out, a8=None, a_scale=None):
        """skinny GEMM into a preallocated bf16 out + f32 scratch.
        Uses the fp8-weight pack when this engine runs in fp8w mode;
        a8/a_scale skip the quant launch (rmsnorm sidecar)."""
        pack = self._fp8_packs.get(id(w_))
        if pack is not None:
            M, K = a.shape
            if a8 is None:
                a8 = self.buf_a8.narrow(0, 0, M * K).view(M, K)
                ops.quant_fp8_rows(a, a8, self.buf_a_scale)
                a_scale = self.buf_a_scale
            ksplit, _ = self._plan(w_)
            return ops.skinny_gemm_fp8(a8, a_scale, pack[0],
                                       pack[1], out=out,
                                       c_f32=self.buf_c32, ksplit=ksplit)
        ksplit, variant = self._plan(w_)
        return ops.skinny_gemm(a, w_, out=out, c_f32=self.buf_c32,
                               ksplit=ksplit, variant=variant)

    def _gemm_slabs(self, a, w_):
        """split-K GEMM emitting f32 slabs (consumer folds them);
        returns the ksplit used.  GPU-only."""
        from mlrun_amd import _hip_ops

        ksplit, variant = self._plan(w_)
        if ksplit <= 1:
            return 0  # caller must use the bf16 path
        _hip_ops.skinny_gemm_slabs(self.buf_c32, a, w_, ksplit, variant)
        return ksplit

    def _maybe_allreduce(self, t):
        if self.tp_size > 1:
            from ..parallel.tp import all_reduce_tensor

            all_reduce_tensor(t, group=self.tp_group)
        return t

    # ------------------------------------------------------------ lora
    def load_adapter(self, slot: int, state: dict):
        """Load a LoRA adapter into table slot ``slot`` (shared by every
        replica built with ``lora=``).  ``state`` maps
        ``layers.{i}.{proj}.lora_A`` -> [r, K] and ``.lora_B`` -> [N, r]
        for any subset of layers and of the projections wqkv / wo / wgu /
        wdown, plus ``alpha``; r <= lora_rank, missing entries stay zero.
        A shape that does not fit the weights is a ValueError naming the
        key.  For an IDLE engine only: the tables are written in place
        under the captured graph, so no request may be decoding."""
        if self.lora is None:
            raise ValueError("engine built with max_adapters=0 holds no "
                             "adapter tables")
        self.lora.load(slot, state)
        # cached KV rows of this table slot are stale now
        self.clear_prefix_cache()

    def unload_adapter(self, slot: int):
        """Zero table slot ``slot`` (idle engine only, like
        load_adapter): rows that still name it then get a zero delta."""
        if self.lora is None:
            raise ValueError("engine built with max_adapters=0 holds no "
                             "adapter tables")
        self.lora.unload(slot)
        self.clear_prefix_cache()

    def _lora_decode(self, li, proj, x, y):
        """y[b] += Bm[id_b] (A[id_b] x[b]) for the decode rows, by
        buf_adapter: two launches, rows with id -1 exit at once."""
        a_tab, b_tab = self.lora.layers[li][proj]
        ops.lora_shrink(x, a_tab, self.buf_adapter, out=self.buf_lora_t)
        ops.lora_expand(y, self.buf_lora_t, b_tab, self.buf_adapter)

    def _adapter_ids(self, adapters, n):
        """Validate ``adapters`` (not None): one id per prompt for ``n``
        prompts, each in [-1, max_adapters).  Returns the ids, or None
        on an engine without adapter tables (where every id must be
        -1)."""
        ids = [int(a) for a in adapters]
        if self.lora is None:
            if any(a >= 0 for a in ids):
                raise ValueError("adapters= needs an engine built with "
                                 "max_adapters > 0")
            return None
        if len(ids) != n:
            raise ValueError(f"adapters has {len(ids)} ids for "
                             f"{n} prompts")
        for a in ids:
            if not -1 <= a < self.max_adapters:
                raise ValueError(f"adapter id {a} outside "
                                 f"[-1, {self.max_adapters})")
        return ids

    def _adapter_plan(self, adapters, slots, counts):
        """Prefill side of ``adapters=``: validate one id per prompt
        (-1 = base), record them in buf_adapter for ``slots`` and return
        the plan _lora_prefill consumes — a list of (id, row mask or
        None), one entry per DISTINCT adapter id of the call, with
        counts[i] token rows for prompt i.  None when no row is adapted.
        The host knows the ids, so nothing here syncs."""
        if adapters is None:
            if self.lora is not None:
                self.buf_adapter[slots] = -1
            return None
        ids = self._adapter_ids(adapters, len(counts))
        if ids is None:
            return None
        self.buf_adapter[slots] = torch.tensor(
            ids, dtype=torch.int32).to(self.device)
        distinct = sorted({a for a in ids if a >= 0})
        if not distinct:
            return None
        if len(set(ids)) == 1:
            return [(distinct[0], None)]  # every row, no mask needed
        row_ids = torch.tensor(
            [a for a, count in zip(ids, counts) for _ in range(count)],
            dtype=torch.int32).to(self.device)
        return [(a, (row_ids == a).unsqueeze(1)) for a in distinct]

    def _lora_prefill(self, plan, li, proj, x, y):
        """Add the adapters' deltas to a prefill projection output
        y = x @ W^T ([T, N] bf16): f32 math, one rounding, one pass per
        distinct id.  Each pass runs over ALL T rows and is masked to
        its own rows, so a row's result cannot depend on which other
        adapters share the call (a library GEMM may round a row
        differently when its row count changes)."""
        if plan is None:
            return y
        a_tab, b_tab = self.lora.layers[li][proj]
        xf = x.float()
        for a, mask in plan:
            delta = (xf @ a_tab[a].float().t()) @ b_tab[a].float().t()
            new = (y.float() + delta).to(y.dtype)
            y = new if mask is None else torch.where(mask, new, y)
        return y

    # ---------------------------------------------------------- decode
    def _decode_step_body(self):
        """One token step for all B sequences.  Reads buf_tokens,
        leaves next tokens in buf_tokens (greedy).  Entirely on-device:
        capturable as one hipGraph."""
        cfg, w = self.cfg, self.weights
        d = cfg.head_dim
        B = self.B
        # embedding (full embed table on every rank)
        torch.index_select(w.embed, 0, self.buf_tokens,
                           out=self.buf_residual)
        fp8 = self.weight_dtype == "fp8w" and self.on_gpu and \
            self.tp_size == 1
        h8 = self.buf_h8 if fp8 else None
        h8s = self.buf_h8_scale if fp8 else None
        ops.rmsnorm(self.buf_residual, w.layers[0]["attn_norm"],
                    eps=cfg.rms_eps, out=self.buf_hidden,
                    out8=h8, out_scale=h8s)
        # incoming token sits at position cache_lens; bump the length
        # once up front so attention covers it in every layer.  Clamp
        # to the cache end: under continuous batching idle/finished
        # slots keep stepping until reused — they must park on the
        # last row instead of running off the cache (graph-safe ops)
        torch.clamp(self.cache_lens, max=self.cfg.max_seq_len - 1,
                    out=self.buf_positions)
        self.cache_lens.add_(1).clamp_(max=self.cfg.max_seq_len)
        positions = self.buf_positions
        # slab fusion (GPU, TP=1): split-K consumers fold the f32 slabs
        # directly.  MEASURED: fusing into the 16-row norm kernels is a
        # net loss (consumer grid = B rows is parallelism-starved vs the
        # 2048-block reduce_cast), so only the rope/KV consumer (grid
        # B x heads) fuses by default; override with MLRUN_SLAB_MODE.
        mode = os.environ.get("MLRUN_SLAB_MODE", "rope")
        on = self.on_gpu and self.tp_size == 1 and mode != "none"
        use_slabs = on and self.weight_dtype == "bf16" and \
            self.kv_dtype == "bf16"  # qkv slab (bf16 caches only)
        use_norm_slabs = on and mode == "all" 
        lora = self.lora is not None
        if lora:
            # the adapter delta has to land on the bf16 GEMM output
            # before rope / norm: the slab-fused consumers are bypassed
            use_slabs = use_norm_slabs = False
        if use_slabs or use_norm_slabs:
            from mlrun_amd import _hip_ops
        for li, layer in enumerate(w.layers):
            # qkv projection -> rope -> caches
            done = 0
            if use_slabs:
                done = self._gemm_slabs(self.buf_hidden, layer["wqkv"])
                if done:
                    _hip_ops.rope_kv_slab(
                        self.buf_qkv, self.k_cache[li], self.v_cache[li],
                        self.buf_c32, positions, self.cos_sin, w.hq, done)
            if not done:
                self._gemm(self.buf_hidden, layer["wqkv"], self.buf_qkv,
                           a8=h8, a_scale=h8s)
                if lora:
                    self._lora_decode(li, "wqkv", self.buf_hidden,
                                      self.buf_qkv)
                ops.rope_kv_fused(self.buf_qkv, self.k_cache[li],
                                  self.v_cache[li], positions,
                                  self.cos_sin, w.hq,
                                  k_scale=self._kscale(li),
                                  v_scale=self._vscale(li))
            q = self.buf_qkv[:, :w.hq * d].view(B, w.hq, d)
            attn_view = self.buf_attn_out.view(B, w.hq, d)
            ops.attn_decode(q, self.k_cache[li], self.v_cache[li],
                            self.cache_lens, self.scale, out=attn_view,
                            partial_ws=self.buf_attn_ws,
                            nsplit=self.attn_nsplit,
                            k_scale=self._kscale(li),
                            v_scale=self._vscale(li))
            # attn-out projection -> residual+norm
            done = 0
            if use_norm_slabs:
                done = self._gemm_slabs(self.buf_attn_out, layer["wo"])
                if done:
                    _hip_ops.fused_add_rmsnorm_slab(
                        self.buf_hidden, self.buf_residual, self.buf_c32,
                        layer["ffn_norm"], done, cfg.rms_eps)
            if not done:
                self._gemm(self.buf_attn_out, layer["wo"], self.buf_proj)
                if lora:
                    self._lora_decode(li, "wo", self.buf_attn_out,
                                      self.buf_proj)
                self._maybe_allreduce(self.buf_proj)
                ops.fused_add_rmsnorm(self.buf_proj, layer["ffn_norm"],
                                      residual=self.buf_residual,
                                      eps=cfg.rms_eps, out=self.buf_hidden,
                                      out8=h8, out_scale=h8s)
            # mlp (fused gate|up projection)
            done = 0
            if use_norm_slabs:
                done = self._gemm_slabs(self.buf_hidden, layer["wgu"])
                if done:
                    _hip_ops.swiglu_slab(self.buf_act, self.buf_c32, done)
            if not done:
                self._gemm(self.buf_hidden, layer["wgu"], self.buf_gu,
                           a8=h8, a_scale=h8s)
                if lora:
                    self._lora_decode(li, "wgu", self.buf_hidden,
                                      self.buf_gu)
                ops.swiglu_fused(self.buf_gu, out=self.buf_act)
            next_norm = w.layers[li + 1]["attn_norm"] \
                if li + 1 < cfg.num_layers else w.final_norm
            done = 0
            if use_norm_slabs:
                done = self._gemm_slabs(self.buf_act, layer["wdown"])
                if done:
                    _hip_ops.fused_add_rmsnorm_slab(
                        self.buf_hidden, self.buf_residual, self.buf_c32,
                        next_norm, done, cfg.rms_eps)
            if not done:
                self._gemm(self.buf_act, layer["wdown"], self.buf_down)
                if lora:
                    self._lora_decode(li, "wdown", self.buf_act,
                                      self.buf_down)
                self._maybe_allreduce(self.buf_down)
                ops.fused_add_rmsnorm(self.buf_down, next_norm,
                                      residual=self.buf_residual,
                                      eps=cfg.rms_eps, out=self.buf_hidden,
                                      out8=h8, out_scale=h8s)
        self._gemm(self.buf_hidden, w.lm_head, self.buf_logits,
                   a8=h8, a_scale=h8s)
        if self.sampling == "request":
            if self.logit_processors:
                # buf_tokens still holds the token this step consumed:
                # the newest generated one, the only one not yet counted
                ops.logit_processors(
                    self.buf_logits, self.buf_tok_state, self.buf_penalties,
                    self.buf_bias_ids, self.buf_bias_val, self.buf_bias_n,
                    tokens=self.buf_tokens)
            # pos = the bumped length: the position of the new token
            ops.sample_tokens(self.buf_logits, self.cache_lens,
                              self.buf_temp_r, self.buf_top_k,
                              self.buf_top_p, self.buf_min_p, self.buf_seed,
                              self.buf_tokens, self.buf_logprob,
                              self.buf_kept)
        else:
            self._select_tokens(self.buf_logits, out=self.buf_tokens)

    def _select_tokens(self, logits: torch.Tensor,
                       out: torch.Tensor = None) -> torch.Tensor:
        """Greedy argmax, or temperature/top-k sampling via the
        Gumbel-max trick: argmax(logits/T + G), G = -log(-log(U)).
        One argmax either way — capture-safe and branch-free on
        device."""
        if self.per_slot_temp and logits.shape[0] == self.B:
            scores = logits.float() / self.buf_temp
            u = torch.rand_like(scores).clamp_(1e-9, 1.0 - 1e-9)
            gumbel = -torch.log(-torch.log(u))
            if out is None:
                return (scores + gumbel).argmax(dim=-1)
            torch.argmax(scores + gumbel, dim=-1, out=out)
            return out
        if self.temperature <= 0.0:
            if out is None:
                return logits.argmax(dim=-1)
            torch.argmax(logits, dim=-1, out=out)
            return out
        scores = logits.float() / self.temperature
        if self.top_k > 0 and self.top_k < scores.shape[-1]:
            kth = torch.topk(scores, self.top_k, dim=-1
                             ).values[..., -1:]
            scores = torch.where(scores < kth,
                                 torch.full_like(scores, float("-inf")),
                                 scores)
        u = torch.rand_like(scores).clamp_(1e-9, 1.0 - 1e-9)
        gumbel = -torch.log(-torch.log(u))
        if out is None:
            return (scores + gumbel).argmax(dim=-1)
        torch.argmax(scores + gumbel, dim=-1, out=out)
        return out

    _capture_lock = None

    def capture_graph(self):
        """Capture the decode step as one hipGraph (3 warmup runs on a
        side stream per torch graph discipline).  Captures are
        serialized process-wide: concurrent stream captures on one
        device corrupt each other."""
        if not self.use_graph or self._graph is not None:
            return
        import threading

        cls = type(self)
        if cls._capture_lock is None:
            cls._capture_lock = threading.Lock()
        with cls._capture_lock:
            self._capture_graph_locked()

    def _capture_graph_locked(self):
        if self._graph is not None:
            return
        import torch.distributed as dist

        lens_backup = self.cache_lens.clone()
        tokens_backup = self.buf_tokens.clone()
        # the warm-up steps sample too: keep the pending tokens' logprobs
        sample_backup = [(buf, buf.clone()) for buf in (
            self.buf_logprob, self.buf_kept)] \
            if self.sampling == "request" else []
        if self.logit_processors:
            # ... and count their tokens: the table must come back exactly
            sample_backup.append((self.buf_tok_state,
                                  self.buf_tok_state.clone()))
        if self.tp_size > 1 and dist.is_available() and \
                dist.is_initialized():
            # warmup runs REAL collectives — align ranks first so the
            # three eager steps pair up even if ranks arrive staggered
            dist.barrier(group=self.tp_group)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self._decode_step_body()
        torch.cuda.current_stream().wait_stream(side)
        self.cache_lens.copy_(lens_backup)
        self.buf_tokens.copy_(tokens_backup)
        for buf, backup in sample_backup:
            buf.copy_(backup)
        graph = torch.cuda.CUDAGraph()
        # RCCL collectives ARE capturable (the all-reduce kernel is
        # recorded into the graph and pairs up across ranks at replay),
        # but the NCCL watchdog thread polls events during capture —
        # "global" capture mode would see those as stray captures, so
        # distributed captures use thread_local error mode (the decode
        # body launches everything from this thread).
        err_mode = "thread_local" if dist.is_available() and \
            dist.is_initialized() else "global"
        with torch.cuda.graph(graph, capture_error_mode=err_mode):
            self._decode_step_body()
        # stream capture records without executing, but restore anyway
        # in case a backend executed eagerly during capture
        self.cache_lens.copy_(lens_backup)
        self.buf_tokens.copy_(tokens_backup)
        for buf, backup in sample_backup:
            buf.copy_(backup)
        self._graph = graph
        logger.info("decode hipGraph captured", batch=self.B,
                    layers=self.cfg.num_layers)

    def decode_step(self):
        if self._graph is not None:
            self._graph.replay()
        else:
            self._decode_step_body()

    # --------------------------------------------------------- prefill
    def rebuild_fp8_packs(self):
        """(Re)quantize the fp8 weight packs from the CURRENT weights.
        Must be called again after load_state_dict — otherwise serving
        would run on packs quantized from the discarded init weights."""
        if self.weight_dtype != "fp8w" or not (self.on_gpu and
                                               self.tp_size == 1):
            return
        w = self.weights
        self._fp8_packs = {}
        for layer in w.layers:
            for key in ("wqkv", "wo", "wgu", "wdown"):
                self._fp8_packs[id(layer[key])] = \
                    ops.quantize_fp8_weight(layer[key])
        self._fp8_packs[id(w.lm_head)] = \
            ops.quantize_fp8_weight(w.lm_head)

    def _kscale(self, li):
        return None if self.k_scale is None else self.k_scale[li]

    def _vscale(self, li):
        return None if self.v_scale is None else self.v_scale[li]

    def _check_token_ids(self, tokens: torch.Tensor):
        """ValueError for a prompt id outside the vocabulary, checked
        on the host: on the device the embedding gather would read
        outside the table, and a fault there ends the whole process.
        Tokens already on the device are not checked (no sync)."""
        if tokens.device.type != "cpu" or tokens.numel() == 0:
            return
        low, high = int(tokens.min()), int(tokens.max())
        if low < 0 or high >= self.cfg.vocab_size:
            raise ValueError(
                f"token id outside [0, {self.cfg.vocab_size}) in prompt")

    def _run_layers(self, residual, project, attend):
        """The layer loop of every non-graph pass (the three prefills
        and verify_step) over the token rows ``residual`` [T, H], which
        it updates in place; returns the final normed hidden [T, H].
        ``project(li, name, x)`` is the GEMM of x with layer li's weight
        ``name`` plus whatever delta the path adds; ``attend(li, qkv)``
        writes the layer's KV rows and returns the attention output
        [T, Hq*d]."""
        cfg, w = self.cfg, self.weights
        hidden = ops.rmsnorm(residual, w.layers[0]["attn_norm"],
                             eps=cfg.rms_eps)
        for li, layer in enumerate(w.layers):
            attn = attend(li, project(li, "wqkv", hidden))
            proj = project(li, "wo", attn)
            self._maybe_allreduce(proj)
            hidden = ops.fused_add_rmsnorm(proj, layer["ffn_norm"],
                                           residual=residual,
                                           eps=cfg.rms_eps)
            gu = project(li, "wgu", hidden)
            act = ops.swiglu_fused(gu.contiguous())
            down = project(li, "wdown", act)
            self._maybe_allreduce(down)
            next_norm = w.layers[li + 1]["attn_norm"] \
                if li + 1 < cfg.num_layers else w.final_norm
            hidden = ops.fused_add_rmsnorm(down, next_norm,
                                           residual=residual,
                                           eps=cfg.rms_eps)
        return hidden

    def _prefill_project(self, plan):
        """_run_layers' ``project`` of the prefills: the library GEMM
        plus the LoRA deltas of ``plan``."""
        layers = self.weights.layers

        def project(li, name, x):
            return self._lora_prefill(plan, li, name, x,
                                      x @ layers[li][name].t())
        return project

    def _dense_attend(self, rows, B, S):
        """_run_layers' ``attend`` of the dense prefills: B prompts of S
        tokens each, rope, K/V into cache rows ``rows`` (an index for
        the cache's batch dimension), causal SDPA."""
        w, d = self.weights, self.cfg.head_dim
        positions = torch.arange(S, dtype=torch.int32, device=self.device
                                 ).repeat(B)

        def attend(li, qkv):
            q = qkv[:, :w.hq * d].reshape(B * S, w.hq, d).contiguous()
            k = qkv[:, w.hq * d:(w.hq + w.hkv) * d].reshape(
                B * S, w.hkv, d).contiguous()
            v = qkv[:, (w.hq + w.hkv) * d:].reshape(B * S, w.hkv, d)
            ops.rope_inplace(q, positions, self.cos_sin)
            ops.rope_inplace(k, positions, self.cos_sin)
            kc = k.view(B, S, w.hkv, d).transpose(1, 2).contiguous()
            vc = v.view(B, S, w.hkv, d).transpose(1, 2).contiguous()
            if self.kv_dtype == "fp8":
                k8, ks = ops.quantize_kv_rows(kc)
                v8, vs = ops.quantize_kv_rows(vc)
                self.k_cache[li, rows, :, :S] = k8
                self.v_cache[li, rows, :, :S] = v8
                self.k_scale[li, rows, :, :S] = ks
                self.v_scale[li, rows, :, :S] = vs
            else:
                self.k_cache[li, rows, :, :S] = kc
                self.v_cache[li, rows, :, :S] = vc
            qh = q.view(B, S, w.hq, d).transpose(1, 2)
            attn = torch.nn.functional.scaled_dot_product_attention(
                qh, kc, vc, is_causal=True, enable_gqa=True)
            return attn.transpose(1, 2).reshape(B * S, w.hq * d)
        return attend

    def _first_tokens(self, logits, slots, prompt):
        """First token of the freshly prefilled ``slots`` (a long
        tensor) into buf_tokens, from their last-token logits;
        ``prompt`` as in _sample_slots."""
        if self.sampling == "request":
            self._sample_slots(logits, slots, prompt)
        elif self.per_slot_temp:
            scores = logits.float() / self.buf_temp[slots]
            u = torch.rand_like(scores).clamp_(1e-9, 1.0 - 1e-9)
            self.buf_tokens[slots] = (
                scores - torch.log(-torch.log(u))).argmax(dim=-1)
        else:
            self.buf_tokens[slots] = self._select_tokens(logits)

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, adapters=None
                ) -> torch.Tensor:
        """Process prompts [B, S]; fill KV caches; return last-token
        logits [B, vocab].  hipBLASLt GEMMs + SDPA.  ``adapters``: one
        LoRA table slot per prompt (-1 = base model, the default); the
        ids stay in buf_adapter for the decode steps that follow."""
        w = self.weights
        B, S = tokens.shape
        self._check_token_ids(tokens)
        plan = self._adapter_plan(adapters, slice(0, B), [S] * B)
        tokens = tokens.to(self.device)
        x = w.embed[tokens.reshape(-1)]  # [B*S, H]
        # K/V fill the cache's whole batch dimension
        hidden = self._run_layers(x.contiguous(),
                                  self._prefill_project(plan),
                                  self._dense_attend(slice(None), B, S))
        self.cache_lens.fill_(S)
        last = hidden.view(B, S, -1)[:, -1]
        logits = last @ w.lm_head.t()
        if self.sampling == "request":
            rows = torch.arange(B, device=self.device)
            self._sample_slots(logits, slice(0, B), (
                rows.repeat_interleave(S), tokens.reshape(-1), None))
        return logits

    @torch.no_grad()
    def prefill_slots(self, tokens: torch.Tensor,
                      slots: torch.Tensor, adapters=None) -> torch.Tensor:
        """Continuous-batching admission: prefill B' <= B prompts and
        scatter their KV/state into cache rows ``slots``, leaving the
        other slots' caches and lengths untouched.  Returns last-token
        logits [B'].  ``adapters``: one LoRA table slot per prompt
        (-1 = base).  Decode then advances ALL slots each step.

        Two code paths.  A sampling="engine" engine, and any engine
        whose shape the packed attention kernel does not serve, runs
        the same prefill math as ``prefill`` on a temporary B'-sized
        view.  A sampling="request" engine that the packed kernel
        serves (bf16 KV, head_dim 128, at most 8 q-heads per KV head)
        does NOT: it hands the prompts to ``prefill_packed``.  A seeded
        request must return the same tokens AND logprobs under either
        prefill mode of the server, which needs one attention code path
        for both, not two that agree within a bound.  On that path the
        argument checks are ``prefill_packed``'s, so a slot count that
        does not match or a prompt that is too long raises ValueError
        where the other path asserts, and ``tokens.tolist()`` syncs
        with the host if ``tokens`` is on the device."""
        cfg, w = self.cfg, self.weights
        Bp, S = tokens.shape
        if self.sampling == "request" and self._packed_prefill_serves():
            assert Bp <= self.B and S < cfg.max_seq_len
            return self.prefill_packed(
                tokens.tolist(), torch.as_tensor(slots).tolist(),
                adapters=adapters)
        slots = torch.as_tensor(slots, dtype=torch.long,
                                device=self.device)
        assert Bp == slots.numel() and Bp <= self.B
        assert S < cfg.max_seq_len
        self._check_token_ids(tokens)
        plan = self._adapter_plan(adapters, slots, [S] * Bp)
        tokens = tokens.to(self.device)
        x = w.embed[tokens.reshape(-1)]
        hidden = self._run_layers(x.contiguous(),
                                  self._prefill_project(plan),
                                  self._dense_attend(slots, Bp, S))
        self.cache_lens[slots] = S
        last = hidden.view(Bp, S, -1)[:, -1]
        logits = last @ w.lm_head.t()
        self._first_tokens(logits, slots, (
            slots.repeat_interleave(S), tokens.reshape(-1), None))
        return logits

    @torch.no_grad()
    def prefill_packed(self, prompts, slots, starts=None, adapters=None
                       ) -> torch.Tensor:
        """Varlen admission: prefill n prompts of ANY lengths in one
        pass over their concatenated (packed) token stream.  Attention
        is causal within each sequence only (``ops.attn_prefill``) and
        K/V are written straight into cache rows ``slots``
        (``ops.rope_kv_varlen``), so there is no padding and a
        request's result does not depend on what it is packed with.

        ``starts[i]`` (default 0) is the number of tokens already cached
        in slot i: the chunk is written at positions starts[i].. and
        attends to that prefix as well (prefix continuation).  Returns
        last-token logits [n, vocab]; sets cache_lens and buf_tokens
        for the slots like ``prefill_slots``.  bf16 KV caches only.
        ``adapters``: one LoRA table slot per prompt (-1 = base)."""
        return self._packed_pass(
            *self._check_packed(prompts, slots, starts), adapters)

    def _check_packed(self, prompts, slots, starts=None):
        """The argument checks of a packed pass, all on the host and
        before any device work.  Returns (prompts, slots, starts) as
        lists of ints."""
        cfg = self.cfg
        if self.kv_dtype == "fp8":
            raise ValueError("packed prefill needs a bf16 KV cache")
        prompts = [[int(t) for t in p] for p in prompts]
        slot_list = [int(s) for s in slots]
        n = len(prompts)
        start_list = [0] * n if starts is None else \
            [int(s) for s in starts]
        if n == 0 or len(slot_list) != n or len(start_list) != n:
            raise ValueError("prompts, slots and starts must be "
                             "non-empty and of equal length")
        if len(set(slot_list)) != n:
            raise ValueError(f"duplicate slots in {slot_list}")
        lens = [len(p) for p in prompts]
        for prompt in prompts:
            # checked on the host: an out-of-range id would make the
            # embedding gather read outside the table on the device
            if prompt and not 0 <= min(prompt) <= max(prompt) < \
                    cfg.vocab_size:
                raise ValueError(
                    f"token id outside [0, {cfg.vocab_size}) in prompt")
        for length, slot, start in zip(lens, slot_list, start_list):
            if length < 1:
                raise ValueError("every prompt needs at least one token")
            if not 0 <= slot < self.B:
                raise ValueError(f"slot {slot} outside [0, {self.B})")
            if start < 0:
                raise ValueError(f"negative start {start}")
            if start + length >= cfg.max_seq_len:
                raise ValueError(
                    f"sequence of {start}+{length} tokens would reach "
                    f"max_seq_len {cfg.max_seq_len}")
        return prompts, slot_list, start_list

    def _packed_pass(self, prompts, slot_list, start_list, adapters,
                     whole=None):
        """The packed pass over checked arguments (_check_packed).
        ``whole`` is None for a plain prefill_packed call, where a chunk
        with starts[i] > 0 continues a sequence and adds only its own
        tokens to the slot's token state.  prefill_cached passes the
        full prompts there: its chunks are the uncached ends of FRESH
        requests, whose every token, the cached ones too, counts as
        in the prompt."""
        cfg, w = self.cfg, self.weights
        n = len(prompts)
        lens = [len(p) for p in prompts]
        d = cfg.head_dim
        T = sum(lens)
        # one host->device copy for all the int32 index vectors
        cu_list = [0]
        pos_list, tok_slot_list = [], []
        for length, slot, start in zip(lens, slot_list, start_list):
            cu_list.append(cu_list[-1] + length)
            pos_list.extend(range(start, start + length))
            tok_slot_list.extend([slot] * length)
        meta = torch.tensor(
            pos_list + tok_slot_list + cu_list + slot_list + start_list,
            dtype=torch.int32).to(self.device)
        positions, tok_slot, cu_seqlens, slots_i32, kv_start = \
            meta.split([T, T, n + 1, n, n])
        tokens = torch.tensor([t for p in prompts for t in p],
                              dtype=torch.int64).to(self.device)
        max_q_len = max(lens)
        plan = self._adapter_plan(adapters, slots_i32.long(), lens)
        x = w.embed[tokens]  # [T, H]

        def attend(li, qkv):
            ops.rope_kv_varlen(qkv, self.k_cache[li], self.v_cache[li],
                               positions, tok_slot, self.cos_sin, w.hq)
            q = qkv[:, :w.hq * d].view(T, w.hq, d)  # strided view
            return ops.attn_prefill(q, self.k_cache[li], self.v_cache[li],
                                    cu_seqlens, slots_i32, kv_start,
                                    self.scale, max_q_len=max_q_len)

        hidden = self._run_layers(x.contiguous(),
                                  self._prefill_project(plan), attend)
        slots_long = slots_i32.long()
        self.cache_lens[slots_long] = kv_start + (
            cu_seqlens[1:] - cu_seqlens[:-1])
        last = hidden[cu_seqlens[1:].long() - 1]
        logits = last @ w.lm_head.t()
        if whole is not None and self.logit_processors:
            state = torch.tensor(
                [slot for slot, p in zip(slot_list, whole) for _ in p]
                + [t for p in whole for t in p],
                dtype=torch.int64).to(self.device)
            prompt = (*state.split(state.numel() // 2), None)
        else:
            prompt = (tok_slot.long(), tokens, kv_start == 0)
        self._first_tokens(logits, slots_long, prompt)
        return logits

    @torch.no_grad()
    def prefill_cached(self, prompts, slots, adapters=None) -> torch.Tensor:
        """prefill_packed through the prefix cache (engines built with
        ``prefix_cache_blocks > 0``): the same arguments, the same
        result and slot state, but the leading 32-token blocks of a
        prompt whose KV rows are in the pool are copied into the slot
        and only the rest is prefilled.

        One ``ops.kv_block_copy`` gathers every hit block of the call,
        one packed pass runs over the uncached ends with ``starts`` =
        the hit lengths, and one more ``kv_block_copy`` stores the
        prompts' new full blocks from the slots into the pool, all on
        the current stream.  A hit is on content: every token up to the
        block's end and the adapter id are equal.  At least one token
        of a prompt is always prefilled.  A call that fails its checks
        changes nothing, in the slots or in the cache."""
        index = self.prefix_index
        if index is None:
            raise ValueError("prefill_cached needs an engine built with "
                             "prefix_cache_blocks > 0")
        prompts, slot_list, _ = self._check_packed(prompts, slots)
        ids = None if adapters is None else \
            self._adapter_ids(adapters, len(prompts))
        keys = ids if ids is not None else [-1] * len(prompts)
        BT = ops.KV_BLOCK_TOKENS
        index.begin()
        hits = [index.lookup(p, key) for p, key in zip(prompts, keys)]
        self._copy_blocks(
            [(block, 0, slot, j) for slot, chain in zip(slot_list, hits)
             for j, block in enumerate(chain)], to_pool=False)
        starts = [len(chain) * BT for chain in hits]
        logits = self._packed_pass(
            [p[start:] for p, start in zip(prompts, starts)],
            slot_list, starts, adapters, whole=prompts)
        self._copy_blocks(
            [(slot, j, block, 0)
             for p, key, slot in zip(prompts, keys, slot_list)
             for j, block in index.insert(p, key)], to_pool=True)
        return logits

    def _copy_blocks(self, entries, to_pool):
        """One ops.kv_block_copy over ``entries`` =
        [(src row, src block, dst row, dst block)], pool -> cache or
        cache -> pool; nothing is launched for an empty list."""
        if not entries:
            return
        rows = torch.tensor(entries, dtype=torch.int32).t().contiguous(
            ).to(self.device)
        pool, cache = (self.pc_k, self.pc_v), (self.k_cache, self.v_cache)
        src, dst = (cache, pool) if to_pool else (pool, cache)
        ops.kv_block_copy(*src, *dst, rows[0], rows[1], rows[2], rows[3])

    # -------------------------------------------------------- generate
    @torch.no_grad()
    def generate(self, tokens: torch.Tensor, max_new_tokens: int = 32,
                 adapters=None) -> torch.Tensor:
        """Greedy generation.  tokens [B, S] -> [B, max_new_tokens].
        ``adapters``: one LoRA table slot per row (-1 = base)."""
        B, S = tokens.shape
        assert B == self.B, f"engine built for batch {self.B}, got {B}"
        assert S + max_new_tokens <= self.cfg.max_seq_len
        logits = self.prefill(tokens, adapters=adapters)
        if self.sampling == "request":
            next_tokens = self.buf_tokens.clone()  # sampled by prefill
        else:
            next_tokens = self._select_tokens(logits)
            self.buf_tokens.copy_(next_tokens)
        generated = [next_tokens.clone()]
        if self.use_graph and self._graph is None:
            self.capture_graph()
        for _ in range(max_new_tokens - 1):
            self.decode_step()
            generated.append(self.buf_tokens.clone())
        return torch.stack(generated, dim=1)

    # ----------------------------------------------------- speculative
    def _check_speculative(self, k: int):
        """Host-side preconditions of the verify path (no device work)."""
        if self.lora is not None:
            raise ValueError(
                f"speculative decoding conflicts with max_adapters="
                f"{self.max_adapters}: the verify pass runs the base "
                "weights only")
        if self.sampling == "request":
            raise ValueError(
                'speculative decoding conflicts with sampling="request": '
                "it is greedy only")
        if self.temperature > 0.0 or self.per_slot_temp:
            raise ValueError(
                "speculative decoding is greedy only (temperature "
                f"{self.temperature} samples)")
        if self.kv_dtype != "bf16":
            raise ValueError("speculative decoding needs a bf16 KV cache "
                             f"(kv_dtype={self.kv_dtype!r})")
        if self.weight_dtype != "bf16":
            raise ValueError("speculative decoding needs bf16 weights "
                             f"(weight_dtype={self.weight_dtype!r})")
        if self.tp_size != 1:
            raise ValueError("speculative decoding needs tp_size == 1")
        if not 1 <= int(k) <= ops.VERIFY_MAX_QL - 1:
            raise ValueError(
                f"speculative k must be in [1, {ops.VERIFY_MAX_QL - 1}], "
                f"got {k}")

    def _verify_gemm(self, a, w_, QL):
        """a [B*QL, K] @ w_[N, K]^T for the verify pass: the library
        GEMM on the GPU (B * QL rows is past the skinny kernel's range).
        The CPU reference runs decode_step's fp32 reference GEMM once
        per query offset j on the B rows (b, j): a CPU GEMM's summation
        order depends on its row count, and only the same call on the
        same shape rounds every row like decode_step does, which is
        what lets the CPU tier compare the two paths token for token."""
        if self.on_gpu:
            return a @ w_.t()
        out = torch.empty(a.shape[0], w_.shape[0], dtype=a.dtype)
        for j in range(QL):
            out[j::QL] = ops.skinny_gemm(a[j::QL].contiguous(), w_)
        return out

    @torch.no_grad()
    def verify_step(self, drafts: torch.Tensor):
        """One speculative step: score the pending token plus k drafted
        tokens per sequence in ONE pass over the weights and accept the
        longest draft prefix that greedy decoding would have produced.

        drafts [B, k] (1 <= k <= 7) on the engine's device.  Row (b, j)
        of the pass carries buf_tokens[b] (j = 0) or drafts[b, j-1] at
        position cache_lens[b] + j.  Returns (pred [B, k+1],
        n_accepted [B]) as device tensors, without a host sync:
        pred[b, j] is the greedy token after row (b, j), n_accepted[b]
        the number of leading drafts equal to pred.  Then cache_lens[b]
        advances by n_accepted[b] + 1 and buf_tokens[b] becomes
        pred[b, n_accepted[b]], exactly the state n_accepted[b] + 1
        decode steps leave behind.  K/V rows of rejected drafts stay
        beyond cache_lens: never read, overwritten later.  All logits
        are kept in buf_verify_logits [B, k+1, vocab]."""
        cfg, w = self.cfg, self.weights
        if drafts.dim() != 2 or drafts.shape[0] != self.B:
            raise ValueError(f"drafts must be [{self.B}, k], got "
                             f"{tuple(drafts.shape)}")
        k = drafts.shape[1]
        self._check_speculative(k)
        B, QL, d = self.B, k + 1, cfg.head_dim
        T = B * QL
        drafts = drafts.to(device=self.device, dtype=torch.int64)
        # an out-of-range id would make the embedding gather read
        # outside the table; clamped it is merely a wrong guess (the
        # acceptance below compares the ORIGINAL ids, so it is rejected)
        fed = drafts.clamp(0, cfg.vocab_size - 1)
        tokens = torch.cat([self.buf_tokens.view(B, 1), fed], dim=1)
        # idle slots park at the cache end, like decode_step
        base = torch.clamp(self.cache_lens, min=0,
                           max=cfg.max_seq_len - QL)
        steps = torch.arange(QL, dtype=torch.int32, device=self.device)
        positions = (base.view(B, 1) + steps).reshape(T)
        tok_slot = torch.arange(B, dtype=torch.int32, device=self.device
                                ).repeat_interleave(QL)
        nsplit, ws = None, None
        if self.on_gpu:
            nsplit = ops.pick_verify_nsplit(B, w.hkv, cfg.max_seq_len)
            need = ops.attn_verify_ws_numel(B, QL, w.hq, nsplit)
            ws = getattr(self, "_verify_ws", None)
            if nsplit > 1 and (ws is None or ws.numel() < need):
                ws = self._verify_ws = torch.empty(
                    need, dtype=torch.float32, device=self.device)

        def project(li, name, x):
            return self._verify_gemm(x, w.layers[li][name], QL)

        def attend(li, qkv):
            ops.rope_kv_varlen(qkv, self.k_cache[li], self.v_cache[li],
                               positions, tok_slot, self.cos_sin, w.hq)
            q = qkv[:, :w.hq * d].view(B, QL, w.hq, d)  # strided view
            return ops.attn_verify(q, self.k_cache[li], self.v_cache[li],
                                   base, self.scale, nsplit=nsplit,
                                   partial_ws=ws)

        hidden = self._run_layers(w.embed[tokens.reshape(T)].contiguous(),
                                  project, attend)
        logits = getattr(self, "buf_verify_logits", None)
        if logits is None or logits.shape[1] != QL:
            logits = self.buf_verify_logits = torch.empty(
                B, QL, cfg.vocab_size, dtype=torch.bfloat16,
                device=self.device)
        logits.view(T, cfg.vocab_size).copy_(
            self._verify_gemm(hidden, w.lm_head, QL))
        pred = logits.argmax(dim=-1)  # [B, QL]
        hits = (drafts == pred[:, :k]).to(torch.int64)
        n_accepted = hits.cumprod(dim=1).sum(dim=1)  # leading matches
        self.cache_lens.add_((n_accepted + 1).to(torch.int32)
                             ).clamp_(max=cfg.max_seq_len)
        self.buf_tokens.copy_(
            pred.gather(1, n_accepted.view(B, 1)).view(B))
        return pred, n_accepted

    def _speculative_loop(self, history: torch.Tensor,
                          hist_lens: torch.Tensor, start_lens: torch.Tensor,
                          active: torch.Tensor, max_new_tokens: int,
                          k: int, ngram: int) -> torch.Tensor:
        """Draft-and-verify until every active row holds max_new_tokens
        generated tokens; returns them [B, max_new_tokens].

        history [B, max_seq_len] int64 holds each row's prompt and the
        tokens generated so far (hist_lens of them, the last one being
        the pending buf_tokens entry, so cache_lens == hist_lens - 1);
        start_lens are the prompt lengths.  A row that has its tokens —
        and every inactive row — is frozen: its cache_lens, buf_tokens
        and history are put back after each verify pass, so it cannot
        run past the cache while slower rows catch up.  The one host
        read per step is the smallest produced count."""
        B, QL = self.B, k + 1
        L = history.shape[1]
        steps = torch.arange(QL, dtype=torch.int64, device=self.device)
        counters = torch.zeros(2, dtype=torch.int64, device=self.device)
        big = torch.full((B,), max_new_tokens, dtype=torch.int32,
                         device=self.device)
        n_steps = 0
        produced_min = 1  # the prefill token
        while produced_min < max_new_tokens:
            produced = hist_lens - start_lens
            done = (produced >= max_new_tokens) | ~active
            drafts = ops.ngram_draft(history, hist_lens, k, n=ngram)
            lens_before = self.cache_lens.clone()
            tokens_before = self.buf_tokens.clone()
            pred, n_accepted = self.verify_step(drafts)
            self.cache_lens.copy_(
                torch.where(done, lens_before, self.cache_lens))
            self.buf_tokens.copy_(
                torch.where(done, tokens_before, self.buf_tokens))
            # all QL predictions go to history[b, len..len+QL); only
            # the first n_accepted + 1 of them become part of it
            idx = (hist_lens.view(B, 1).long() + steps).clamp_(max=L - 1)
            vals = torch.where(done.view(B, 1), history.gather(1, idx),
                               pred)
            history.scatter_(1, idx, vals)
            live = ~done
            hist_lens.add_((live * (n_accepted + 1)).to(torch.int32))
            counters[0] += live.sum() * k
            counters[1] += (n_accepted * live).sum()
            n_steps += 1
            produced_min = int(torch.where(
                active, hist_lens - start_lens, big).min())
        drafted, accepted = counters.tolist()
        self.spec_stats["steps"] += n_steps
        self.spec_stats["drafted"] += drafted
        self.spec_stats["accepted"] += accepted
        cols = start_lens.view(B, 1).long() + torch.arange(
            max_new_tokens, dtype=torch.int64, device=self.device)
        return history.gather(1, cols.clamp_(max=L - 1))

    @torch.no_grad()
    def generate_speculative(self, tokens: torch.Tensor,
                             max_new_tokens: int = 32, k: int = 3,
                             ngram: int = 2) -> torch.Tensor:
        """Greedy generation, several tokens per pass over the weights:
        an n-gram lookup in each row's own history drafts k tokens
        (``ops.ngram_draft``) and ``verify_step`` keeps the prefix that
        plain greedy decoding would have produced, so the output equals
        ``generate``'s.  tokens [B, S] -> [B, max_new_tokens].
        Acceptance counters accumulate in ``spec_stats``."""
        B, S = tokens.shape
        assert B == self.B, f"engine built for batch {self.B}, got {B}"
        self._check_speculative(k)
        assert S + max_new_tokens + k <= self.cfg.max_seq_len, \
            "speculative decoding needs room for k drafted tokens: " \
            f"{S}+{max_new_tokens}+{k} > {self.cfg.max_seq_len}"
        logits = self.prefill(tokens)
        self.buf_tokens.copy_(self._select_tokens(logits))
        history = torch.zeros(B, self.cfg.max_seq_len, dtype=torch.int64,
                              device=self.device)
        history[:, :S] = tokens.to(self.device)
        history[:, S] = self.buf_tokens
        hist_lens = torch.full((B,), S + 1, dtype=torch.int32,
                               device=self.device)
        start_lens = torch.full((B,), S, dtype=torch.int32,
                                device=self.device)
        active = torch.ones(B, dtype=torch.bool, device=self.device)
        return self._speculative_loop(history, hist_lens, start_lens,
                                      active, max_new_tokens, k, ngram)

    def reset(self):
        self.cache_lens.zero_()


class LlamaServer:
    """V2ModelServer-protocol step serving LlamaDecodeEngine inside a
    serving graph (the north-star config: gen-AI serving graph with a
    Llama V2ModelServer — BASELINE.json).

    Request: {"inputs": [[tok, ...], ...], "max_tokens": G}
    Response outputs: [[generated tokens], ...]

    Serving structure:
    - ``replicas`` engine replicas per GPU, each on its OWN HIP stream
      with private KV caches/buffers but SHARED weights — decode is
      latency-bound (PMC wait/busy ~7), so concurrent replica streams
      raise aggregate HBM utilization; requests must arrive
      concurrently (or via the batcher) to overlap
    - a task queue feeds the replica workers; events are chunked to
      the engine batch size
    - ``batch_window_ms``: small concurrent requests coalesce into one
      engine pass (dynamic batching)
    - ``prefill``: how continuous scheduling prefills an admitted
      group — "exact" (default) one pass per distinct prompt length,
      "packed" one varlen pass over all of them (bf16 KV only)
    - ``speculative``: k > 0 (at most 7) turns batch scheduling's
      decode loop into speculative greedy decoding — an n-gram lookup
      drafts k tokens per step and one verify pass keeps those that
      greedy decoding would have produced (greedy, bf16 weights and KV,
      ``scheduling="batch"`` only; default 0 = off)
    - ``adapters``: {name: model uri or state file} of LoRA adapters,
      loaded into table slots shared by all replicas; a request selects
      one with ``"adapter": name`` (absent / null = base model) and one
      engine pass — one captured graph — serves rows of different
      adapters.  ``max_adapters`` (default: their number) sizes the
      tables, ``lora_rank`` (8/16/32/64) is the table rank.  Not with
      ``speculative > 0``.  Adapters are fixed once ``load()`` ran.
    - ``sampling``: "engine" (default) picks tokens with the engine-wide
      ``temperature`` / ``top_k``; "request" gives every request its own
      ``temperature``, ``top_k``, ``top_p``, ``min_p``, ``seed`` and
      ``logprobs`` fields on the fused ``ops.sample_tokens`` kernel, in
      both schedulers and through the batcher.  The constructor's
      ``temperature``, ``top_k``, ``top_p`` and ``min_p`` are then the
      defaults of requests that omit them.  Prompt j of a request draws
      with ``seed + j``; a request without a seed gets a random one.
      A request's tokens depend on its prompt, seed and parameters
      only.  Not with ``speculative > 0``.
    - ``logit_processors``: True (needs ``sampling="request"``) also
      reads a request's ``repetition_penalty`` ([0.1, 10]),
      ``presence_penalty`` / ``frequency_penalty`` ([-2, 2]) and
      ``logit_bias`` ({token id: value in [-100, 100]}, at most 64) and
      applies them, in that order, with ``ops.logit_processors`` before
      every draw; logprobs are then those of the processed logits.
      Without the flag the four fields are not read.
    - ``prefix_cache_blocks``: N > 0 gives every replica a pool of N
      32-token KV blocks; admission then goes through
      ``engine.prefill_cached``, which copies the cached leading blocks
      of a prompt into its slot and prefills the rest, in both
      schedulers and whatever ``prefill`` says.  Each replica has its
      own pool: a prefix cached on one misses on another.  Not with
      ``kv_dtype="fp8"`` or ``speculative > 0``.  Default 0 = off.
    """

    def __init__(self, context=None, name=None, model_path=None,
                 config=None, batch_size=16, max_new_tokens=32,
                 device=None, use_graph=True, batch_window_ms=0,
                 replicas=1, weight_dtype="bf16", kv_dtype="bf16",
                 scheduling="batch", stop_token: int = None,
                 temperature: float = 0.0, top_k: int = 0,
                 prefill: str = "exact", speculative: int = 0,
                 adapters: dict = None, max_adapters: int = None,
                 lora_rank: int = 16, sampling: str = "engine",
                 top_p: float = 1.0, min_p: float = 0.0,
                 logit_processors: bool = False,
                 prefix_cache_blocks: int = 0, **class_args):
        import queue as queue_mod
        import threading

        from ..serving.v2_serving import V2ModelServer  # noqa: F401

        self.name = name
        self.context = context
        self.model_path = model_path
        self.ready = False
        self.error = ""
        self.protocol = "v2"
        self.model_spec = None
        self._model_logger = None
        self._params = class_args
        self.cfg_name = config or "llama-3-8b"
        self.batch_size = batch_size
        self.max_new_tokens = max_new_tokens
        self.device = device
        self.use_graph = use_graph
        self.weight_dtype = weight_dtype
        self.kv_dtype = kv_dtype
        self.scheduling = scheduling  # "batch" | "continuous"
        # continuous admission: "exact" = one prefill_slots pass per
        # distinct prompt length; "packed" = one prefill_packed pass
        # over the whole mixed-length group (bf16 KV only)
        if prefill not in ("exact", "packed"):
            raise ValueError(f"unknown prefill mode {prefill!r} "
                             "(expected 'exact' or 'packed')")
        self.prefill = prefill
        self.stop_token = stop_token  # finish a request at this token
        self.temperature = float(temperature)
        self.top_k = int(top_k)
        # speculative=k > 0: batch scheduling drafts k tokens per step
        # by n-gram lookup and verifies them in one pass (greedy, bf16)
        self.speculative = int(speculative)
        # multi-LoRA: {name: model uri or state file}; a request picks
        # one with "adapter": name.  Table slot = position in the dict.
        self.adapters = dict(adapters or {})
        self.adapter_slots = {name: slot for slot, name
                              in enumerate(self.adapters)}
        self.max_adapters = len(self.adapters) if max_adapters is None \
            else int(max_adapters)
        if self.max_adapters < len(self.adapters):
            raise ValueError(
                f"max_adapters={self.max_adapters} is below the "
                f"{len(self.adapters)} adapters configured")
        self.lora_rank = int(lora_rank)
        self._lora_requests = {name: 0 for name in self.adapters}
        self._lora_lock = threading.Lock()
        if sampling not in ("engine", "request"):
            raise ValueError(f"unknown sampling mode {sampling!r} "
                             "(expected 'engine' or 'request')")
        self.sampling = sampling
        self.logit_processors = bool(logit_processors)
        if self.logit_processors and sampling != "request":
            raise ValueError(
                f"logit_processors=True needs sampling=\"request\", got "
                f"sampling={sampling!r}")
        self._sampling_defaults = None
        self._sampling_counts = {"requests": 0, "sampled": 0, "greedy": 0}
        if sampling == "request":
            if self.temperature < 0:
                raise ValueError(
                    f"temperature={temperature} conflicts with "
                    'sampling="request": per-slot temperatures are the '
                    "request field there, the default must be >= 0")
            # the constructor's values are the requests' defaults
            self._sampling_defaults = SamplingParams(
                temperature=temperature, top_k=top_k, top_p=top_p,
                min_p=min_p).validate()
        self._check_speculative_config()
        # prefix cache: N pool blocks of 32 tokens per replica (0 = off)
        self.prefix_cache_blocks = int(prefix_cache_blocks)
        if self.prefix_cache_blocks < 0:
            raise ValueError(
                f"prefix_cache_blocks={prefix_cache_blocks} is negative")
        if self.prefix_cache_blocks > 0 and kv_dtype == "fp8":
            raise ValueError(
                f"prefix_cache_blocks={prefix_cache_blocks} conflicts with "
                'kv_dtype="fp8": cached prefixes are bf16 KV rows')
        if self.prefix_cache_blocks > 0 and self.speculative > 0:
            raise ValueError(
                f"prefix_cache_blocks={prefix_cache_blocks} conflicts with "
                f"speculative={self.speculative}: the speculative path "
                "prefills without the cache")
        self.replicas = max(int(replicas), 1)
        self.engines: typing.List[LlamaDecodeEngine] = []
        self.batch_window_ms = batch_window_ms
        self._tasks: "queue_mod.Queue" = queue_mod.Queue()
        self._workers: typing.List[threading.Thread] = []
        self._pending = []          # [(prompt, max_new, future)]
        self._pending_cv = threading.Condition()
        self._batcher = None
        self.engine_calls = 0

    @property
    def engine(self):
        return self.engines[0] if self.engines else None

    def _check_speculative_config(self):
        """speculative > 0 only combines with greedy batch scheduling
        on bf16 weights and a bf16 KV cache; name the conflict."""
        k = self.speculative
        if k == 0:
            return
        if self.sampling == "request":
            raise ValueError(
                f'speculative={k} conflicts with sampling="request": '
                "speculative decoding is greedy only")
        if self.max_adapters > 0:
            raise ValueError(
                f"speculative={k} conflicts with LoRA adapters "
                f"({sorted(self.adapters)}): the verify pass runs the "
                "base weights only")
        if not 1 <= k <= ops.VERIFY_MAX_QL - 1:
            raise ValueError(
                f"speculative={k} is outside [0, {ops.VERIFY_MAX_QL - 1}]")
        if self.scheduling == "continuous":
            raise ValueError(
                f'speculative={k} conflicts with scheduling="continuous" '
                "(its output ring takes one token per slot per step): "
                'use scheduling="batch"')
        if self.temperature != 0.0:
            raise ValueError(
                f"speculative={k} conflicts with temperature="
                f"{self.temperature}: speculative decoding is greedy only")
        if self.kv_dtype == "fp8":
            raise ValueError(
                f'speculative={k} conflicts with kv_dtype="fp8": the '
                "verify attention kernel reads bf16 caches only")
        if self.weight_dtype == "fp8w":
            raise ValueError(
                f'speculative={k} conflicts with weight_dtype="fp8w": '
                "the verify pass runs on the bf16 weights")

    def post_init(self, mode="sync"):
        stream = getattr(self.context, "stream", None) if self.context \
            else None
        if stream is not None:
            from ..serving.v2_serving import _ModelLogPusher

            self._model_logger = _ModelLogPusher(self, stream)
        if mode == "sync":
            self.load()
            self.ready = True

    def _build_config(self) -> LlamaConfig:
        if self.cfg_name in ("llama-3-8b", "8b"):
            cfg = LlamaConfig.llama3_8b()
        elif self.cfg_name in ("llama-3-70b", "70b"):
            cfg = LlamaConfig.llama3_70b()
        elif self.cfg_name == "tiny":
            cfg = LlamaConfig.tiny()
        elif isinstance(self.cfg_name, LlamaConfig):
            cfg = self.cfg_name
        else:
            raise ValueError(f"unknown llama config {self.cfg_name}")
        for key, value in self._params.items():
            if hasattr(cfg, key):
                setattr(cfg, key, value)
        return cfg

    def load(self):
        import threading

        cfg = self._build_config()
        self._check_speculative_config()
        if self.prefill == "packed" and self.kv_dtype == "fp8":
            raise ValueError(
                'prefill="packed" needs a bf16 KV cache (the packed '
                'attention kernel does not read fp8 caches): use '
                'kv_dtype="bf16" or prefill="exact"')
        if not torch.cuda.is_available():
            self.replicas = 1
        # sampling="request": the engine-wide temperature / top_k stay
        # off, the constructor's values are per-request defaults
        by_request = self.sampling == "request"
        engine_temp = 0.0 if by_request else self.temperature
        engine_top_k = 0 if by_request else self.top_k
        first = LlamaDecodeEngine(cfg, self.batch_size, device=self.device,
                                  use_graph=self.use_graph,
                                  weight_dtype=self.weight_dtype,
                                  kv_dtype=self.kv_dtype,
                                  temperature=engine_temp,
                                  top_k=engine_top_k,
                                  max_adapters=self.max_adapters,
                                  lora_rank=self.lora_rank,
                                  sampling=self.sampling,
                                  logit_processors=self.logit_processors,
                                  prefix_cache_blocks=self.prefix_cache_blocks)
        self.engines = [first]
        for _ in range(self.replicas - 1):
            replica = LlamaDecodeEngine(
                cfg, self.batch_size, device=self.device,
                use_graph=self.use_graph, weights=first.weights,
                weight_dtype="bf16", kv_dtype=self.kv_dtype,
                temperature=engine_temp, top_k=engine_top_k,
                lora=first.lora, sampling=self.sampling,
                logit_processors=self.logit_processors,
                prefix_cache_blocks=self.prefix_cache_blocks)
            replica.weight_dtype = first.weight_dtype
            replica._fp8_packs = first._fp8_packs  # shared packs
            if first.weight_dtype == "fp8w" and replica.on_gpu:
                import torch as _torch

                replica.buf_a8 = _torch.empty_like(first.buf_a8)
                replica.buf_a_scale = _torch.empty_like(
                    first.buf_a_scale)
                replica.buf_h8 = _torch.empty_like(first.buf_h8)
                replica.buf_h8_scale = _torch.empty_like(
                    first.buf_h8_scale)
            self.engines.append(replica)
        # load a checkpoint artifact if given (model_spec.yaml layout)
        if self.model_path:
            from ..artifacts import get_model

            model_file, spec, extra = get_model(self.model_path)
            state = torch.load(model_file, map_location=first.device,
                               weights_only=True)
            first.weights.load_state_dict(state)
            first.rebuild_fp8_packs()  # packs quantized pre-load are
            self.model_spec = spec     # stale (fp8w + model_path)
            for replica in self.engines[1:]:
                replica._fp8_packs = first._fp8_packs
        # adapters go into the shared table slots before any capture
        for name, path in self.adapters.items():
            from ..artifacts import get_model

            adapter_file, _, _ = get_model(path)
            state = torch.load(adapter_file, map_location="cpu",
                               weights_only=True)
            first.load_adapter(self.adapter_slots[name], state)
        for idx, engine in enumerate(self.engines):
            engine._serve_stream = torch.cuda.Stream() \
                if engine.on_gpu else None
            if engine.use_graph:
                # capture sequentially before workers start (concurrent
                # captures on one device conflict); cache state is
                # restored by capture_graph
                if engine._serve_stream is not None:
                    with torch.cuda.stream(engine._serve_stream):
                        engine.capture_graph()
                    engine._serve_stream.synchronize()
                else:
                    engine.capture_graph()
            target = self._continuous_loop \
                if self.scheduling == "continuous" else self._worker_loop
            worker = threading.Thread(target=target,
                                      args=(engine,), daemon=True,
                                      name=f"llama-worker-{self.name}-{idx}")
            worker.start()
            self._workers.append(worker)

    def shutdown(self):
        """Stop the worker/batcher threads (one sentinel per engine).
        In-flight requests finish first; daemon threads would
        otherwise live until process exit (test hygiene)."""
        self._stopping = True
        with self._pending_cv:
            self._pending_cv.notify_all()
        for _ in self.engines:
            self._tasks.put(None)
        for worker in self._workers:
            worker.join(timeout=10)
        self._workers = []
        if self._batcher is not None:
            self._batcher.join(timeout=10)
            self._batcher = None

    def _worker_loop(self, engine: LlamaDecodeEngine):
        while True:
            item = self._tasks.get()
            if item is None:
                return
            prompts, max_new, future = item[:3]
            ids = item[3] if len(item) > 3 else None  # adapter slots
            # SamplingParams per prompt (sampling="request")
            params = item[4] if len(item) > 4 else None
            try:
                if engine._serve_stream is not None:
                    with torch.cuda.stream(engine._serve_stream):
                        result = self._generate_on(engine, prompts,
                                                   max_new, ids, params)
                    engine._serve_stream.synchronize()
                else:
                    result = self._generate_on(engine, prompts, max_new,
                                               ids, params)
                future.set_result(result)
            except Exception as exc:
                if not future.done():
                    future.set_exception(exc)

    def _stream_generate(self, inputs, max_new, event, req_temp=None,
                         adapter_id=-1, params=None):
        """Token streaming (continuous scheduling only): yields one
        json line per generated token as the slots produce them; with
        ``"logprobs": true`` (sampling="request") a line carries the
        token's "logprob" as well."""
        import concurrent.futures
        import json as _json
        import queue as queue_mod

        streams = []
        for j, prompt in enumerate(inputs):
            future = concurrent.futures.Future()
            stream_q: "queue_mod.Queue" = queue_mod.Queue()
            self._tasks.put((prompt, max_new, future, stream_q,
                             req_temp, adapter_id,
                             params[j] if params else None))
            streams.append(stream_q)

        def gen():
            done = 0
            indexes = {id(q): i for i, q in enumerate(streams)}
            active = list(streams)
            while active:
                for stream_q in list(active):
                    try:
                        token = stream_q.get(timeout=0.05)
                    except queue_mod.Empty:
                        continue
                    if token is None:
                        active.remove(stream_q)
                        continue
                    line = {"index": indexes[id(stream_q)], "token": token}
                    if isinstance(token, tuple):  # (token, logprob)
                        line["token"], line["logprob"] = token
                    yield _json.dumps(line) + "\n"

        return gen()

    def _continuous_loop(self, engine: LlamaDecodeEngine):
        """Token-level continuous batching: the engine decodes ALL
        slots every step; finished slots free up and new prompts are
        admitted at token boundaries via ``prefill_slots`` — no
        generate-pass barrier (vLLM-style scheduling on the fixed-B
        hipGraph).  Each request is one queue item (prompt, max_new,
        future[, stream queue[, temperature[, adapter slot[,
        SamplingParams]]]])."""
        import contextlib
        import queue as queue_mod

        B = self.batch_size
        ring_len = engine.cfg.max_seq_len
        out_ring = torch.empty(B, ring_len, dtype=torch.int64,
                               device=engine.device)
        slots: list = [None] * B
        step = 0
        # sampling="request": a logprob ring next to the token ring, and
        # every result is a (tokens, logprobs) pair
        by_request = engine.sampling == "request"
        lp_ring = torch.empty(B, ring_len, dtype=torch.float32,
                              device=engine.device) if by_request else None
        # prefix cache on: every admission group goes through
        # prefill_cached, whatever ``prefill`` says
        cached = engine.prefix_index is not None

        def emit(state, token, logprob):
            """One streamed token, with its logprob when asked for."""
            state["stream"].put((token, float(logprob))
                                if state["logprobs"] else token)

        def stream_ctx():
            return torch.cuda.stream(engine._serve_stream) \
                if engine._serve_stream is not None else \
                contextlib.nullcontext()

        if engine.use_graph and engine._graph is None:
            with stream_ctx():
                engine.capture_graph()
        while True:
            free = [i for i in range(B) if slots[i] is None]
            have_active = len(free) < B
            taken = []
            if free:
                try:
                    item = self._tasks.get(block=not have_active)
                    if item is None:
                        return  # shutdown sentinel
                    taken.append(item)
                except queue_mod.Empty:
                    pass
                while len(taken) < len(free):
                    try:
                        item = self._tasks.get_nowait()
                        if item is None:
                            return
                        taken.append(item)
                    except queue_mod.Empty:
                        break
            if taken:
                self.engine_calls += 1
                prompts, admit_slots, admit_ids = [], [], []
                admit_params = []
                for item, slot in zip(taken, free):
                    prompt, max_new, future = item[:3]
                    stream_q = item[3] if len(item) > 3 else None
                    temp = item[4] if len(item) > 4 else None
                    admit_ids.append(item[5] if len(item) > 5 else -1)
                    params = item[6] if len(item) > 6 else None
                    if by_request and params is None:
                        params = self._sampling_defaults
                    admit_params.append(params)
                    if engine.per_slot_temp:
                        engine.buf_temp[slot] = max(
                            float(temp or 0.0), 1e-4)
                    max_new = max(1, min(max_new,
                                         engine.cfg.max_seq_len - 2))
                    keep = engine.cfg.max_seq_len - max_new - 1
                    prompt = list(prompt)[-keep:] or [0]
                    prompts.append(prompt)
                    admit_slots.append(slot)
                    slots[slot] = {"future": future, "max_new": max_new,
                                   "start": step, "produced": 1,
                                   "stream": stream_q,
                                   "logprobs": bool(
                                       by_request and params.logprobs)}
                # prefill per EXACT prompt length: left-padding a
                # mixed-length admission group would make a request's
                # output depend on co-arriving traffic (pad tokens are
                # attended) — measured by the scheduler property test
                by_len: dict = {}
                for prompt, slot, aid in zip(prompts, admit_slots,
                                             admit_ids):
                    by_len.setdefault(len(prompt), []).append(
                        (prompt, slot, aid))
                lora_on = engine.lora is not None
                try:
                    if by_request:
                        # the slots' parameters, before their prefill
                        # samples the first token with them
                        with stream_ctx():
                            engine.set_sampling_slots(admit_slots,
                                                      admit_params)
                    if self.prefill == "packed" or cached:
                        # the whole mixed-length group in ONE pass:
                        # packed rows carry no padding, so the result
                        # is independent of co-arriving traffic too.
                        # With the prefix cache on, the same pass after
                        # the cached blocks were copied into the slots.
                        by_len = {}
                        slot_ids = torch.tensor(admit_slots,
                                                dtype=torch.long)
                        admit = engine.prefill_cached if cached \
                            else engine.prefill_packed
                        with stream_ctx():
                            if lora_on:
                                admit(prompts, admit_slots,
                                      adapters=admit_ids)
                            else:
                                admit(prompts, admit_slots)
                            out_ring[slot_ids, step % ring_len] = \
                                engine.buf_tokens[slot_ids]
                            if by_request:
                                lp_ring[slot_ids, step % ring_len] = \
                                    engine.buf_logprob[slot_ids]
                    for length, group in by_len.items():
                        tokens = torch.tensor(
                            [g[0] for g in group], dtype=torch.int64)
                        slot_ids = torch.tensor(
                            [g[1] for g in group], dtype=torch.long)
                        with stream_ctx():
                            if lora_on:
                                engine.prefill_slots(
                                    tokens, slot_ids,
                                    adapters=[g[2] for g in group])
                            else:
                                engine.prefill_slots(tokens, slot_ids)
                            out_ring[slot_ids, step % ring_len] = \
                                engine.buf_tokens[slot_ids]
                            if by_request:
                                lp_ring[slot_ids, step % ring_len] = \
                                    engine.buf_logprob[slot_ids]
                except Exception as exc:  # admission failed: fail the
                    if by_request:            # requests, free the slots
                        # freed slots decode on: back to greedy, like
                        # every other path that frees one
                        try:
                            with stream_ctx():
                                engine.set_sampling_slots(
                                    admit_slots, [None] * len(admit_slots))
                        except Exception as reset_exc:
                            logger.error("sampling reset failed",
                                         error=str(reset_exc))
                    for slot in admit_slots:
                        state = slots[slot]
                        if state is None:
                            continue
                        if not state["future"].done():
                            state["future"].set_exception(exc)
                        if state["stream"]:
                            state["stream"].put(None)
                        slots[slot] = None
                    logger.error("continuous admission failed",
                                 error=str(exc))
                    continue
                done_at_admit = [
                    slot for slot in admit_slots
                    if slots[slot]["max_new"] <= 1]
                if self.stop_token is not None or done_at_admit:
                    # the ADMISSION token can already be the stop
                    # token, and max_tokens=1 requests finish here
                    if engine._serve_stream is not None:
                        engine._serve_stream.synchronize()
                    first = engine.buf_tokens.cpu()
                    first_lp = engine.buf_logprob.cpu() if by_request \
                        else None
                    for slot in admit_slots:
                        state = slots[slot]
                        token = int(first[slot])
                        if token != self.stop_token and \
                                state["max_new"] > 1:
                            continue
                        logprob = float(first_lp[slot]) if by_request \
                            else None
                        if state["stream"]:
                            emit(state, token, logprob)
                            state["stream"].put(None)
                            state["_first_sent"] = True
                        state["future"].set_result(
                            ([token], [logprob]) if by_request
                            else [token])
                        slots[slot] = None
                        if by_request:
                            with stream_ctx():
                                engine.set_sampling_slots([slot], [None])
            active = [i for i in range(B) if slots[i] is not None]
            if not active:
                continue
            stop = self.stop_token
            streaming = [i for i in active if slots[i]["stream"]]
            if streaming:
                # streamers need the admission token on the host too
                for i in streaming:
                    state = slots[i]
                    if state["produced"] == 1 and \
                            not state.get("_first_sent"):
                        if engine._serve_stream is not None:
                            engine._serve_stream.synchronize()
                        col = state["start"] % ring_len
                        emit(state, int(out_ring[i, col]),
                             lp_ring[i, col] if by_request else None)
                        state["_first_sent"] = True
            with stream_ctx():
                engine.decode_step()
                step += 1
                out_ring[:, step % ring_len].copy_(engine.buf_tokens)
                if by_request:
                    lp_ring[:, step % ring_len].copy_(engine.buf_logprob)
            host_tokens = None
            if streaming or stop is not None:
                if engine._serve_stream is not None:
                    engine._serve_stream.synchronize()
                host_tokens = engine.buf_tokens.cpu()
                host_lp = engine.buf_logprob.cpu() \
                    if by_request and streaming else None
                for i in streaming:
                    emit(slots[i], int(host_tokens[i]),
                         host_lp[i] if by_request else None)
            finished = []
            for i in active:
                state = slots[i]
                state["produced"] += 1
                hit_stop = stop is not None and \
                    int(host_tokens[i]) == stop
                if state["produced"] >= state["max_new"] or hit_stop:
                    state["max_new"] = state["produced"]  # actual len
                    finished.append(i)
            if finished:
                if engine._serve_stream is not None:
                    engine._serve_stream.synchronize()
                for i in finished:
                    state = slots[i]
                    cols = torch.tensor(
                        [(state["start"] + j) % ring_len
                         for j in range(state["max_new"])],
                        dtype=torch.long)
                    cols = cols.to(out_ring.device)
                    result = out_ring[i, cols].cpu().tolist()
                    if by_request:
                        result = (result, lp_ring[i, cols].cpu().tolist())
                    state["future"].set_result(result)
                    if state["stream"]:
                        state["stream"].put(None)  # end-of-stream
                    slots[i] = None
                if engine.lora is not None:
                    # freed slots keep stepping: back to the base model,
                    # so they stop paying for an adapter nobody reads
                    with stream_ctx():
                        engine.buf_adapter[torch.tensor(
                            finished, dtype=torch.long)] = -1
                if by_request:
                    # freed slots keep stepping too: greedy is cheapest
                    with stream_ctx():
                        engine.set_sampling_slots(
                            finished, [None] * len(finished))

    def do_event(self, event):
        import concurrent.futures
        import time as _time

        start = _time.perf_counter()
        body = event.body if isinstance(event.body, dict) else {}
        path = event.path or ""
        if path.endswith("/ready"):
            event.body = {"name": self.name, "ready": self.ready}
            return event
        inputs = body.get("inputs")
        if inputs is None:
            raise ValueError('expected {"inputs": [[token ids], ...]}')
        max_new = int(body.get("max_tokens", self.max_new_tokens))
        req_temp = body.get("temperature")
        adapter_id = self._adapter_slot(body.get("adapter"))
        # sampling="request": one SamplingParams per prompt, else None
        params = self._request_sampling(body, len(inputs))
        if params is not None:
            req_temp = None  # "temperature" is a SamplingParams field
        if self.scheduling == "continuous" and body.get("stream"):
            event.body = self._stream_generate(inputs, max_new, event,
                                               req_temp, adapter_id, params)
            return event
        if self.scheduling == "continuous":
            futures = []
            for j, prompt in enumerate(inputs):
                future = concurrent.futures.Future()
                self._tasks.put((prompt, max_new, future, None,
                                 req_temp, adapter_id,
                                 params[j] if params else None))
                futures.append(future)
            outputs = [f.result(timeout=600) for f in futures]
        elif self.batch_window_ms and len(inputs) < self.batch_size:
            outputs = self._batched_submit(inputs, max_new, adapter_id,
                                           params)
        else:
            futures = []
            for chunk_start in range(0, len(inputs), self.batch_size):
                chunk = inputs[chunk_start:chunk_start + self.batch_size]
                future = concurrent.futures.Future()
                self._tasks.put((
                    chunk, max_new, future, [adapter_id] * len(chunk),
                    params[chunk_start:chunk_start + self.batch_size]
                    if params else None))
                futures.append(future)
            outputs = []
            for future in futures:
                outputs.extend(future.result(timeout=600))
        event.body = {"id": event.id, "model_name": self.name,
                      "outputs": outputs}
        if params is not None:
            # rows are (tokens, logprobs) pairs in this mode
            event.body["outputs"] = [row[0] for row in outputs]
            if body.get("logprobs"):
                event.body["logprobs"] = [row[1] for row in outputs]
        if "retrieval" in body:  # RAG upstream step metadata
            event.body["retrieval"] = body["retrieval"]
        if self._model_logger:
            self._model_logger.push(start, {"inputs": [len(inputs)]},
                                    event.body)
        return event

    def _request_sampling(self, body: dict, n_prompts: int):
        """The request's sampling fields as one SamplingParams per
        prompt (sampling="request"; None otherwise, and then no field
        is looked at).  Absent fields take the server's defaults, prompt
        j draws with seed + j, an absent seed is drawn at random.  A
        field out of range is a ValueError naming it, which fails this
        request alone.  A logit_processors=True server also reads the
        penalties and ``logit_bias`` and checks the bias ids against the
        vocabulary here; without the flag those fields stay unread."""
        if self.sampling != "request":
            return None
        import dataclasses
        import random

        base = self._sampling_defaults
        names = ("temperature", "top_k", "top_p", "min_p", "seed",
                 "logprobs")
        if self.logit_processors:
            names += ("repetition_penalty", "presence_penalty",
                      "frequency_penalty", "logit_bias")
        fields = {name: body[name] for name in names
                  if body.get(name) is not None}
        first = dataclasses.replace(base, **fields).validate()
        if self.logit_processors:
            # here, not at admission: a failure there would fail every
            # request admitted together with this one
            self.engine._check_processors(first)
        if "seed" not in fields:
            first.seed = random.SystemRandom().getrandbits(63)
        with self._lora_lock:
            self._sampling_counts["requests"] += 1
            self._sampling_counts[
                "sampled" if first.temperature > 0 else "greedy"] += 1
        return [dataclasses.replace(first,
                                    seed=(first.seed + j) % (1 << 63))
                for j in range(n_prompts)]

    def _adapter_slot(self, name) -> int:
        """Table slot of a request's "adapter" field; absent or null
        selects the base model (-1).  An unknown name fails the request
        that carries it, nothing else."""
        if name is None:
            return -1
        if name not in self.adapter_slots:
            raise ValueError(
                f"unknown adapter {name!r}; loaded adapters: "
                f"{sorted(self.adapter_slots)}")
        with self._lora_lock:
            self._lora_requests[name] += 1
        return self.adapter_slots[name]

    def _batched_submit(self, inputs: list, max_new: int,
                        adapter_id: int = -1, params: list = None) -> list:
        """Queue small requests; the batcher gathers up to batch_size
        prompts within batch_window_ms and submits ONE engine task."""
        import concurrent.futures
        import threading

        futures = []
        with self._pending_cv:
            if self._batcher is None:
                self._batcher = threading.Thread(
                    target=self._batch_loop, daemon=True,
                    name=f"llama-batcher-{self.name}")
                self._batcher.start()
            for j, prompt in enumerate(inputs):
                future = concurrent.futures.Future()
                self._pending.append((prompt, max_new, future, adapter_id,
                                      params[j] if params else None))
                futures.append(future)
            self._pending_cv.notify()
        return [f.result(timeout=600) for f in futures]

    def _batch_loop(self):
        import concurrent.futures
        import time as _time

        while not getattr(self, "_stopping", False):
            with self._pending_cv:
                while not self._pending:
                    self._pending_cv.wait()
                    if getattr(self, "_stopping", False):
                        return
            _time.sleep(self.batch_window_ms / 1000.0)
            with self._pending_cv:
                batch, self._pending = \
                    self._pending[:self.batch_size], \
                    self._pending[self.batch_size:]
            if not batch:
                continue
            prompts = [b[0] for b in batch]
            max_new = max(b[1] for b in batch)
            task_future = concurrent.futures.Future()
            # one engine pass may mix adapters: one id per prompt
            ids = [b[3] if len(b) > 3 else -1 for b in batch]
            # ... and parameter sets: one SamplingParams per prompt
            params = [b[4] if len(b) > 4 else None for b in batch]
            self._tasks.put((prompts, max_new, task_future, ids, params))
            try:
                results = task_future.result(timeout=600)
                for entry, result in zip(batch, results):
                    if isinstance(result, tuple):  # (tokens, logprobs)
                        result = tuple(part[:entry[1]] for part in result)
                    else:
                        result = result[:entry[1]]
                    entry[2].set_result(result)
            except Exception as exc:
                for entry in batch:
                    if not entry[2].done():
                        entry[2].set_exception(exc)

    def _generate_on(self, engine: LlamaDecodeEngine, prompts: list,
                     max_new: int, adapters: list = None,
                     params: list = None) -> list:
        """Batch generation with per-LENGTH prefill groups: padding a
        mixed-length batch would let pad tokens be attended, making a
        prompt's output depend on its co-batch (see the continuous
        scheduler property test).  On a sampling="request" engine
        ``params`` holds one SamplingParams per prompt (None = the
        server's defaults) and every row of the result is a
        (tokens, logprobs) pair."""
        self.engine_calls += 1
        n = len(prompts)
        by_len: dict = {}
        for i, prompt in enumerate(prompts):
            by_len.setdefault(len(prompt), []).append(i)
        engine.reset()
        by_request = engine.sampling == "request"
        if by_request:
            # rows beyond n decode greedily: they are never read
            row_params = [self._sampling_defaults] * n if params is None \
                else [self._sampling_defaults if item is None else item
                      for item in params]
            engine.set_sampling_slots(
                range(engine.B), row_params + [None] * (engine.B - n))
        lora_on = engine.lora is not None
        if lora_on:
            engine.buf_adapter.fill_(-1)  # rows beyond n run the base
        if engine.prefix_index is not None:
            # prefix cache on: rows 0..n-1 in ONE pass over what the
            # pool does not hold (packed rows carry no padding either)
            by_len = {}
            if lora_on and adapters is not None:
                engine.prefill_cached(prompts, range(n), adapters=adapters)
            else:
                engine.prefill_cached(prompts, range(n))
        for length, idxs in by_len.items():
            tokens = torch.tensor([prompts[i] for i in idxs],
                                  dtype=torch.int64)
            slot_ids = torch.tensor(idxs, dtype=torch.long)
            if lora_on and adapters is not None:
                engine.prefill_slots(tokens, slot_ids,
                                     adapters=[adapters[i] for i in idxs])
            else:
                engine.prefill_slots(tokens, slot_ids)
        if self.speculative > 0:
            out = self._speculate_on(engine, prompts, max_new)
        else:
            if engine.use_graph and engine._graph is None:
                engine.capture_graph()
            generated = [engine.buf_tokens.clone()]
            logprobs = [engine.buf_logprob.clone()] if by_request else None
            for _ in range(max_new - 1):
                engine.decode_step()
                generated.append(engine.buf_tokens.clone())
                if by_request:
                    logprobs.append(engine.buf_logprob.clone())
            out = torch.stack(generated, dim=1)
        rows = out[:n].cpu().tolist()
        if self.stop_token is not None:
            trimmed = []
            for row in rows:
                if self.stop_token in row:
                    row = row[:row.index(self.stop_token) + 1]
                trimmed.append(row)
            rows = trimmed
        if by_request:
            lp_rows = torch.stack(logprobs, dim=1)[:n].cpu().tolist()
            return [(row, lp[:len(row)]) for row, lp in zip(rows, lp_rows)]
        return rows

    def _speculate_on(self, engine: LlamaDecodeEngine, prompts: list,
                      max_new: int) -> torch.Tensor:
        """The decode loop of _generate_on in speculative mode: the
        prompts (already prefilled into rows 0..n-1) seed the draft
        history, rows beyond them have length 0 and stay frozen."""
        k = self.speculative
        n, B = len(prompts), engine.B
        smax = engine.cfg.max_seq_len
        longest = max(len(p) for p in prompts)
        if longest + max_new + k > smax:
            raise ValueError(
                f"speculative={k}: a prompt of {longest} tokens plus "
                f"max_tokens={max_new} plus {k} drafted tokens exceeds "
                f"max_seq_len {smax}")
        host = torch.zeros(B, smax, dtype=torch.int64)
        lens = [len(p) for p in prompts] + [0] * (B - n)
        for i, prompt in enumerate(prompts):
            host[i, :len(prompt)] = torch.tensor(prompt, dtype=torch.int64)
        history = host.to(engine.device)
        start_lens = torch.tensor(lens, dtype=torch.int32
                                  ).to(engine.device)
        active = torch.arange(B, device=engine.device) < n
        # the prefill token is the first generated one
        history.scatter_(1, start_lens.view(B, 1).long(),
                         (engine.buf_tokens * active).view(B, 1))
        hist_lens = start_lens + active.to(torch.int32)
        return engine._speculative_loop(history, hist_lens, start_lens,
                                        active, max_new, k, 2)

    def logged_results(self, request, response, op):
        return request.get("inputs"), None

    def stats(self):
        out = self._feature_stats()
        if self.prefix_cache_blocks > 0:
            # summed over the replicas, each of which has its own pool
            names = (("requests", "lookups"),
                     ("prompt_tokens", "prompt_tokens"),
                     ("hit_tokens", "hit_tokens"),
                     ("blocks", "blocks_in_use"), ("capacity", "capacity"),
                     ("evictions", "evicted"))
            totals = {key: 0 for key, _ in names}
            for engine in self.engines:
                counters = engine.prefix_stats
                for key, source in names:
                    totals[key] += counters[source]
            out["prefix_cache"] = totals
        return out

    def _feature_stats(self):
        if self.sampling == "request":
            with self._lora_lock:
                out = {"sampling": dict(self._sampling_counts)}
                if self.adapters:
                    out["lora"] = {"adapters": list(self.adapters),
                                   "requests": dict(self._lora_requests)}
            return out
        if self.adapters:
            with self._lora_lock:
                counts = dict(self._lora_requests)
            return {"lora": {"adapters": list(self.adapters),
                             "requests": counts}}
        if not self.speculative:
            return {}
        totals = {"steps": 0, "drafted": 0, "accepted": 0}
        for engine in self.engines:
            for key in totals:
                totals[key] += engine.spec_stats[key]
        return {"speculative": totals}
