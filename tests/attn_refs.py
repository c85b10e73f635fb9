# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""float64 reference, error bound, input cases and mutants of the MFMA
attention kernels attn_prefill and attn_verify, shared by
test_attn_mfma.py (CPU) and test_attn_mfma_gpu.py.  Everything here runs
on the CPU.

Reference.  Query j of sequence i sits at position pos = kv_start[i] + j
and sees rows 0..pos of cache[slots[i], h // G]; attn_verify is the same
with kv_start = base_lens, every sequence QL rows long and on its own
cache row.  The reference is softmax(q . k * scale) . v in float64 on
the bf16 values the kernel reads, one sequence at a time.

Bound.  What the shared tile loop (pf_tile) does to one output row:

* a score is an fp32 MFMA sum of D exact products (bf16 x bf16 is exact
  in fp32), then x = s * (scale * log2 e): by the n-term rule of
  decode_refs (n * 2^-24 * sum|terms|) and with four more roundoffs for
  the scaling, the subtraction of the maximum and the exponential's
  argument, x is off by at most
      delta = (D + 4) * 2^-24 * scale * log2(e) * max_i(|k_i| . |q|)
  over the keys i the row sees;
* p_i = exp2(x_i - m) in fp32: the running maximum m carries the same
  error as the scores, so the exponent is off by 2 * delta and p_i by
  the relative 2 * ln(2) * delta;
* l sums the unrounded fp32 p_i over the keys of a tile, the tiles are
  folded with a rescale each, the splits of attn_verify once more, and
  1 / l and the product with o follow; the P.V sum is an fp32 MFMA sum
  of as many terms as the row has keys.  Together
      (keys + tiles + nsplit + 8) * 2^-24;
* so every weight the kernel uses, and its sum l, are within the
  relative
      E = 2 ln(2) delta + (keys + tiles + nsplit + 8) * 2^-24
  of the exact ones, E computed per (row, head) from the inputs;
* P is rounded ONCE to bf16 (round to nearest even) before the P.V MFMA:
  the numerator's weights are off by the relative R1 + E, the
  denominator's by E.  With w the exact softmax, A = sum_i w_i |v_i|
  (per row and dim) and ref = sum_i w_i v_i, the fp32 value before the
  last rounding is
      o = (ref + e_num) / (1 + e_l),  |e_num| <= (R1 + E) A, |e_l| <= E
  hence |o - ref| <= ((R1 + E) A + E |ref|) / (1 - E);
* o * (1 / l) is rounded once to bf16: R1 |ref| + (1 + R1) |o - ref|.

      bound = R1 |ref| + (1 + R1) ((R1 + E) A + E |ref|) / (1 - E)

Every number in it is R1 = 2^-8, 2^-24 or a count taken from the inputs;
no term comes from a kernel's output.  The MFMA itself has no term:
docs/kernels.md measured that v_mfma_f32_16x16x32_bf16 accumulates in
fp32.  The bound is first order in E, so test_attn_mfma.py asserts
E <= R1 / 2 on every row of every case.

Cases.  Smax = 261 is no multiple of 64 or 4.  q, K and V are N(0,1)
rounded to bf16.  A ramp case adds 0.5 to q and RAMP * i (rising) or
RAMP * (kv_end - 1 - i) (falling) to key row i, as decode_refs.attn_case
does, so that the newest keys (rising) or key 0 (falling) carry the
weight of every row.  `keys` / `vals` are float64 and finite everywhere;
the bf16 caches the kernels get hold NaN at and past each sequence's end
and in every slot no live sequence uses.

Mutants.  `mutant(case, name)` is the reference with one defect, and the
(row, head) pairs the defect touches."""

import math

import torch

from decode_refs import (EPS32, R1, check, f64, rope_reference, same_bits,
                         sentinel_bf16)

D = 128
SMAX = 261
TILE = 64
SCALE = 1.0 / math.sqrt(D)
LOG2E = 1.4426950408889634
RAMP = 0.04

NSPLITS = (1, 2, 3, 4, 16)

# (Hq, Hkv); the last one is G = 3
PREFILL_HEADS = ((8, 2), (2, 2), (8, 1), (6, 2))
# (length, kv_start) of the sequences of one packed call
PREFILL_SEQS = {
    "lengths": ((1, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0),
                (65, 0), (130, 0)),
    # the diagonal on every side of need_mask = tile0 + 63 > wave_min_pos
    # and of the tile skip tile0 > wave_max_pos; the last ends at Smax
    "diagonal": ((17, 47), (17, 48), (33, 63), (33, 64), (1, 63), (1, 64),
                 (64, 64), (65, 127), (70, 7), (5, 256)),
}
PREFILL_RAMP_SEQS = ((130, 0), (130, 40), (200, 0), (200, 40))
# (length, kv_start, slot): a zero-length sequence, slot -1, slot B and
# start -1 between good ones; slot None = the builder picks
PREFILL_GUARD_SEQS = ((17, 0, None), (0, 5, None), (9, 3, -1),
                      (20, 0, None), (7, 2, "B"), (5, -1, None),
                      (33, 64, None))

# (Hq, Hkv, QL): G * QL = 1, 4, 16, 21, 35, 35, 56, 64
VERIFY_SHAPES = ((2, 2, 1), (4, 2, 2), (8, 2, 4), (6, 2, 7), (10, 2, 7),
                 (14, 2, 5), (16, 2, 7), (16, 2, 8))
VERIFY_RAMP_SHAPE = (6, 2, 7)


def verify_bases(ql):
    return (0, 1, 63, 64, 65, 200, SMAX - ql)


def verify_guard_bases(ql):
    """Rows 1 and 3 are the two the kernels skip."""
    return (0, -1, 63, SMAX - ql + 1, 65, 200, SMAX - ql)


# ------------------------------------------------------------ reference

def attend(q, keys, vals, pos, kvh, visible=None, tiles=1, scale=SCALE):
    """q [n, Hq, D], keys / vals [Hkv, S, D] f64, pos [n], kvh [Hq] the
    KV head of each q head.  Row r sees the keys of visible[r] (default:
    key <= pos[r]).  Returns ref and A [n, Hq, D] and the weight error E
    [n, Hq] without its nsplit term."""
    S = keys.shape[1]
    if visible is None:
        visible = torch.arange(S)[None, :] <= pos[:, None]
    k, v = keys[kvh], vals[kvh]                         # [Hq, S, D]
    hidden = ~visible[:, None, :]
    x = torch.einsum("nhd,hsd->nhs", q, k) * scale
    w = torch.softmax(x.masked_fill(hidden, -math.inf), -1)
    ref = torch.einsum("nhs,hsd->nhd", w, v)
    A = torch.einsum("nhs,hsd->nhd", w, v.abs())
    mag = torch.einsum("nhd,hsd->nhs", q.abs(), k.abs())
    mag = mag.masked_fill(hidden, 0.0).amax(-1)
    delta = (D + 4) * EPS32 * scale * LOG2E * mag
    nkeys = visible.sum(-1)[:, None].to(torch.float64)
    E = 2 * math.log(2) * delta + (nkeys + tiles + 8) * EPS32
    return ref, A, E


def bound(case, nsplit=1):
    E = (case["E"] + nsplit * EPS32)[..., None]
    ref = case["ref"].abs()
    return R1 * ref + (1 + R1) * ((R1 + E) * case["A"] + E * ref) / (1 - E)


def _skipped(rule, length, start, slot, B):
    if rule == "verify":
        return start < 0 or start + length > SMAX
    return not 0 <= slot < B or start < 0


def _reference(case, edit=None, wide=False):
    """ref, A, E over all rows; rows of skipped sequences stay zero.
    edit(i, pos, S) -> (pos, visible, kvh) changes one sequence's query
    positions, visibility or head map (the mutants).  wide: the keys are
    the whole (finite) float64 row of the slot, for the mutants that
    look one key past a sequence's end."""
    T, Hq = case["q"].shape[:2]
    ref = torch.zeros(T, Hq, D, dtype=torch.float64)
    A, E = torch.zeros_like(ref), torch.zeros(T, Hq, dtype=torch.float64)
    q = f64(case["q"])
    for i, (length, start, slot) in enumerate(case["seqs"]):
        if not case["live_seq"][i] or length == 0:
            continue
        row0 = case["cu"][i]
        end = min(start + length, SMAX)
        S = SMAX if wide else end
        pos = start + torch.arange(length)
        visible, kvh = None, case["kvh"]
        if edit is not None:
            pos, visible, kvh = edit(i, pos, S)
        rows = slice(row0, row0 + length)
        ref[rows], A[rows], E[rows] = attend(
            q[rows], case["keys"][slot][:, :S], case["vals"][slot][:, :S],
            pos, kvh, visible, tiles=(end + TILE - 1) // TILE)
    return ref, A, E


_CASES = {}


def build_case(Hq, Hkv, seqs, ramp=0.0, rule="prefill", nslots=None,
               seed=0):
    """seqs: (length, kv_start[, slot]) per sequence of the packed call.
    Without a slot the sequences get distinct slots out of order among
    nslots = len(seqs) + 2 (two slots stay unused); rule "verify" puts
    sequence i on slot i of len(seqs)."""
    key = (Hq, Hkv, tuple(seqs), ramp, rule, nslots, seed)
    if key in _CASES:
        return _CASES[key]
    n = len(seqs)
    B = nslots or (n if rule == "verify" else n + 2)
    g = torch.Generator().manual_seed(
        7919 * Hq + 131 * Hkv + 17 * n + sum(s[0] + s[1] for s in seqs) +
        int(ramp * 1e4) + seed + 10 ** 6)
    order = torch.randperm(B, generator=g).tolist()
    full = []
    for i, s in enumerate(seqs):
        slot = s[2] if len(s) > 2 else None
        if slot is None:
            slot = i if rule == "verify" else order[i]
        full.append((s[0], s[1], B if slot == "B" else slot))
    lens = [s[0] for s in full]
    cu = [0]
    for length in lens:
        cu.append(cu[-1] + length)
    T = cu[-1]
    q = torch.randn(T, Hq, D, generator=g)
    k = torch.randn(B, Hkv, SMAX, D, generator=g)
    v = torch.randn(B, Hkv, SMAX, D, generator=g)
    live_seq = [not _skipped(rule, *s, B) for s in full]
    dead = torch.ones(B, SMAX, dtype=torch.bool)
    for (length, start, slot), live in zip(full, live_seq):
        if not live:
            continue
        end = min(start + length, SMAX)
        dead[slot, :end] = False
        if ramp:
            rows = torch.arange(SMAX, dtype=torch.float32)
            step = rows if ramp > 0 else (end - 1 - rows)
            k[slot] += (abs(ramp) * step).view(1, SMAX, 1)
    if ramp:
        q += 0.5
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    G = Hq // Hkv
    live = torch.zeros(T, dtype=torch.bool)
    for i in range(n):
        live[cu[i]:cu[i + 1]] = live_seq[i]
    case = dict(Hq=Hq, Hkv=Hkv, G=G, B=B, T=T, seqs=full, cu=cu,
                live_seq=live_seq, live=live, ramp=ramp, rule=rule, q=q,
                keys=f64(k), vals=f64(v), kvh=torch.arange(Hq) // G,
                cu_seqlens=torch.tensor(cu, dtype=torch.int32),
                slots=torch.tensor([s[2] for s in full], dtype=torch.int32),
                kv_start=torch.tensor([s[1] for s in full],
                                      dtype=torch.int32),
                max_q_len=max(lens))
    dead = dead[:, None, :].expand(B, Hkv, SMAX)
    k[dead] = float("nan")
    v[dead] = float("nan")
    case.update(kc=k, vc=v)
    case["ref"], case["A"], case["E"] = _reference(case)
    _CASES[key] = case
    return case


# On a plain case every mutant that applies has to show in every
# sequence (test_attn_mfma.py).  A sequence of one row and two heads has
# two softmax rows to show it in, so two cases take the first seed at
# which their inputs do, instead of seed 0.
SEEDS = {(2, 2, "diagonal"): 1, (4, 2, 2): 6}


def prefill_case(heads, name):
    return build_case(*heads, PREFILL_SEQS[name],
                      seed=SEEDS.get((*heads, name), 0))


# On a ramp case a mask mutant has to show on EVERY (row, head) pair it
# touches.  A key's score carries N(0,1) noise of standard deviation 1.1
# and a step of the ramp is 0.23, so with seed 0 a few pairs in a
# thousand have the one key in question two standard deviations low and
# miss the factor (a steeper ramp would break E <= R1 / 2).  Each ramp
# case is therefore one sequence with Hq 4, Hkv 2 (520 or 800 pairs; the
# verify case has 294) and takes the first seed at which every mutant of
# its ramp reaches 4.1 times the bound on every pair and E <= 0.495 R1;
# the seeds follow from the float64 references alone.
RAMP_HEADS = (4, 2)
RAMP_SEEDS = {(1, 130, 0): 2, (1, 130, 40): 11, (1, 200, 0): 8,
              (1, 200, 40): 73, (-1, 130, 0): 1, (-1, 130, 40): 3,
              (-1, 200, 0): 0, (-1, 200, 40): 4,
              (1, "verify"): 1, (-1, "verify"): 0}


def prefill_ramp_case(sign, seq):
    """One sequence (length, kv_start) of PREFILL_RAMP_SEQS."""
    return build_case(*RAMP_HEADS, (seq,), ramp=sign * RAMP,
                      seed=RAMP_SEEDS[(sign, *seq)])


def verify_ramp_case(sign):
    return verify_case(*VERIFY_RAMP_SHAPE, ramp=sign * RAMP)


def prefill_guard_case():
    return build_case(8, 2, PREFILL_GUARD_SEQS)


def verify_case(Hq, Hkv, QL, ramp=0.0, bases=None):
    bases = bases or verify_bases(QL)
    return build_case(Hq, Hkv, tuple((QL, b) for b in bases), ramp=ramp,
                      rule="verify",
                      seed=RAMP_SEEDS[(1 if ramp > 0 else -1, "verify")]
                      if ramp else SEEDS.get((Hq, Hkv, QL), 0))


# -------------------------------------------------------------- mutants

MUTANTS = ("leak", "no_diagonal", "no_key0", "no_tile_first", "start+1",
           "start-1", "head_mod", "swap_gj")


def mutant(case, name):
    """The reference with one defect, and the [T, Hq] mask of the (row,
    head) pairs the defect touches (None: it does not apply to the case).

    leak            key pos + 1 is visible (rows whose pos + 1 < Smax)
    no_diagonal     key pos is not (rows with pos >= 1)
    no_key0         key 0 is not (rows with pos >= 1)
    no_tile_first   keys 64, 128, 192, 256 are not (rows with pos >= 64)
    start+1, -1     every position of the sequence moves by one, which
                    for each row is the leak or the dropped diagonal
    head_mod        KV head h % Hkv instead of h // G
    swap_gj         attn_verify's column c = g * QL + j taken apart as
                    (j', g') = (c // G, c % G): the output of (g, j) is
                    the attention of (g', j')"""
    T, Hq, G, Hkv = case["T"], case["Hq"], case["G"], case["Hkv"]
    touched = torch.zeros(T, Hq, dtype=torch.bool)
    if name == "swap_gj":
        QL = case["seqs"][0][0]
        if case["rule"] != "verify" or G == 1 or QL == 1:
            return None, None
        ref = case["ref"].view(-1, QL, Hkv, G, D)
        out = ref.clone()
        mask = touched.view(-1, QL, Hkv, G)
        for g_ in range(G):
            for j in range(QL):
                c = g_ * QL + j
                j2, g2 = c // G, c % G
                out[:, j, :, g_] = ref[:, j2, :, g2]
                mask[:, j, :, g_] = (j2, g2) != (j, g_)
        touched &= case["live"][:, None]
        return out.view(T, Hq, D), touched
    if name == "head_mod":
        kvh = torch.arange(Hq) % Hkv
        if torch.equal(kvh, case["kvh"]):
            return None, None
        touched[:, kvh != case["kvh"]] = True
        touched &= case["live"][:, None]
        return _reference(case, lambda i, pos, S: (pos, None, kvh))[0], \
            touched

    def edit(i, pos, S):
        row0 = case["cu"][i]
        rows = slice(row0, row0 + len(pos))
        keys = torch.arange(S)
        visible = keys[None, :] <= pos[:, None]
        if name in ("leak", "start+1"):
            hit = pos + 1 < SMAX
            visible = keys[None, :] <= (pos + hit.long())[:, None]
        elif name in ("no_diagonal", "start-1"):
            hit = pos >= 1
            visible = keys[None, :] <= (pos - hit.long())[:, None]
        elif name == "no_key0":
            hit = pos >= 1
            visible[hit, 0] = False
        elif name == "no_tile_first":
            hit = pos >= TILE
            visible[:, TILE::TILE] = False
        touched[rows] = hit[:, None]
        return pos, visible, case["kvh"]

    if name not in MUTANTS:
        raise ValueError(name)
    return _reference(case, edit, name in ("leak", "start+1"))[0], touched


def margins(case, out, touched, nsplit=1):
    """|mutant - ref| / bound, the maximum over the head dim: [T, Hq],
    zero where the mutant does not touch."""
    ratio = ((out - case["ref"]).abs() / bound(case, nsplit)).amax(-1)
    return torch.where(touched, ratio, torch.zeros_like(ratio))


# ------------------------------------------- the kernel's arithmetic

def simulate(case, nsplit=1):
    """pf_tile's arithmetic on the CPU: fp32 scores in tiles of 64,
    x = s * (scale * log2 e), a running maximum and fp32 l over the
    unrounded p, P rounded to bf16 before the fp32 P.V sum, o * (1 / l)
    rounded to bf16.  With nsplit > 1 the tiles are dealt to splits and
    folded as attn_verify_combine_kernel folds them."""
    T, Hq = case["q"].shape[:2]
    out = torch.zeros(T, Hq, D, dtype=torch.bfloat16)
    sl2 = torch.tensor(SCALE, dtype=torch.float32) * \
        torch.tensor(LOG2E, dtype=torch.float32)
    q32 = case["q"].float()
    for i, (length, start, slot) in enumerate(case["seqs"]):
        if not case["live_seq"][i] or length == 0:
            continue
        row0 = case["cu"][i]
        S = min(start + length, SMAX)
        q = q32[row0:row0 + length]
        k = case["keys"][slot][case["kvh"]].float()
        v = case["vals"][slot][case["kvh"]].float()
        pos = start + torch.arange(length)
        ntiles = (S + TILE - 1) // TILE
        ns = min(nsplit, ntiles)
        parts = []
        for split in range(ns):
            m = torch.full((length, Hq), -1e30)
            l = torch.zeros(length, Hq)
            o = torch.zeros(length, Hq, D)
            for t in range(split * ntiles // ns, (split + 1) * ntiles // ns):
                keys = torch.arange(t * TILE, min((t + 1) * TILE, S))
                x = torch.einsum("nhd,hsd->nhs", q, k[:, keys]) * sl2
                hidden = (keys[None, :] > pos[:, None])[:, None, :]
                x = x.masked_fill(hidden, -math.inf)
                m_new = torch.maximum(m, x.amax(-1))
                alpha = torch.exp2(m - m_new)
                p = torch.exp2(x - m_new[..., None])
                l = l * alpha + p.sum(-1)
                pb = p.to(torch.bfloat16).float()
                o = o * alpha[..., None] + torch.einsum(
                    "nhs,hsd->nhd", pb, v[:, keys])
                m = m_new
            parts.append((m, l, o))
        m_star = torch.stack([p[0] for p in parts]).amax(0)
        l = sum(torch.exp2(p[0] - m_star) * p[1] for p in parts)
        o = sum(torch.exp2(p[0] - m_star)[..., None] * p[2] for p in parts)
        out[row0:row0 + length] = (o * (1.0 / l)[..., None]).to(
            torch.bfloat16)
    return out


# ------------------------------------------------------- rope_kv_varlen

ROPE_T, ROPE_HQ, ROPE_HKV, ROPE_SLOTS, ROPE_PAD = 37, 4, 2, 3, 24
# (Smax, rows of the cos/sin table): each of the two limits is the
# smaller one once
ROPE_CASES = [(d, smax, table) for d in (128, 64)
              for smax, table in ((20, 16), (16, 20))]
ROPE_SKIPPED = (3, 10, 17, 25, 31)


def rope_varlen_case(d, smax, table_len):
    """37 tokens at distinct (slot, position) pairs scattered over 3
    slots, in a qkv buffer whose rows are 24 columns wider than the
    heads (NaN there).  Tokens 3, 10, 17, 25 and 31 have slot -1,
    slot B, position -1, position Smax and position = the table's
    length: the op skips them."""
    from mlrun_amd import ops

    g = torch.Generator().manual_seed(d + smax)
    heads = ROPE_HQ + 2 * ROPE_HKV
    limit = min(smax, table_len)
    pick = torch.randperm(ROPE_SLOTS * limit, generator=g)[:ROPE_T]
    slot, pos = (pick // limit).int(), (pick % limit).int()
    slot[3], slot[10] = -1, ROPE_SLOTS
    pos[17], pos[25], pos[31] = -1, smax, table_len
    live = torch.ones(ROPE_T, dtype=torch.bool)
    live[list(ROPE_SKIPPED)] = False
    qkv = torch.full((ROPE_T, heads * d + ROPE_PAD), float("nan"),
                     dtype=torch.bfloat16)
    qkv[:, :heads * d] = torch.randn(ROPE_T, heads * d, generator=g).to(
        torch.bfloat16)
    table = ops.build_rope_cos_sin(table_len, d)
    ref = rope_reference(f64(qkv[live])[None], pos[live], table, ROPE_HQ,
                         ROPE_HKV, d)
    return dict(d=d, smax=smax, qkv=qkv, slot=slot, pos=pos, live=live,
                table=table, ref=ref,
                kc=sentinel_bf16(ROPE_SLOTS, ROPE_HKV, smax, d),
                vc=sentinel_bf16(ROPE_SLOTS, ROPE_HKV, smax, d).flip(0))


def check_rope_varlen(case, qkv, kc, vc, what, kernel):
    """qkv, kc, vc (CPU tensors) after the op ran on copies of the
    case's: roped q and k and the K rows inside the bound, V rows bit
    copies, a skipped token's row and every unwritten cache element
    bit-unchanged."""
    d, live, ref = case["d"], case["live"], case["ref"]
    hq, hkv = ROPE_HQ, ROPE_HKV
    n = int(live.sum())
    slot, pos = case["slot"][live].long(), case["pos"][live].long()
    got = qkv[live]
    check(got[:, :hq * d].view(n, hq, d), ref["q"]["ref"],
          ref["q"]["bound"], what + " q", kernel)
    check(got[:, hq * d:(hq + hkv) * d].view(n, hkv, d), ref["k"]["ref"],
          ref["k"]["bound"], what + " k in qkv", kernel)
    check(kc[slot, :, pos], ref["k"]["ref"], ref["k"]["bound"],
          what + " K rows", kernel)
    v0 = case["qkv"][live][:, (hq + hkv) * d:(hq + 2 * hkv) * d]
    assert same_bits(vc[slot, :, pos].reshape(n, -1), v0), what + " V rows"
    assert same_bits(kc[slot, :, pos][..., :d].reshape(n, -1),
                     got[:, hq * d:(hq + hkv) * d]), what + " K row != k"
    assert same_bits(got[:, (hq + hkv) * d:], case["qkv"][live][
        :, (hq + hkv) * d:]), what + ": v or surplus columns changed"
    assert same_bits(qkv[~live], case["qkv"][~live]), \
        what + ": a skipped token's row changed"
    kc, vc = kc.clone(), vc.clone()
    kc[slot, :, pos] = case["kc"][slot, :, pos]
    vc[slot, :, pos] = case["vc"][slot, :, pos]
    assert same_bits(kc, case["kc"]) and same_bits(vc, case["vc"]), \
        what + ": an unwritten cache element changed"
