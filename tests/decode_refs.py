# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""float64 references, error bounds and input cases of the decode-step
kernels, shared by test_decode_kernels.py (CPU) and
test_decode_kernels_gpu.py.  Everything here runs on the CPU.

Every reference is the plain formula in float64 on exactly the bf16 / f32
/ fp8 values the kernel reads.  An output the kernel writes as bf16 is
held to ``|got - ref| <= r * |ref| + a`` elementwise:

* ``r`` is R1 = 2^-8, the worst relative half-ulp of one bf16 rounding,
  or R2 = 3 * 2^-9 for the norm kernels, which round the new residual to
  bf16 and normalize that rounded value;
* ``a`` is what fp32 arithmetic can add before the rounding: the
  standard ``n * 2^-24 * sum|terms|`` of an n-term fp32 sum, propagated
  through the formula, plus one 2^-24 per further fp32 operation.  It is
  computed from the inputs, and enters as ``a * (1 + r)`` because the
  rounding acts on the fp32 value, not on the reference.

The norm kernels round ``z = sum + residual`` to bf16 and read it back.
Where the float64 z lies within the fp32 error of a bf16 rounding
boundary, fp32 may round it the other way, a whole bf16 ulp from the
reference.  When a case is built, such elements (a few per thousand) get
small dyadic terms instead, whose sum is exact in fp32 and a bf16 value
(the lines marked settle_ties), so that one answer is right."""

import math

import torch

EPS32 = 2.0 ** -24          # unit roundoff of fp32
R1 = 2.0 ** -8              # one bf16 rounding
R2 = 3 * 2.0 ** -9          # norm kernels: rounded residual, rounded out
ATTN_ABS = 1e-4             # fp32 softmax at S <= 130, N(0,1) inputs
FP8_MAX = 448.0
NORM_EPS = 1e-5


def f64(t):
    return t.detach().cpu().to(torch.float64)


def bf16_round(x):
    """float64 -> nearest bf16, as float64 (through fp32, which is exact
    away from the rounding boundaries the cases keep clear of)."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def worst(got, ref, bound):
    """max of error / bound; inf where the error is NaN or the bound is
    zero and the error is not."""
    err = (f64(got) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, math.inf),
                        ratio)
    return ratio.max().item() if ratio.numel() else 0.0


MEASURED = {}


def check(got, ref, bound, what, kernel=None):
    """Print error / bound, remember the maximum per kernel, assert."""
    ratio = worst(got, ref, bound)
    if kernel:
        MEASURED[kernel] = max(MEASURED.get(kernel, 0.0), ratio)
    print(f"err/bound {ratio:.3f}  {what}")
    assert ratio <= 1.0, f"{what}: error is {ratio:.3f} of the bound"
    return ratio


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---------------------------------------------------------------- norms

def norm_reference(parts, residual, weight, eps=NORM_EPS, skip=None):
    """parts [n, rows, hidden] f64 are summed with the residual (or
    without one: residual None).  Returns the new residual z, the
    normalized output and their bounds.  skip: a part to leave out (the
    mutation)."""
    if skip is not None:
        parts = torch.cat([parts[:skip], parts[skip + 1:]])
    terms = parts if residual is None else \
        torch.cat([parts, residual[None]])
    n = terms.shape[0]
    z = terms.sum(0)
    a_z = n * EPS32 * terms.abs().sum(0) if n > 1 else torch.zeros_like(z)
    hidden = z.shape[-1]
    inv = 1.0 / torch.sqrt((z * z).mean(-1, keepdim=True) + eps)
    zr = bf16_round(z) if n > 1 else z
    out = zr * inv * weight
    # sumsq: hidden positive fp32 terms, halved by the square root; then
    # rsqrt, the division by hidden, eps, two products
    a_out = (hidden / 2 + 8) * EPS32 * out.abs()
    return dict(z=z, a_z=a_z, z_bound=R1 * z.abs() + a_z * (1 + R1),
                out=out, out_bound=R2 * out.abs() + a_out * (1 + R2))


def tie_risk(z, a_z):
    """Elements whose bf16 rounding fp32 arithmetic could flip."""
    guard = 4 * a_z + 4 * EPS32 * z.abs()
    return bf16_round(z + guard) != bf16_round(z - guard)


def norm_slab_case(hidden, ksplit, seed, rows=3):
    """Random f32 slabs [ksplit, rows, hidden], bf16 residual and
    weight for fused_add_rmsnorm_slab."""
    g = torch.Generator().manual_seed(seed)
    slabs = torch.randn(ksplit, rows, hidden, generator=g)
    residual = torch.randn(rows, hidden, generator=g).to(torch.bfloat16)
    weight = (1 + 0.1 * torch.randn(hidden, generator=g)).to(
        torch.bfloat16)
    ref = norm_reference(f64(slabs), f64(residual), f64(weight))
    risk = tie_risk(ref["z"], ref["a_z"])           # settle_ties
    for s in range(ksplit):     # an exact sum that is a bf16 value
        slabs[s][risk] = 0.125 * (s + 1)
    residual[risk] = 0.5
    ref = norm_reference(f64(slabs), f64(residual), f64(weight))
    assert not tie_risk(ref["z"], ref["a_z"]).any()
    return slabs, residual, weight


def norm_case(hidden, seed, rows=3, with_residual=True, zero_row=1):
    """bf16 x, residual and weight for fused_add_rmsnorm; row
    `zero_row` is all zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, hidden, generator=g).to(torch.bfloat16)
    residual = torch.randn(rows, hidden, generator=g).to(torch.bfloat16)
    weight = (1 + 0.1 * torch.randn(hidden, generator=g)).to(
        torch.bfloat16)
    x[zero_row] = 0
    residual[zero_row] = 0
    if not with_residual:
        return x, None, weight
    ref = norm_reference(f64(x)[None], f64(residual), f64(weight))
    risk = tie_risk(ref["z"], ref["a_z"])       # settle_ties
    x[risk] = 0.5
    residual[risk] = 0.25
    return x, residual, weight


# --------------------------------------------------------------- swiglu

def swiglu_reference(parts, swap=False, skip=None):
    """parts [n, rows, 2 * inter] f64: out = silu(sum gate) * sum up."""
    if skip is not None:
        parts = torch.cat([parts[:skip], parts[skip + 1:]])
    n, _, two_i = parts.shape
    inter = two_i // 2
    gate, up = parts[..., :inter], parts[..., inter:]
    if swap:
        gate, up = up, gate
    g, u = gate.sum(0), up.sum(0)
    acc = n * EPS32 if n > 1 else 0.0
    a_g, a_u = acc * gate.abs().sum(0), acc * up.abs().sum(0)
    silu = g / (1 + torch.exp(-g))
    out = silu * u
    # |silu'| <= 1.1; then per element: g * log2(e) (|g| roundoffs of
    # the exponential), the exponential, 1 + e, the division and the
    # product with u, at up to two roundoffs each
    a = 1.1 * u.abs() * a_g + silu.abs() * a_u + \
        (g.abs() + 8) * EPS32 * out.abs()
    return dict(out=out, bound=R1 * out.abs() + a * (1 + R1))


def swiglu_case(rows, inter, ksplit, seed):
    """f32 slabs [ksplit, rows, 2 * inter]; the summed gate spans
    [-12, 12] including both ends."""
    g = torch.Generator().manual_seed(seed)
    slabs = torch.randn(ksplit, rows, 2 * inter, generator=g)
    want = torch.rand(rows, inter, generator=g) * 24 - 12
    want.view(-1)[0], want.view(-1)[-1] = -12.0, 12.0
    slabs[-1, :, :inter] = want - slabs[:-1, :, :inter].sum(0)
    return slabs


# ----------------------------------------------------------------- rope

def rope_reference(parts, positions, cos_sin, hq, hkv, d, sign=1.0,
                   skip=None):
    """parts [n, B, qkv_row] f64 -> rotated q [B, hq, d], rotated k and
    plain v [B, hkv, d], each with its bound."""
    if skip is not None:
        parts = torch.cat([parts[:skip], parts[skip + 1:]])
    n, B, _ = parts.shape
    heads = hq + 2 * hkv
    half = d // 2
    terms = parts[:, :, :heads * d].reshape(n, B, heads, d)
    x = terms.sum(0)
    a_x = (n * EPS32 if n > 1 else 0.0) * terms.abs().sum(0)
    table = f64(cos_sin)[positions.long()]              # [B, half, 2]
    c, s = table[:, None, :, 0], sign * table[:, None, :, 1]
    lo, hi = x[..., :half], x[..., half:]
    a_lo, a_hi = a_x[..., :half], a_x[..., half:]
    rot = torch.cat([lo * c - hi * s, hi * c + lo * s], -1)
    # two products and a sum (or a product and an fma) in fp32
    a_rot = torch.cat([
        c.abs() * a_lo + s.abs() * a_hi +
        3 * EPS32 * ((lo * c).abs() + (hi * s).abs()),
        c.abs() * a_hi + s.abs() * a_lo +
        3 * EPS32 * ((hi * c).abs() + (lo * s).abs())], -1)

    def pack(ref, a):
        return dict(ref=ref, bound=R1 * ref.abs() + a * (1 + R1))

    return dict(q=pack(rot[:, :hq], a_rot[:, :hq]),
                k=pack(rot[:, hq:hq + hkv], a_rot[:, hq:hq + hkv]),
                v=pack(x[:, hq + hkv:], a_x[:, hq + hkv:]))


def rope_case(B, hq, hkv, d, ksplit, pad, seed):
    g = torch.Generator().manual_seed(seed)
    qkv_row = (hq + 2 * hkv) * d + pad
    return torch.randn(ksplit, B, qkv_row, generator=g)


def sentinel_bf16(*shape):
    """A bf16 tensor of distinct finite bit patterns."""
    n = math.prod(shape)
    bits = (torch.arange(n, dtype=torch.int32) % 30011 + 1).to(torch.int16)
    return bits.view(torch.bfloat16).view(*shape).clone()


# ------------------------------------------------------------ attention

D = 128
HKV = 2
SMAX = 129
ATTN_LENS = ((1, 32, 33), (64, 65, 97), (0, 31, SMAX))
RAMP_LENS = (128, 96, 64)     # no chunk of 32 or 64 ends in a short tail
GROUPS = (1, 2, 4, 8)
NSPLITS = (1, 2, 3, 4, 16)
ATTN_SCALE = 1.0 / math.sqrt(D)


def e4m3_decode(u8):
    return u8.contiguous().view(torch.float8_e4m3fn).to(torch.float64)


def attn_reference(q, keys, vals, lens, scale=ATTN_SCALE, drop=None):
    """q [B, Hq, D], keys / vals [B, Hkv, S, D] f64; rows >= len are
    never touched.  A sequence of length 0 gives zeros.  drop: (b, row)
    leaves one KV row of one sequence out."""
    B, Hq, _ = q.shape
    G = Hq // keys.shape[1]
    out = torch.zeros_like(q)
    for b in range(B):
        rows = list(range(int(lens[b])))
        if drop is not None and drop[0] == b:
            rows.remove(drop[1])
        if not rows:
            continue
        for h in range(Hq):
            k, v = keys[b, h // G, rows], vals[b, h // G, rows]
            p = torch.softmax(k @ q[b, h] * scale, 0)
            out[b, h] = p @ v
    return out


def attn_bound(ref):
    return R1 * ref.abs() + ATTN_ABS


_ATTN = {}


def attn_case(G, lens, kv="bf16", ramp=0.0):
    """One decode-attention case, built once.  q, K and V are N(0,1);
    with `ramp`, q gains 0.5 in every dim and key row i gains ramp * i
    (or ramp * (len-1-i) when ramp < 0), so that scores rise (fall) by
    about 5.7 * |ramp| per row.  kv="fp8" quantizes K and V per row.
    Rows >= len hold NaN (fp8: code 0x7F and a NaN scale).  `keys` and
    `vals` are the float64 values the kernel reads."""
    key = (G, tuple(lens), kv, ramp)
    if key in _ATTN:
        return _ATTN[key]
    from mlrun_amd import ops

    B, Hq = len(lens), HKV * G
    g = torch.Generator().manual_seed(
        1000 * G + sum(lens) + (7 if kv == "fp8" else 0) + int(ramp * 1e4))
    q = torch.randn(B, Hq, D, generator=g)
    k = torch.randn(B, HKV, SMAX, D, generator=g)
    v = torch.randn(B, HKV, SMAX, D, generator=g)
    if ramp:
        q += 0.5
        for b, length in enumerate(lens):
            pos = torch.arange(SMAX, dtype=torch.float32)
            step = pos if ramp > 0 else (length - 1 - pos)
            k[b] += (abs(ramp) * step).view(1, SMAX, 1)
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    case = dict(G=G, lens=tuple(lens), kv=kv, q=q,
                seq_lens=torch.tensor(lens, dtype=torch.int32))
    dead = torch.zeros(B, SMAX, dtype=torch.bool)
    for b, length in enumerate(lens):
        dead[b, length:] = True
    dead = dead[:, None, :].expand(B, HKV, SMAX)
    if kv == "fp8":
        k8, ks = ops.quantize_kv_rows(k)
        v8, vs = ops.quantize_kv_rows(v)
        exact_k = e4m3_decode(k8) * f64(ks)[..., None]
        exact_v = e4m3_decode(v8) * f64(vs)[..., None]
        # the kernel stages the dequantized rows as bf16
        case.update(keys=bf16_round(exact_k), vals=bf16_round(exact_v),
                    keys_exact=exact_k, vals_exact=exact_v)
        for codes, scales in ((k8, ks), (v8, vs)):
            codes[dead] = 0x7F
            scales[dead] = float("nan")
        case.update(kc=k8.contiguous(), vc=v8.contiguous(),
                    k_scale=ks.contiguous(), v_scale=vs.contiguous())
    else:
        case.update(keys=f64(k), vals=f64(v))
        k[dead] = float("nan")
        v[dead] = float("nan")
        case.update(kc=k, vc=v, k_scale=None, v_scale=None)
    case["ref"] = attn_reference(f64(q), case["keys"], case["vals"], lens)
    case["bound"] = attn_bound(case["ref"])
    _ATTN[key] = case
    return case


def chunk_maxima(case, b, h, chunk):
    """Per-chunk maximum score of one (sequence, head)."""
    length = case["lens"][b]
    s = case["keys"][b, h // case["G"], :length] @ f64(case["q"])[b, h]
    return [s[i:i + chunk].max().item() for i in range(0, length, chunk)]


# ------------------------------------------------------------------ fp8

def ulp32(x):
    """fp32 ulp at |x| (float64 tensor)."""
    return torch.exp2(torch.floor(torch.log2(x.abs())) - 23)


def fp8_code_ratio(codes, scale, x):
    """Dequantized unswizzled codes [rows, cols] against the values x
    they encode: error over the e4m3 half step, 2^-4 |x| for normals
    plus scale * 2^-10 for the subnormal range."""
    scale = f64(scale)[:, None]
    x = f64(x)
    return worst(e4m3_decode(codes) * scale, x,
                 2.0 ** -4 * x.abs() + scale * 2.0 ** -10)


def quant_case(cols, seed, rows=3, zero_row=1):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(rows, cols, generator=g) * 3).to(torch.bfloat16)
    a[zero_row] = 0
    return a


def check_quant(codes, scale, a, what, kernel=None):
    """quant_fp8_rows: scale = amax / 448 within 2 fp32 ulps; an
    all-zero row has zero codes and any finite positive scale; the
    codes are the e4m3 rounding of a / scale in the pair-swizzled
    layout."""
    from mlrun_amd import ops

    amax = f64(a).abs().amax(-1)
    live = amax > 0
    want = amax[live] / FP8_MAX
    got = f64(scale)
    off = ((got[live] - want).abs() / ulp32(want)).max().item()
    print(f"scale off by {off:.2f} ulp  {what}")
    assert off <= 2.0, f"{what}: scale off by {off} ulp"
    assert torch.isfinite(got).all() and (got > 0).all(), what
    plain = ops._fp8_pair_unswizzle(codes.cpu())
    assert (plain[~live] == 0).all(), f"{what}: zero row has nonzero codes"
    ratio = fp8_code_ratio(plain, scale, a)
    if kernel:
        MEASURED[kernel] = max(MEASURED.get(kernel, 0.0), ratio)
    print(f"err/half-step {ratio:.3f}  {what}")
    assert ratio <= 1.0, f"{what}: code error {ratio:.3f} of the half step"


GEMM_N = 80
GEMM_MS = (1, 16, 17, 32, 33, 64)
GEMM_KS = (64, 192, 1088)
GEMM_KSPLITS = (1, 2, 5)

_GEMM = {}


def gemm_fp8_case(m, k, n=GEMM_N):
    """Random e4m3 codes (no NaN codes) and scales, built once."""
    if (m, k, n) in _GEMM:
        return _GEMM[(m, k, n)]
    g = torch.Generator().manual_seed(10 * k + m)

    def codes(rows):
        c = torch.randint(0, 256, (rows, k), generator=g, dtype=torch.int32)
        c[(c & 0x7F) == 0x7F] = 0x38            # NaN codes -> 1.0
        return c.to(torch.uint8)

    a8, w8 = codes(m), codes(n)
    # neighbouring rows' scales differ by 1.7 x at least, so that a
    # scale taken from the wrong row shows
    step = 1.25 ** ((3 * torch.arange(m)) % 17).float()
    a_scale = 0.002 * step * (1 + 0.05 * torch.rand(m, generator=g))
    w_scale = torch.rand(n, generator=g) * 0.003 + 0.0002
    _GEMM[(m, k, n)] = (a8, a_scale, w8, w_scale)
    return _GEMM[(m, k, n)]


# v_mfma_f32_16x16x32_fp8_fp8 does not add its 32 products in fp32.  The
# f32 slabs of the split-K kernel, summed in float64, are off the float64
# product by up to 3581 * 2^-24 = 2^-12.2 of sum|terms| (M 64, K 64, two
# chained instructions in one wave), where fp32 accumulation predicts at
# most (K + 2) * 2^-24 = 2^-17.9; the error follows the largest product
# of an instruction, not sum|terms|: quantized N(0,1) operands at K 1088
# are off 48 * 2^-24 of sum|terms| but 6380 * 2^-24 of the largest term,
# random codes 601 and 9018, and the figures are the same for ksplit 1, 2
# and 5.  The instruction's own error therefore enters the bound as a
# term of its own: the measured maximum with a margin of 2.3.
MFMA_FP8_ACC = 2.0 ** -11


def gemm_fp8_reference(a8, a_scale, w8, w_scale, ksplit, shift_scale=False,
                       mfma=True):
    """The float64 product of the dequantized operands.  fp8 products
    are exact in fp32: K of them are accumulated, ksplit slabs are
    added, and two scales multiplied in.  mfma: allow for the fp8 MFMA's
    accumulation (the CPU branch runs without)."""
    from mlrun_amd import ops

    sa = f64(a_scale)
    if shift_scale:                 # the mutation: a_scale[m] from m + 1
        sa = torch.roll(sa, -1)
    a = e4m3_decode(ops._fp8_pair_unswizzle(a8)) * sa[:, None]
    w = e4m3_decode(ops._fp8_pair_unswizzle(w8)) * f64(w_scale)[:, None]
    ref = a @ w.t()
    k = a.shape[1]
    a_acc = ((k + ksplit + 2) * EPS32 + (MFMA_FP8_ACC if mfma else 0.0)) * \
        (a.abs() @ w.abs().t())
    return ref, R1 * ref.abs() + a_acc * (1 + R1)
