"""CPU references of the forward GEMM's epilogues (csrc/gemm.hip: vp_gemm_bf16, vp_gemm_bf16_ws, vp_gemm_mx_fp8) and of
vp_head_norm_rope_bf16, written from the chains documented in include/vp_hip.h, plus the case lists that
tests/test_gemm_refs_cpu.py and tests/test_gemm_epilogues_gpu.py share.  Nothing here imports the package under test.

Exact operands.  `exact_operands` draws A and W as integers in [-3, 3] times one power of two per tensor and a bias
that is a bf16 multiple of the product scale, so every product and every partial sum of the accumulator is exactly
representable in fp32 whatever the main loop, the K split or the summation order: acc + bias is known exactly,
y = rnd(acc + bias) is known bit for bit, and so is every epilogue that the header states as single fp32 operations
each followed by a rounding to bf16 (BIAS, BIAS_SCALE, GATED, BIAS_ADDROWS, the aux outputs).  `epilogue_ref`
evaluates those chains in float32 torch: the product of two bf16 values is exact in fp32 and one fp32 addition is
correctly rounded on both sides, so the result is the expected bits.  GELU, GELU_BWD and QKNORM_ROPE are compared per
element with the float64 references on the exactly known y.

`expected` builds, for one case, the whole expected output buffer (sentinel rows past the last output row, sentinel
columns in [N, ldc), rows that the row remap leaves alone) and `check_output` is the one gate both test files use:
bit equality wherever `allowed` is absent, |got - ref| <= allowed elsewhere.  `expected(..., mutant=name)` evaluates a
deliberately wrong epilogue (MUTANTS); tests/test_gemm_refs_cpu.py asserts that the gate rejects every one of them on
every case list it can affect."""
import functools
import math
from types import SimpleNamespace

import torch

from tests.backward_refs import (C_F32_HEAD, F64, _ln_stats, bf16_ulps, gelu_bwd_ref, gelu_ref, rnd_bf16,  # noqa: F401
                                 row_kind, wide, worst_ratio)

BF = torch.bfloat16
F32 = torch.float32
U8 = 2.0 ** -8    # the largest relative error of one rounding to bf16
SENT = 7.0        # what every output buffer holds before the launch
GUARD = 4         # sentinel rows after the last output row

BIAS, GELU, SCALE, GATED, ADDROWS, GELU_MX, QKNORM, GELU_BWD = 0, 1, 2, 3, 4, 5, 6, 7  # include/vp_hip.h VP_EPI_*
EPI_NAMES = {BIAS: "bias", GELU: "gelu", SCALE: "scale", GATED: "gated", ADDROWS: "addrows", GELU_MX: "gelu_mx",
             QKNORM: "qknorm", GELU_BWD: "gelu_bwd"}

# c_f32 of the forward head vectors (rnd(LN64) -> RoPE), measured as tests/backward_refs.py describes: the worst
# |fp32 - fp64| / E of head_norm_rope_ref in float32 torch on the CPU over every QKNORM case and every head-norm case
# below, times 8, rounded up to two digits.  tests/test_gemm_refs_cpu.py::test_c_f32_head_fwd repeats the measurement
# and fails if 8 x worst leaves [C / 2, C].  backward_refs.C_F32_HEAD (1.4e-06) is reused only if it holds that band.
#   forward head vectors:  worst 1.888e-07  ->  x 8 = 1.511e-06  (outside C_F32_HEAD's band: a constant of its own)
C_F32_HEAD_FWD = 1.6e-06


# ------------------------------------------------------------------------------------------------------------------
# exact operands
# ------------------------------------------------------------------------------------------------------------------

def exact_operands(M, K, n_seg, nsegs, seed, scale_a, scale_w, bias_max=1000, a_tail=None):
    """bf16 a [M, Ka], w[s] [n_seg, K], bias[s] [n_seg]: integers in [-3, 3] times scale_a / scale_w (powers of two),
    w[:, 0] asymmetric across the output columns ((n % 7) - 3), the bias a bf16-representable integer in
    [-bias_max, bias_max] times scale_a scale_w.  a_tail = (k0, r) (K = k0 + r): Ka = k0 + nsegs r and segment s
    reads the columns [0, k0) and [k0 + s r, k0 + (s + 1) r) of a (vp_gemm_desc.a_tail_k / a_tail_off).
    Asserts the exactness precondition: K 9 + |bias| < 2^24 in unscaled units, and the float32, float64 and int64
    matmuls of the unscaled integers agree exactly (on the first and last 32 rows when M N K > 2^29).
    Returns a namespace with a, w, bias, acc (fp32 [M, N] = the exact accumulator), acc_drop8 (the last 8 K columns
    left out), bias_row (fp32 [N]) and scale = scale_a scale_w."""
    for s in (scale_a, scale_w):
        assert s > 0 and math.frexp(s)[0] == 0.5, "scales are powers of two"
    g = torch.Generator().manual_seed(seed)
    Ka = K if a_tail is None else a_tail[0] + nsegs * a_tail[1]
    assert a_tail is None or K == a_tail[0] + a_tail[1]
    ai = torch.randint(-3, 4, (M, Ka), generator=g)
    wi = torch.randint(-3, 4, (nsegs, n_seg, K), generator=g)
    wi[:, :, 0] = ((torch.arange(nsegs * n_seg) % 7) - 3).view(nsegs, n_seg)
    bi = rnd_bf16(torch.randint(-bias_max, bias_max + 1, (nsegs, n_seg), generator=g).float()).long()
    assert K * 9 + int(bi.abs().max()) < 2 ** 24
    N = n_seg * nsegs
    acc = torch.empty(M, N, dtype=F32)
    drop = torch.empty(M, N, dtype=F32)
    rows = torch.arange(M) if M * N * K <= 2 ** 29 else torch.cat([torch.arange(32), torch.arange(M - 32, M)])
    for s in range(nsegs):
        if a_tail is None:
            ms = ai
        else:
            k0, r = a_tail
            ms = torch.cat([ai[:, :k0], ai[:, k0 + s * r:k0 + (s + 1) * r]], 1)
        sl = slice(s * n_seg, (s + 1) * n_seg)
        acc[:, sl] = ms.float() @ wi[s].float().T
        drop[:, sl] = ms[:, :K - 8].float() @ wi[s][:, :K - 8].float().T
        i64 = ms[rows] @ wi[s].T
        assert torch.equal(acc[rows, sl].long(), i64) and torch.equal(acc[rows, sl].double(), acc[rows, sl].long().double())
        assert torch.equal((ms[rows].double() @ wi[s].double().T).long(), i64)
    sc = scale_a * scale_w
    return SimpleNamespace(a=(ai.float() * scale_a).to(BF), w=[(wi[s].float() * scale_w).to(BF) for s in range(nsegs)],
                           bias=[(bi[s].float() * sc).to(BF) for s in range(nsegs)], acc=acc * sc, acc_drop8=drop * sc,
                           bias_row=bi.reshape(-1).float() * sc, scale=sc, scale_a=scale_a, Ka=Ka)


@functools.lru_cache(maxsize=None)
def _operands(M, K, n_seg, nsegs, seed, small, a_tail):
    # "big": y = rnd(acc + bias) in the hundreds (up to ~1500: more than 8 significant bits, so the rounding is
    # exercised); "small": |y| up to about 8 (the GELU's and the LayerNorm's working range)
    sa, sw = (2.0 ** -4, 2.0 ** -3) if small else (2.0 ** -2, 2.0 ** 2)
    return exact_operands(M, K, n_seg, nsegs, seed, sa, sw, a_tail=a_tail)


# ------------------------------------------------------------------------------------------------------------------
# the documented chains
# ------------------------------------------------------------------------------------------------------------------

def f32(t):
    return t.detach().cpu().to(F32)


def epilogue_ref(kind, y, *, alpha=1.0, gate_rows=None, R_rows=None, inject_rows=None, inject_on=None,
                 addrows_rows=None, z=None, inner_rnd=True):
    """The chain of include/vp_hip.h after y = rnd(acc + bias) (fp32 [M, N] of bf16 values), one IEEE fp32 operation
    per step, rounded to bf16 wherever the header says rnd.  The row-wise operands come gathered per GEMM row:
    gate_rows / R_rows / inject_rows / addrows_rows [M, N], inject_on bool [M].  BIAS, SCALE, GATED, ADDROWS: the
    expected bits (fp32 of bf16 values).  GELU / GELU_BWD: the float64 value, unrounded.  inner_rnd=False is the
    mutant that drops the gated chain's rnd(gate * y)."""
    if kind == BIAS:
        return y
    if kind == SCALE:
        return rnd_bf16(y * torch.tensor(alpha, dtype=F32))
    if kind == GATED:
        t = f32(gate_rows) * y  # exact: two bf16 factors
        if inner_rnd:
            t = rnd_bf16(t)
        c = rnd_bf16(f32(R_rows) + t)
        if inject_rows is not None:
            c = torch.where(inject_on[:, None], rnd_bf16(c + f32(inject_rows)), c)
        return c
    if kind == ADDROWS:
        return rnd_bf16(y + f32(addrows_rows))
    if kind == GELU:
        return gelu_ref(y)
    if kind == GELU_BWD:
        return gelu_bwd_ref(y, z)
    raise ValueError(kind)


def _pairs(t):
    return t[..., 0::2], t[..., 1::2]


def _inter(a, b):
    return torch.stack((a, b), -1).flatten(-2)


def head_norm_rope_ref(x, lw, lb, eps, H, T, rope=None, mask=None, pre_scale=1.0, dt=F64, rot_from=None):
    """vp_head_norm_rope_bf16 and the q / k heads of VP_EPI_BIAS_QKNORM_ROPE: x [B, N, H 64] ->
    rnd(RoPE(rnd(LN64(x; lw, lb, eps)))) with the interleaved-pair RoPE (y0 = n0 c0 - n1 s0, y1 = n1 c1 + n0 s1, table
    row token - T) on the rows >= T; optional pre-mask x <- rnd(rnd(x mask[b, n]) pre_scale).
    Returns y UNROUNDED with both roundings of the chain left out (as adaln_modulate_ref / final_norm_ref do with
    theirs), `mag` = one term per omitted rounding (text rows: rnd(rnd(n)) = rnd(n), |n|; video rows: the rounding of
    n seen through the rotation, |n0 c0| + |n1 s0|, plus |y|) and the fp32 magnitude scale E (the same formula with
    the absolute values of its terms).  rot_from: the first rotated row if not T (a mutant; table row max(n - T, 0))."""
    B, N, _ = x.shape
    xw = wide(x, dt)
    if mask is not None:
        xw = rnd_bf16(rnd_bf16(xw * wide(mask, dt)[..., None]) * pre_scale)
    xw = xw.reshape(B, N, H, 64)
    w, b = wide(lw, dt), wide(lb, dt)
    _, xhat, e_xhat = _ln_stats(xw, eps)
    n = xhat * w + b
    E = e_xhat * w.abs() + b.abs()
    y, mag = n.clone(), n.abs()
    lo = T if rot_from is None else rot_from
    if rope is not None and lo < N:
        idx = (torch.arange(lo, N) - T).clamp(min=0)
        cos, sin = (wide(t, dt)[idx][:, None, :] for t in rope)  # [rows, 1, 64]: broadcast over heads
        (n0, n1), (e0, e1) = _pairs(n[:, lo:]), _pairs(E[:, lo:])
        (c0, c1), (s0, s1) = _pairs(cos), _pairs(sin)
        yv = _inter(n0 * c0 - n1 * s0, n1 * c1 + n0 * s1)
        y[:, lo:] = yv
        mag[:, lo:] = _inter((n0 * c0).abs() + (n1 * s0).abs(), (n1 * c1).abs() + (n0 * s1).abs()) + yv.abs()
        E[:, lo:] = _inter(e0 * c0.abs() + e1 * s0.abs(), e1 * c1.abs() + e0 * s1.abs())
    return dict(y=y.reshape(B, N, H * 64), mag=mag.reshape(B, N, H * 64), E=E.reshape(B, N, H * 64))


def head_allowed(r):
    return C_F32_HEAD_FWD * r["E"] + U8 * r["mag"]


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------

_DEFAULTS = dict(api="bf16", nsegs=1, lda_pad=0, ldc_pad=0, rpg=None, gs=0, ro=0, alpha=0.37, tpb=1, T=0,
                 inject=None, inject_pad=0, alias_R=False, addrows_offset=0, addrows_pad=0, aux=False, a_tail=None,
                 ws="none", H=0, rope=None, grid=None, seed=0)
INJECT_MODES = (None, "nomask", "zeros", "ones", "random", "first", "last")


def case(name, epi, M, K, n_seg, **kw):
    """One GEMM launch.  ws: "none" / "split" / "tail" = what vp_gemm_bf16_workspace_bytes must say.  inject: one of
    INJECT_MODES (the mask: none, all 0 = every video row injected, all 1, random, or one clear byte at the first /
    last video row of each batch).  rope: None / "full" / "sep" (a separable table on `grid`)."""
    bad = set(kw) - set(_DEFAULTS)
    assert not bad, bad
    c = SimpleNamespace(**{**_DEFAULTS, **kw}, name=name, epi=epi, M=M, K=K, n_seg=n_seg)
    c.N = n_seg * c.nsegs
    c.small = epi in (GELU, GELU_BWD, QKNORM, GELU_MX)
    c.rpg = c.rpg or M
    c.lda = (K if c.a_tail is None else c.a_tail[0] + c.nsegs * c.a_tail[1]) + c.lda_pad
    c.ldc = c.N + c.ldc_pad
    m = torch.arange(M)
    c.gin = m % c.rpg
    c.orow = (m // c.rpg) * c.gs + c.ro + c.gin
    c.out_rows = int(c.orow.max()) + 1
    c.remap = bool((c.orow != m).any())
    c.B = (M + c.tpb - 1) // c.tpb
    c.Nv = c.tpb - c.T
    assert c.inject in INJECT_MODES and (c.inject is None or epi == GATED)
    return c


def _randbf(g, *shape, std=1.0):
    return (torch.randn(*shape, generator=g) * std).to(BF)


def inputs(c):
    """Every tensor of the launch on the CPU (bf16 unless stated), from c.seed.  Row-wise operands carry full random
    mantissas; stride gaps hold values of their own (a wrong stride reads them)."""
    o = _operands(c.M, c.K, c.n_seg, c.nsegs, 100 + c.seed, c.small, c.a_tail)
    g = torch.Generator().manual_seed(9000 + c.seed)
    t = SimpleNamespace(ops=o)
    a = torch.full((c.M, c.lda), float("nan"), dtype=BF)  # A's padding columns [Ka, lda) hold NaN
    a[:, :o.Ka] = o.a
    t.a = a
    N = c.N
    if c.epi == GATED:
        t.mod = _randbf(g, c.B, 6 * N + 8)                # gate = chunk 2, gate_text = chunk 5, batch stride 6 N + 8
        t.R = _randbf(g, c.out_rows, c.ldc if c.alias_R else N + 8, std=300.0)
        if c.inject is not None:
            nv = max(c.Nv, 1)
            t.inject = _randbf(g, c.B, nv, N + c.inject_pad, std=100.0)
            mask = {"nomask": None, "zeros": torch.zeros(c.B, nv), "ones": torch.ones(c.B, nv),
                    "random": (torch.rand(c.B, nv, generator=g) > 0.5).float(), "first": torch.ones(c.B, nv),
                    "last": torch.ones(c.B, nv)}[c.inject]
            if c.inject == "first":
                mask[:, 0] = 0
            if c.inject == "last":
                mask[:, -1] = 0
            t.inject_mask = None if mask is None else mask.to(torch.uint8)
    if c.epi == ADDROWS:
        t.addrows = _randbf(g, c.rpg + c.addrows_offset + 1, N + c.addrows_pad, std=300.0)
    if c.epi == GELU_BWD:
        t.z = _randbf(g, c.M, N, std=2.0)
    if c.epi == QKNORM:
        t.lnw = [(1 + 0.2 * torch.randn(64, generator=g)).to(BF) for _ in range(2)]
        t.lnb = [(0.1 * torch.randn(64, generator=g)).to(BF) for _ in range(2)]
        # k's eps far from q's, so that the wrong one is a visible error (a head vector's variance is about 20)
        t.eps = (1e-6, 4.0)
        t.rope = None
        if c.rope == "full":  # random rows: every table row, row 0 included, is a rotation of its own
            t.rope = (torch.randn(c.Nv, 64, generator=g), torch.randn(c.Nv, 64, generator=g))
        elif c.rope == "sep":  # per-axis factors (dims 0-15 by frame, 16-39 by row, 40-63 by column), random
            F_, Hh, Ww = c.grid
            assert F_ * Hh * Ww == c.Nv
            tabs = []
            for _ in range(2):
                ax = [torch.randn(F_, 16, generator=g), torch.randn(Hh, 24, generator=g),
                      torch.randn(Ww, 24, generator=g)]
                full = torch.cat([ax[0][:, None, None].expand(F_, Hh, Ww, 16), ax[1][None, :, None].expand(F_, Hh, Ww, 24),
                                  ax[2][None, None, :].expand(F_, Hh, Ww, 24)], -1)
                tabs.append(full.reshape(c.Nv, 64).contiguous())
            t.rope = tuple(tabs)
    return t


# the shared mistakes (tests/test_gemm_refs_cpu.py: the gate must see each one wherever it can show)
MUTANTS = ("gate_prev_batch", "text_gate_at_T", "video_gate_at_Tm1", "neighbour_bias", "inject_on_masked",
           "inject_vtok_p1", "addrows_offset_p1", "remap_last_row_p1", "drop_inner_rnd", "drop_last_8k",
           "add_a_padding", "rope_last_text_row", "eps_q_for_k")


def mutant_applies(mu, c, t):
    """whether mutant mu changes what case c computes (where it cannot, the case is excluded from it by this rule)"""
    gated = c.epi == GATED
    masked = gated and c.inject is not None and c.Nv > 0
    some_on = masked and (t.inject_mask is None or bool((t.inject_mask == 0).any()))
    some_off = masked and t.inject_mask is not None and bool((t.inject_mask != 0).any())
    return {"gate_prev_batch": gated and c.B >= 2,
            "text_gate_at_T": gated and c.T < c.tpb,
            "video_gate_at_Tm1": gated and c.T >= 1,
            "neighbour_bias": c.nsegs > 1,
            "inject_on_masked": some_off,
            "inject_vtok_p1": some_on and c.Nv > 1,
            "addrows_offset_p1": c.epi == ADDROWS,
            "remap_last_row_p1": c.remap,
            "drop_inner_rnd": gated,
            "drop_last_8k": True,
            "add_a_padding": c.lda_pad > 0,
            "rope_last_text_row": c.epi == QKNORM and c.rope is not None and c.T >= 1 and c.Nv > 0,
            "eps_q_for_k": c.epi == QKNORM}[mu]


def expected(c, t, mutant=None):
    """{"C": expectation, "aux": expectation or None}; an expectation = namespace(buf, ref, allowed): buf = the whole
    bf16 buffer ([out_rows + GUARD, ldc] for C, [M + GUARD, ld_aux] for aux) with the expected bits (rnd(ref) where a
    tolerance applies), ref / allowed float64 of buf's shape or None; allowed == 0 = bit equality."""
    assert mutant is None or (mutant in MUTANTS and mutant_applies(mutant, c, t)), (mutant, c.name)
    o, N, M = t.ops, c.N, c.M
    acc = o.acc_drop8 if mutant == "drop_last_8k" else o.acc
    if mutant == "add_a_padding":
        # the K loop run on to lda over finite garbage: 1 (in a's units) in every padding column against the
        # weight columns [0, lda_pad) again -- a plausible wrong sum, not a NaN
        wpad = torch.cat([w.float()[:, :c.lda_pad] for w in o.w]).sum(1)
        acc = acc + wpad * o.scale_a
    bias = o.bias_row
    if mutant == "neighbour_bias":
        bias = bias.clone()
        for s in range(1, c.nsegs):
            e = s * c.n_seg
            w = min(8, c.n_seg)
            bias[e - w:e] = o.bias_row[e:e + w]      # the last columns of segment s - 1 take segment s's first
            bias[e:e + w] = o.bias_row[e - w:e]      # and the other way round
    y = rnd_bf16(acc + bias)
    m = torch.arange(M)
    b, tok = m // c.tpb, m % c.tpb
    kw = {}
    if c.epi == GATED:
        text = tok < c.T
        gb = b.clone()
        if mutant == "gate_prev_batch":
            gb[(tok == 0) & (b > 0)] -= 1
        if mutant == "text_gate_at_T":
            text = text | (tok == c.T)
        if mutant == "video_gate_at_Tm1":
            text = text & (tok != c.T - 1)
        gv, gt = t.mod[:, 2 * N:3 * N], t.mod[:, 5 * N:6 * N]
        kw["gate_rows"] = torch.where(text[:, None], gt[gb], gv[gb])
        kw["R_rows"] = t.R[c.orow, :N]
        kw["inner_rnd"] = mutant != "drop_inner_rnd"
        if c.inject is not None and c.Nv > 0:
            video = tok >= c.T
            vtok = (tok - c.T).clamp(min=0)
            on = video if t.inject_mask is None or mutant == "inject_on_masked" else \
                video & (t.inject_mask[b, vtok] == 0)
            if mutant == "inject_vtok_p1":
                vtok = (vtok + 1) % c.Nv
            kw["inject_rows"], kw["inject_on"] = t.inject[b, vtok, :N], on
    if c.epi == ADDROWS:
        kw["addrows_rows"] = t.addrows[c.gin + c.addrows_offset + (mutant == "addrows_offset_p1"), :N]
    if c.epi == GELU_BWD:
        kw["z"] = t.z
    ref = allowed = None
    if c.epi in (BIAS, SCALE, GATED, ADDROWS, GELU, GELU_BWD):
        rows = epilogue_ref(c.epi, y, alpha=c.alpha, **kw)
        if c.epi == GELU:
            ref, allowed = rows, U8 * rows.abs() + 2.0 ** -118
        elif c.epi == GELU_BWD:
            ref, allowed = rows, U8 * rows.abs() + 2.0 ** -118 * y.abs().clamp(min=1.0).double()
    elif c.epi == GELU_MX:
        rows = y  # only the aux output (z = rnd(acc + bias)) is compared; C is MX-quantised
    else:
        assert c.epi == QKNORM and c.nsegs == 3 and M == c.B * c.tpb and c.n_seg == c.H * 64
        ref, allowed = y.double().clone(), torch.zeros(M, N, dtype=F64)
        for s in range(2):
            sl = slice(s * c.n_seg, (s + 1) * c.n_seg)
            r = head_norm_rope_ref(y[:, sl].reshape(c.B, c.tpb, c.n_seg), t.lnw[s], t.lnb[s],
                                   t.eps[0 if mutant == "eps_q_for_k" else s], c.H, c.T, t.rope,
                                   rot_from=c.T - 1 if mutant == "rope_last_text_row" else None)
            ref[:, sl] = r["y"].reshape(M, c.n_seg)
            allowed[:, sl] = head_allowed(r).reshape(M, c.n_seg)
        rows = ref
    orow = c.orow + ((c.gin == c.rpg - 1) if mutant == "remap_last_row_p1" else 0)
    buf = torch.full((c.out_rows + GUARD, c.ldc), SENT, dtype=BF)
    if c.alias_R:
        buf[:c.out_rows] = t.R
    ex = SimpleNamespace(buf=buf, ref=None, allowed=None)
    if ref is None:
        buf[orow, :N] = rows.to(BF)
    else:
        buf[orow, :N] = rnd_bf16(rows).to(BF)
        ex.ref = buf.double()
        ex.allowed = torch.zeros_like(ex.ref)
        ex.ref[orow, :N], ex.allowed[orow, :N] = rows.double(), allowed
    out = {"C": ex, "aux": None}
    if c.aux:
        width = 2 * c.n_seg if c.epi == QKNORM else N
        ab = torch.full((M + GUARD, width + 8), SENT, dtype=BF)
        ab[:M, :width] = y[:, :width].to(BF)
        out["aux"] = SimpleNamespace(buf=ab, ref=None, allowed=None)
    return out


def check_output(name, ex, got, quiet=False):
    """The gate of both test files: `got` (the whole bf16 buffer after the launch) against the expectation, every
    element: equal values where no tolerance applies (sentinels included), else |got - ref| <= allowed.  Returns the
    worst error / allowed (0.0: bit-equal) and prints it."""
    got = got.detach().cpu()
    assert got.shape == ex.buf.shape and got.dtype == BF, f"{name}: buffer {tuple(got.shape)} {got.dtype}"
    if ex.ref is None:
        same = got.float() == ex.buf.float()
        if not bool(same.all()):
            bad = (~same).nonzero()
            r, col = (int(v) for v in bad[0])
            d = (got.double() - ex.buf.double()).abs().nan_to_num(nan=float("inf"))
            raise AssertionError(f"{name}: {len(bad)} of {got.numel()} elements differ (largest |got - expected| = "
                                 f"{float(d.max()):g}), first at row {r} column {col}: got {float(got[r, col])}, "
                                 f"expected {float(ex.buf[r, col])}")
        if not quiet:
            print(f"  {name}: bit-equal ({got.numel()} elements)")
        return 0.0
    g64 = got.double()
    assert bool(torch.isfinite(g64).all()), f"{name}: non-finite output"
    ratio = worst_ratio((g64 - ex.ref).abs(), ex.allowed)
    if not quiet:
        exact = int((ex.allowed == 0).sum())
        print(f"  {name}: worst error / allowed = {ratio:.4f} ({exact} of {got.numel()} elements bit-equal by contract)")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio}"
    return ratio


# ---- the case lists (each edge once, not their product) ----

VARIANTS = ("1", "5", "11", "13")
# K: 8 / 72 (K % 64 != 0: the ring loop with a zero-filled K tail), 136, 448 (< 8 K-tiles: variant 5 under 13), 512
# (the shortest staggered prologue), 576 (an odd tile count), 1024
MAIN_KS = (8, 72, 136, 448, 512, 576, 1024)


def main_loop_cases():
    """per main loop (run under every VP_GEMM_VARIANT): BIAS at every K, ragged M and N, lda > K, ldc > N; the gated
    epilogue (whose instance differs per loop) at one K of each loop family"""
    cs = [case(f"bias K={K}", BIAS, 257, K, 264, lda_pad=8, ldc_pad=8, seed=K) for K in MAIN_KS]
    cs += [case(f"gated K={K}", GATED, 514, K, 264, tpb=257, T=1, inject="random", lda_pad=8, ldc_pad=8, seed=K + 1)
           for K in (72, 448, 576)]
    return cs


def row_col_cases():
    cs = [case(f"bias M={M}", BIAS, M, 512, 264, lda_pad=16, ldc_pad=24, seed=M) for M in (1, 255, 256, 257, 513)]
    cols = [(8, 1), (264, 1), (88, 3), (64, 3), (320, 3), (256, 3)]
    cs += [case(f"bias N={n}x{s}", BIAS, 257, 512, n, nsegs=s, seed=n + s) for n, s in cols]
    cs += [case("bias N=88x3 K=72", BIAS, 257, 72, 88, nsegs=3, seed=5),
           case("scale N=88x3", SCALE, 257, 512, 88, nsegs=3, ldc_pad=8, seed=6),
           case("scale N=264 K=136", SCALE, 300, 136, 264, seed=7),
           case("gelu N=264", GELU, 300, 512, 264, ldc_pad=8, seed=8),
           case("gelu aux N=264", GELU, 300, 512, 264, aux=True, seed=9),
           case("gelu aux N=264 K=136", GELU, 300, 136, 264, aux=True, seed=10),
           case("gelu_bwd N=264", GELU_BWD, 300, 512, 264, ldc_pad=8, seed=11),
           case("gelu_bwd N=264 K=136", GELU_BWD, 300, 136, 264, seed=12),
           case("gelu N=320x3", GELU, 257, 512, 320, nsegs=3, seed=13)]
    return cs


GATED_TRIPLES = ((3, 256, 0), (2, 257, 1), (2, 300, 256), (2, 300, 300), (2, 320, 64), (4, 100, 7))


def gated_cases():
    """K = 512: the default loop's compile-time gated instance, i.e. the row pass (tokens_per_batch >= 256) and, for
    (4, 100, 7), the per-row form with several batch boundaries in one tile.  N = 264: a ragged second column tile."""
    cs = []
    for i, (B, tpb, T) in enumerate(GATED_TRIPLES):
        for mode in (INJECT_MODES if T < tpb else INJECT_MODES[:2]):
            cs.append(case(f"gated B={B} tpb={tpb} T={T} inject={mode}", GATED, B * tpb, 512, 264, tpb=tpb, T=T,
                           inject=mode, seed=20 + i))
    cs += [case("gated inject_ld > N", GATED, 600, 512, 264, tpb=300, T=256, inject="random", inject_pad=16, seed=30),
           case("gated R = C", GATED, 600, 512, 264, tpb=300, T=256, inject="random", alias_R=True, ldc_pad=8, seed=31),
           case("gated R = C per-row", GATED, 400, 512, 264, tpb=100, T=7, inject="random", alias_R=True, seed=32),
           # the row remap: every batch's rows land after `row_offset` rows of a longer output stream
           case("gated remap row pass", GATED, 600, 512, 264, tpb=300, T=256, inject="random", rpg=300, gs=310, ro=5,
                seed=33),
           case("gated remap per-row", GATED, 400, 512, 264, tpb=100, T=7, inject="random", rpg=100, gs=110, ro=5,
                ldc_pad=8, seed=34),
           case("gated N=64x3", GATED, 514, 512, 64, nsegs=3, tpb=257, T=1, inject="first", seed=35)]
    return cs


def addrows_cases():
    """the patch-embed placement: rows_per_group = Nv video rows of each batch placed after its T text rows"""
    cs = []
    for Nv, T, pad in ((250, 10, 0), (300, 7, 16)):
        cs.append(case(f"addrows Nv={Nv} T={T} ld+{pad}", ADDROWS, 2 * Nv, 136, 264, rpg=Nv, gs=T + Nv, ro=T,
                       addrows_offset=T, addrows_pad=pad, seed=40 + pad))
    cs.append(case("addrows N=320x3 K=512", ADDROWS, 2 * 300, 512, 320, nsegs=3, rpg=300, gs=307, ro=7,
                   addrows_offset=7, seed=42))
    return cs


def splitk_cases():
    cs = []
    shapes = [(1, 1024), (37, 2560), (452, 1024), (452, 2560), (37, 1024), (1, 2560)]
    epis = [(BIAS, {}), (GELU, dict(aux=True)), (SCALE, {}), (ADDROWS, dict(addrows_offset=3)), (GELU_BWD, {}),
            (GATED, dict(inject="random"))]
    for i, ((M, K), (epi, kw)) in enumerate(zip(shapes, epis)):
        if epi == GATED:
            kw = dict(kw, tpb=max(1, M // 2), T=min(5, M // 4))
        cs.append(case(f"splitk {EPI_NAMES[epi]} M={M} K={K}", epi, M, K, 88, nsegs=3, ws="split", ldc_pad=8,
                       seed=50 + i, **kw))
    cs.append(case("splitk gated M=452 K=1024", GATED, 452, 1024, 264, tpb=226, T=26, inject="last", ws="split",
                   seed=57))
    return cs


def tail_cases():
    """4352 x 4096 x 1024: 17 x 16 = 272 tiles on 256 CUs, the last 16 as split-K workgroups and a reduce"""
    return [case("tail bias", BIAS, 4352, 1024, 4096, ws="tail", seed=60),
            case("tail gated inject", GATED, 4352, 1024, 4096, tpb=2176, T=226, inject="random", ws="tail", seed=60),
            case("tail gelu aux", GELU, 4352, 1024, 4096, aux=True, ws="tail", seed=60)]


def a_tail_cases():
    return [case("a_tail bias 3 segments", BIAS, 300, 576, 256, nsegs=3, a_tail=(512, 64), lda_pad=8, seed=70),
            case("a_tail gated", GATED, 600, 576, 256, tpb=300, T=37, inject="random", a_tail=(512, 64), seed=71),
            case("a_tail qknorm", QKNORM, 2 * 77, 576, 256, nsegs=3, H=4, tpb=77, T=5, rope="full",
                 a_tail=(512, 64), seed=72)]


QK_GRID = (3, 8, 12)  # 288 video rows


def qknorm_cases():
    """tokens_per_batch = T + 288 (or 288, or all text): batch and text boundaries inside a 256-row tile"""
    cs = []
    nv = QK_GRID[0] * QK_GRID[1] * QK_GRID[2]
    for i, (H, T, rope, aux, K) in enumerate([(1, 0, "full", False, 512), (5, 5, "full", True, 512),
                                              (1, 5, None, True, 136), (5, 0, None, False, 512),
                                              (5, 5, "sep", False, 512), (1, 5, "sep", True, 72)]):
        cs.append(case(f"qknorm H={H} T={T} rope={rope} aux={aux} K={K}", QKNORM, 2 * (T + nv), K, H * 64, nsegs=3,
                       H=H, tpb=T + nv, T=T, rope=rope, grid=QK_GRID if rope == "sep" else None, aux=aux, seed=80 + i))
    # T = tokens_per_batch: all rows text, no table row may be read
    cs.append(case("qknorm H=5 T=tpb=150", QKNORM, 300, 512, 320, nsegs=3, H=5, tpb=150, T=150, rope="full", seed=87))
    return cs


def mx_cases():
    """vp_gemm_mx_fp8: K = 128 / 640 run the unstaggered MX loop, K = 1024 (>= 8 K-steps) the staggered default"""
    return [case("mx bias M=255 N=256 K=128", BIAS, 255, 128, 256, api="mx", seed=90),
            case("mx bias M=513 N=256x3 K=640", BIAS, 513, 640, 256, nsegs=3, api="mx", seed=91),
            case("mx bias M=513 N=768 K=1024", BIAS, 513, 1024, 768, api="mx", seed=92),
            case("mx scale M=255 N=768 K=640", SCALE, 255, 640, 768, api="mx", seed=93),
            case("mx gated M=510 N=256 K=1024", GATED, 510, 1024, 256, api="mx", tpb=255, T=9, inject="random", seed=94),
            case("mx gated M=513 N=256x3 K=128", GATED, 513, 128, 256, nsegs=3, api="mx", tpb=171, T=9,
                 inject="random", seed=95),
            case("mx addrows M=510 N=256 K=640", ADDROWS, 510, 640, 256, api="mx", rpg=255, gs=260, ro=5,
                 addrows_offset=5, seed=96),
            case("mx gelu aux M=255 N=256 K=1024", GELU_MX, 255, 1024, 256, api="mx", aux=True, seed=97),
            case("mx gelu aux M=513 N=768 K=128", GELU_MX, 513, 128, 768, api="mx", aux=True, seed=98)]


def all_case_lists():
    return dict(small_case_lists(), tail=tail_cases())


def small_case_lists():
    """name -> cases, everything but the tail-mode shape (whose reference is too large for the mutant sweep)"""
    return {"main_loops": main_loop_cases(), "rows_cols": row_col_cases(), "gated": gated_cases(),
            "addrows": addrows_cases(), "splitk": splitk_cases(), "a_tail": a_tail_cases(),
            "qknorm": qknorm_cases(), "mx": mx_cases()}


# ------------------------------------------------------------------------------------------------------------------
# accumulation precision, real-valued operands
# ------------------------------------------------------------------------------------------------------------------

ACCUM_KS = (136, 512, 3072)


def accum_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return _randbf(g, M, K), _randbf(g, N, K, std=K ** -0.5), _randbf(g, N, std=0.1)


def accum_bound(a, w, bias):
    """y64 = a w^T + bias in float64 and the per-element allowance of C = rnd(acc + bias) with an fp32 accumulator:
    products of bf16 values are exact in fp32, and K fp32 additions (the bias among them) in any order err by at most
    K 2^-24 E, E = sum |a| |w| + |bias| (first order; (K - 1) additions of the products and one of the bias);
    then one rounding to bf16 of a value within g of y64: |got - y64| <= g + U8 (|y64| + g).  Derived, not measured."""
    a64, w64, b64 = a.double(), w.double(), bias.double()
    y = a64 @ w64.T + b64
    g = a.shape[1] * 2.0 ** -24 * (a64.abs() @ w64.abs().T + b64.abs())
    return y, g + U8 * (y.abs() + g)


# ------------------------------------------------------------------------------------------------------------------
# vp_head_norm_rope_bf16 forward: the extra cases next to backward_refs.HEAD_CASES
# ------------------------------------------------------------------------------------------------------------------

def head_fwd_mask(B, N, seed=5):
    """a token mask with both values among the text and the video rows"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N, generator=g) > 0.4).to(torch.uint8)


def rot_bias_bits(lb, H, rope):
    """What vp_head_norm_rope_bf16 writes for a zeroed input row, bit for bit, per video position: [rows, H 64] bf16.
    LN(64) of a zero row is fma(0 * rstd, w, b) = the bias b exactly; then the rotation in the order of
    ln64_rope16_regs (vp_common.h), every step one fp32 operation: y0 = fma(b0, c0, -fl32(b1 s0)),
    y1 = fma(b1, c1, fl32(b0 s1)), then one rounding to bf16.  A bf16 x fp32 product is exact in float64, so
    fl32 / fma are float64 evaluations rounded once to float32.  rope None / no rows: the bias itself."""
    b = lb.detach().cpu().double()
    if rope is None:
        return lb.detach().cpu().to(BF).repeat(H)[None]
    cos, sin = (t.detach().cpu().double() for t in rope)
    (b0, b1), (c0, c1), (s0, s1) = _pairs(b), _pairs(cos), _pairs(sin)
    p0, p1 = (b1 * s0).float().double(), (b0 * s1).float().double()
    y = _inter((b0 * c0 - p0).float(), (b1 * c1 + p1).float())
    return y.to(BF).repeat(1, H)


# ------------------------------------------------------------------------------------------------------------------
# the AdaLN modulation's chain, bit for bit: y = rnd(rnd(n s1) + shift), n = rnd(LN(x) w + b), s1 = rnd(1 + scale)
# ------------------------------------------------------------------------------------------------------------------
# Rows of +-0.5 in equal numbers with eps = 0.75: the mean is 0 and var + eps = 1 exactly in any summation order, so
# rstd = 1, LN(x) = +-0.5, and +-0.5 w + b is exact in fp32: n and every later step are single roundings of exactly
# known values, as in the GEMM cases.  (vp_final_norm_bf16: first norm w = 1, b = 0, so its output is the same row.)

ADALN_EXACT_DS = (8, 520, 3072)
ADALN_EXACT_EPS = 0.75
ADALN_EXACT_B, ADALN_EXACT_N = 2, 19


def adaln_exact_case(D):
    g = torch.Generator().manual_seed(5000 + D)
    B, N = ADALN_EXACT_B, ADALN_EXACT_N
    x = torch.empty(B, N, D)
    half = torch.cat([torch.full((D // 2,), 0.5), torch.full((D // 2,), -0.5)])
    for b in range(B):
        for n in range(N):
            x[b, n] = half[torch.randperm(D, generator=g)]
    mod = torch.full((B, 6 * D + 64), 7.0)
    mod[:, :6 * D] = 0.5 * torch.randn(B, 6 * D, generator=g)
    return dict(x=x.to(BF), lw=(1 + 0.2 * torch.randn(D, generator=g)).to(BF),
                lb=(0.1 * torch.randn(D, generator=g)).to(BF), mod=mod.to(BF))


def adaln_exact_ref(c, T, final=False, product_rnd=True):
    """the expected bits [rows, D] (bf16) of vp_adaln_modulate_bf16 (chunks shift 0 / scale 1 for video rows, 3 / 4
    for text rows) or, final=True, of vp_final_norm_bf16 on the video rows (mod = shift | scale).
    product_rnd=False: the mutant without rnd(n s1)."""
    x, mod = c["x"].float(), c["mod"].float()
    B, N, D = x.shape
    assert bool((x.sum(-1) == 0).all()) and bool((x.abs() == 0.5).all())
    n = rnd_bf16(x * c["lw"].float() + c["lb"].float())  # +-0.5 w + b: exact in fp32, then one rounding
    if final:
        n, shift, scale = n[:, T:], mod[:, None, :D], mod[:, None, D:2 * D]
    else:
        text = (torch.arange(N) < T)[None, :, None]
        shift = torch.where(text, mod[:, None, 3 * D:4 * D], mod[:, None, :D])
        scale = torch.where(text, mod[:, None, 4 * D:5 * D], mod[:, None, D:2 * D])
    p = n * rnd_bf16(1.0 + scale)  # exact: two bf16 factors
    if product_rnd:
        p = rnd_bf16(p)
    return rnd_bf16(p + shift).to(BF).reshape(-1, D)
