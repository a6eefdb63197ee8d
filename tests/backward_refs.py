"""Plain-torch CPU references of the row / elementwise kernels of csrc/backward.hip and of their forward twins in
csrc/norm.hip, one function per entry point, written from the formulas documented in include/vp_hip.h.

Every function widens its (bf16) inputs to `dt` (float64 unless stated) and returns UNROUNDED results in `dt`; where
a tolerance needs it, it also returns a magnitude scale `E_*`: the same formula with the absolute values of its
terms, i.e. what a relative error of one working-precision rounding per term amounts to.  Nothing here imports the
package under test.  tests/test_backward_refs_cpu.py checks each function against torch.autograd / a one-line torch
form, and measures the c_f32 constants (below) by running these same functions with dt = float32.

The case generators at the end are shared by the CPU measurement and the GPU tests, so the constants are measured on
exactly the inputs they are used with.
"""
import math

import torch

F64 = torch.float64
K0 = math.sqrt(2.0 / math.pi)
K1 = 0.044715

# c_f32: error of an fp32 evaluation of a row formula, in units of its magnitude scale E.  Measured, not chosen:
# tests/test_backward_refs_cpu.py::test_c_f32_constants evaluates the reference functions below in float32 torch on
# the CPU over every case of the GPU tests, takes the worst |fp32 - fp64| / E and multiplies by 8 (the kernels' wave
# reduction order and rsqrtf differ from torch's); the constants here are those products rounded up to two digits.
# That test repeats the measurement and fails if 8 x worst leaves [C / 2, C].  In the final_norm cases the float32
# evaluation of the second norm starts from the float64 evaluation's rounded first norm (bf16 values, exact in
# float32), so that every case is measured and what is measured is arithmetic, not a rounding decided the other way.
#   AdaLN rows (adaln_bwd, adaln_modulate, final_norm cases):  worst 2.490e-07  ->  x 8 = 1.992e-06
#   head vectors (head_norm_rope_bwd cases):                   worst 1.630e-07  ->  x 8 = 1.304e-06
C_F32_ADALN = 2.0e-06
C_F32_HEAD = 1.4e-06


def wide(t, dt=F64):
    return t.detach().cpu().to(dt)


def rnd_bf16(x):
    """Round to the nearest bf16 (ties to even), result in x's dtype.  float64 goes through float32 first; where
    that first rounding lands exactly on a bf16 tie that the exact value is not on, step one fp32 ulp back towards
    the exact value so that the second rounding goes the right way."""
    if x.dtype != F64:
        return x.to(torch.bfloat16).to(x.dtype)
    f = x.to(torch.float32)
    bits = f.view(torch.int32)
    resid = x - f.double()
    tie = ((bits & 0xFFFF) == 0x8000) & (resid != 0) & torch.isfinite(f)
    step = torch.where((resid > 0) == (f > 0), 1, -1).to(torch.int32)
    f = torch.where(tie, bits + step, bits).view(torch.float32)
    return f.to(torch.bfloat16).to(F64)


def bf16_ulps(a, b):
    """|a - b| in bf16 units in the last place (a, b bf16 tensors of finite values)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)
    return (key(a) - key(b)).abs()


def worst_ratio(err, allowed):
    """max over elements of err / allowed, with 0 / 0 = 0 (an exact result needs no allowance)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    r = torch.nan_to_num(r, nan=float("inf"))
    return float(r.max()) if r.numel() else 0.0


def row_kind(rows, ntok, text_len):
    m = torch.arange(rows)
    return m // ntok, (m % ntok) < text_len


def mod_rows(mod, D, ntok, text_len, ch_v, ch_t, rows, dt=F64):
    """chunk ch_v (video rows) / ch_t (text rows) of mod [B, >= 6 D] for each of `rows` rows: [rows, D]"""
    m = wide(mod, dt)
    b, text = row_kind(rows, ntok, text_len)
    mv = m[:, ch_v * D:(ch_v + 1) * D][b]
    mt = m[:, ch_t * D:(ch_t + 1) * D][b]
    return torch.where(text[:, None], mt, mv)


# ------------------------------------------------------------------------------------------------------------------
# data movement, sums, elementwise
# ------------------------------------------------------------------------------------------------------------------

def transpose_ref(x, pad_to=1):
    """x [nb, R, C] -> [C, nb * R rounded up to pad_to], batch b in columns b R ..; pad columns zero (x's dtype)"""
    x = x.detach().cpu()
    nb, R, C = x.shape
    cols = nb * R
    out = torch.zeros(C, (cols + pad_to - 1) // pad_to * pad_to, dtype=x.dtype)
    for b in range(nb):
        for r in range(R):
            out[:, b * R + r] = x[b, r]
    return out


def colsum_ref(a, b, ntok, text_len, dt=F64):
    """(sums, sums of |terms|), each [rows / ntok, 2, cols]: index 1 = the text rows (m % ntok < text_len)"""
    p = wide(a, dt) if b is None else wide(a, dt) * wide(b, dt)
    rows, cols = p.shape
    bi, text = row_kind(rows, ntok, text_len)
    nb = rows // ntok
    s = torch.zeros(nb, 2, cols, dtype=dt)
    sa = torch.zeros(nb, 2, cols, dtype=dt)
    for m in range(rows):
        s[bi[m], int(text[m])] += p[m]
        sa[bi[m], int(text[m])] += p[m].abs()
    return s, sa


def rowscale_ref(x, mod, ntok, text_len, ch_v, ch_t, dt=F64):
    x = wide(x, dt)
    rows, D = x.shape
    return x * mod_rows(mod, D, ntok, text_len, ch_v, ch_t, rows, dt)


def axpy_ref(a, b, alpha, dt=F64):
    return wide(a, dt) + alpha * wide(b, dt)


def _gelu_s(z):
    u2 = 2.0 * K0 * (z + K1 * z * z * z)
    return torch.sigmoid(u2), torch.sigmoid(-u2)  # s and 1 - s, each to full relative accuracy


def gelu_ref(z, dt=F64):
    """z s with s = 1 / (1 + exp(-2 u)) = (1 + tanh u) / 2, u = sqrt(2 / pi) (z + 0.044715 z^3)"""
    z = wide(z, dt)
    return z * _gelu_s(z)[0]


def gelu_bwd_ref(dh, z, dt=F64):
    """dh (s + z s (1 - s) 2 u')"""
    z = wide(z, dt)
    s, sm = _gelu_s(z)
    up2 = 2.0 * K0 * (1.0 + 3.0 * K1 * z * z)
    return wide(dh, dt) * (s + ((z * sm) * s) * up2)


def silu_ref(x, dt=F64):
    x = wide(x, dt)
    return x * torch.sigmoid(x)


def silu_bwd_ref(dy, x, dt=F64):
    """dy s (1 + x (1 - s))"""
    x = wide(x, dt)
    s, sm = torch.sigmoid(x), torch.sigmoid(-x)
    return wide(dy, dt) * (s + (x * sm) * s)


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm rows
# ------------------------------------------------------------------------------------------------------------------

def _ln_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xhat = (x - mean) * rstd
    e_xhat = (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd
    return rstd, xhat, e_xhat


def _ln_bwd(dxhat, xhat, rstd):
    """LN' and its magnitude scale E = rstd (|dxhat| + mean|dxhat| + |xhat| mean|dxhat xhat|)"""
    g1 = dxhat.mean(-1, keepdim=True)
    g2 = (dxhat * xhat).mean(-1, keepdim=True)
    delta = rstd * (dxhat - g1 - xhat * g2)
    E = rstd * (dxhat.abs() + dxhat.abs().mean(-1, keepdim=True)
                + xhat.abs() * (dxhat * xhat).abs().mean(-1, keepdim=True))
    return delta, E


def adaln_s1_shift(mod, D, ntok, text_len, chunks, rows, dt=F64):
    """s1 = bf16(1 + scale) and shift per row, [rows, D] each (chunks = shift_v, scale_v, shift_t, scale_t)"""
    sh_v, sc_v, sh_t, sc_t = chunks
    s1 = rnd_bf16(1.0 + mod_rows(mod, D, ntok, text_len, sc_v, sc_t, rows, dt))
    return s1, mod_rows(mod, D, ntok, text_len, sh_v, sh_t, rows, dt)


def adaln_bwd_ref(x, dy, mod, lw, lb, eps, text_len, chunks=(0, 1, 3, 4), dt=F64):
    """x, dy [B, N, D].  n = LN(x) w + b, dn = dy s1, xhat = LN(x) without the affine, delta = LN'(dn w) (the
    kernel's dx is old + delta), all [B N, D] unrounded, with their magnitude scales E_*."""
    B, N, D = x.shape
    rows = B * N
    xw, dyw = wide(x, dt).reshape(rows, D), wide(dy, dt).reshape(rows, D)
    w, b = wide(lw, dt), wide(lb, dt)
    s1, _ = adaln_s1_shift(mod, D, N, text_len, chunks, rows, dt)
    rstd, xhat, e_xhat = _ln_stats(xw, eps)
    dn = dyw * s1
    delta, E = _ln_bwd(dn * w, xhat, rstd)
    return dict(n=xhat * w + b, dn=dn, xhat=xhat, delta=delta, E_n=e_xhat * w.abs() + b.abs(), E_dn=dn.abs(),
                E_xhat=e_xhat, E_dx=E)


def adaln_modulate_ref(x, mod, lw, lb, eps, text_len, dt=F64):
    """vp_adaln_modulate_bf16: y = rnd(rnd(n s1) + shift), n = rnd(LN(x) w + b), s1 = rnd(1 + scale).
    Returns y with the three roundings of the data path left out (s1, which both sides compute exactly, rounded),
    `mag` = |n s1| + |rnd(n s1)| + |y| from the rounded chain (one term per omitted rounding: a result that rounds
    at those three points lies within 2^-8 mag of the unrounded value), and the fp32 scale E."""
    B, N, D = x.shape
    rows = B * N
    xw = wide(x, dt).reshape(rows, D)
    w, b = wide(lw, dt), wide(lb, dt)
    s1, shift = adaln_s1_shift(mod, D, N, text_len, (0, 1, 3, 4), rows, dt)
    return _modulate(xw, w, b, eps, s1, shift)


def _modulate(xw, w, b, eps, s1, shift):
    rstd, xhat, e_xhat = _ln_stats(xw, eps)
    n = xhat * w + b
    y = n * s1 + shift
    nr = rnd_bf16(n)
    pr = rnd_bf16(nr * s1)
    mag = (nr * s1).abs() + pr.abs() + rnd_bf16(pr + shift).abs()
    E = (e_xhat * w.abs() + b.abs()) * s1.abs() + shift.abs()
    return dict(y=y, mag=mag, E=E, n=n)


def final_norm_ref(x, text_len, w1, b1, w2, b2, eps, mod, dt=F64, n1_rounded=None):
    """vp_final_norm_bf16 on the video rows: y = rnd(rnd(n2 s1) + shift), n2 = rnd(LN2(n1)), n1 = rnd(LN1(x)),
    mod [B, 2 D] = shift | scale.  n1 is rounded here (it is the input of the second LayerNorm, as stated in the
    header); the last three roundings are left out and bounded by `mag` as in adaln_modulate_ref.
    n1_rounded: bf16 values [B Nv, D] to use as the rounded n1 instead of this evaluation's own (the c_f32
    measurement hands the float32 evaluation the float64 one's, so that it measures the arithmetic of the second
    norm on the same input)."""
    B, N, D = x.shape
    Nv = N - text_len
    xw = wide(x, dt)[:, text_len:].reshape(B * Nv, D)
    rstd, xhat, e_xhat = _ln_stats(xw, eps)
    n1 = xhat * wide(w1, dt) + wide(b1, dt)
    e_n1 = e_xhat * wide(w1, dt).abs() + wide(b1, dt).abs()
    n1r = rnd_bf16(n1) if n1_rounded is None else wide(n1_rounded, dt)
    m = wide(mod, dt)
    bi = torch.arange(B * Nv) // Nv
    s1 = rnd_bf16(1.0 + m[:, D:2 * D][bi])
    out = _modulate(n1r, wide(w2, dt), wide(b2, dt), eps, s1, m[:, :D][bi])
    out.update(n1_exact=n1, n1_rounded=n1r, E_n1=e_n1)
    return out


def rope_t(dy, cos, sin):
    """transpose of apply_rotary_emb (y0 = n0 c0 - n1 s0, y1 = n1 c1 + n0 s1 on interleaved pairs) and the sum of
    the absolute values of its two terms; dy [..., Nv, 64], cos / sin [Nv, 64]"""
    d0, d1 = dy[..., 0::2], dy[..., 1::2]
    c0, c1, s0, s1 = cos[..., 0::2], cos[..., 1::2], sin[..., 0::2], sin[..., 1::2]
    dn = torch.stack((d0 * c0 + d1 * s1, d1 * c1 - d0 * s0), -1).flatten(-2)
    mag = torch.stack(((d0 * c0).abs() + (d1 * s1).abs(), (d1 * c1).abs() + (d0 * s0).abs()), -1).flatten(-2)
    return dn, mag


def head_norm_rope_bwd_ref(x, dy, lw, lb, eps, heads, text_len, rope=None, dt=F64):
    """x, dy [B, N, heads * 64].  dx = LN64'(RoPE^T(dy) w) per head vector ([B, N, heads * 64]) with its scale E,
    dlw = sum dn xhat, dlb = sum dn over all vectors ([64]) with the sums of |terms|."""
    B, N, _ = x.shape
    xw = wide(x, dt).reshape(B, N, heads, 64)
    dn = wide(dy, dt).reshape(B, N, heads, 64).clone()
    mag = dn.abs()
    if rope is not None:
        cos, sin = (wide(t, dt)[:, None, :] for t in rope)  # [Nv, 1, 64]: broadcast over heads
        r, m = rope_t(dn[:, text_len:], cos, sin)
        dn[:, text_len:] = r
        mag[:, text_len:] = m
    w = wide(lw, dt)
    rstd, xhat, _ = _ln_stats(xw, eps)
    delta, _ = _ln_bwd(dn * w, xhat, rstd)
    _, E = _ln_bwd(mag * w.abs(), xhat, rstd)
    tw = (dn * xhat).reshape(-1, 64)
    tb = dn.reshape(-1, 64)
    tw_mag = (mag * xhat.abs()).reshape(-1, 64)
    return dict(dx=delta.reshape(B, N, heads * 64), E=E.reshape(B, N, heads * 64), dlw=tw.sum(0), dlb=tb.sum(0),
                S_w=tw_mag.sum(0), S_b=mag.reshape(-1, 64).sum(0))


# ------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_backward_kernels_gpu.py (bf16 CPU tensors, fixed seeds)
# ------------------------------------------------------------------------------------------------------------------

ADALN_B, ADALN_N = 2, 19  # rows % 4 == 2
ADALN_DS = (8, 384, 520, 1032, 2056, 3072, 3080, 4096)  # every NCH instance, every partially filled last chunk
ADALN_TEXT = (0, 5, 19)
ADALN_CHUNKS = ((0, 1, 3, 4), (0, 1, 0, 1))
FINAL_DS = (8, 520, 3072, 4096)
EPS_ADALN = 1e-5


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def adaln_case(D, mod_extra=0):
    """x = 3 randn + 1 with one constant and one all-zero row; mod [B, 6 D + mod_extra]"""
    g = torch.Generator().manual_seed(1000 + D)
    B, N = ADALN_B, ADALN_N
    x = _randn(g, B, N, D) * 3 + 1
    x[0, 3] = 1.5
    x[1, 7] = 0.0
    c = dict(x=x, dy=_randn(g, B, N, D), old=_randn(g, B, N, D), lw=1 + 0.1 * _randn(g, D), lb=0.1 * _randn(g, D),
             lw2=1 + 0.1 * _randn(g, D), lb2=0.1 * _randn(g, D))
    mod = torch.full((B, 6 * D + mod_extra), 7.0)
    mod[:, :6 * D] = 0.5 * _randn(g, B, 6 * D)
    c["mod"] = mod
    return {k: v.bfloat16() for k, v in c.items()}


def axpy_inputs(n):
    g = torch.Generator().manual_seed(3000 + n)
    return _randn(g, n).bfloat16(), (_randn(g, n) * 0.7).bfloat16()


ROWSCALE_NTOK = 37


def rowscale_inputs(D):
    """x [2 * 37, D], mod [2, 6 D + 64] (row stride wider than 6 D, the gap poisoned)"""
    g = torch.Generator().manual_seed(4000 + D)
    mod = torch.full((2, 6 * D + 64), 7.0)
    mod[:, :6 * D] = _randn(g, 2, 6 * D)
    return _randn(g, 2 * ROWSCALE_NTOK, D).bfloat16(), mod.bfloat16()


HEAD_EPS = 1e-6
# (heads, text_len, kind): kind "rope" = text_len text rows + the RoPE grid's video rows, "text" = all rows text
# (N = text_len, no table row is read), "norope" = rope=None.  The grid (32 x 48 pixels = 2 x 3 patches, 2 frames: 12 rows)
# keeps B N heads off a multiple of 64, so the last block has clamped invalid vectors.
HEAD_CASES = [(H, T, "rope") for H in (1, 3) for T in (0, 8)] + [(3, 8, "text"), (1, 8, "norope")]
HEAD_B = 2


def head_rope():
    from oracle.cogvideox_oracle import prepare_rotary_positional_embeddings
    cos, sin = prepare_rotary_positional_embeddings(32, 48, 2, 64)
    return cos.float().contiguous(), sin.float().contiguous()


def head_case(H, T, kind):
    """qkv / dqkv: fused [B, N, 3 H 64] buffers whose q (slice 0) and k (slice 1) column slices are the operands;
    row 2 of batch 1 is zero in both (the null key's LN(0))."""
    g = torch.Generator().manual_seed(2000 + 100 * H + 10 * T + len(kind))
    cos, sin = head_rope()
    Nv = cos.shape[0]
    N = T if kind == "text" else T + Nv
    qkv = _randn(g, HEAD_B, N, 3 * H * 64) * 2 + 0.5
    qkv[1, 2] = 0.0
    dqkv = _randn(g, HEAD_B, N, 3 * H * 64)
    c = dict(qkv=qkv.bfloat16(), dqkv=dqkv.bfloat16(), lw=(1 + 0.2 * _randn(g, 64)).bfloat16(),
             lb=(0.1 * _randn(g, 64)).bfloat16(), N=N)
    # "text": the first 0 rows of the table (a non-NULL pointer of which no row may be read)
    c["rope"] = None if kind == "norope" else (cos, sin)
    c["rope_rows"] = Nv if kind == "rope" else 0
    return c


def head_operands(c, H, which, dt=F64):
    """the q (which = 0) or k (1) column slice of the case's two fused buffers, and its rope tables, for the ref"""
    sl = slice(which * H * 64, (which + 1) * H * 64)
    rope = None if c["rope"] is None else tuple(t[:c["rope_rows"]] for t in c["rope"])
    return c["qkv"][..., sl], c["dqkv"][..., sl], rope
