"""The row / elementwise kernels of csrc/backward.hip (and their forward twins in csrc/norm.hip) at their edges, per
element against the float64 references of tests/backward_refs.py (each checked on the CPU by
tests/test_backward_refs_cpu.py, where the c_f32 constants are measured too).

Every check is per element: `ratio` = max over elements of |got - ref| / allowed, asserted <= 1 and printed, so a
run with -s is the record of how far each kernel is from its bound.  Regions a kernel must not touch (stride gaps,
rows past the end, neighbouring slices) hold a sentinel and are compared afterwards.

U8 = 2^-8 is the largest relative error of one rounding to bf16 (half an ulp at the bottom of a binade)."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from tests import backward_refs as R

pytestmark = pytest.mark.gpu
dev = "cuda"
U8 = 2.0 ** -8
SENT = 7.0
BF = torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from videopainter_amd import kernels
    print(f"\nc_f32 (tests/backward_refs.py; measured by tests/test_backward_refs_cpu.py::test_c_f32_constants as 8 x "
          f"the worst |fp32 - fp64| / E of the reference formulas in float32 torch on the CPU, over these cases): "
          f"AdaLN rows {R.C_F32_ADALN:.2e}, head vectors {R.C_F32_HEAD:.2e}")
    return kernels


def check(name, got, ref, allowed, quiet=False):
    """per element |got - ref| <= allowed; returns the worst ratio, and prints it unless the caller sums it up"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    ratio = R.worst_ratio((got - ref).abs(), allowed)
    if not quiet:
        print(f"  {name}: worst error / allowed = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio}"
    return ratio


def check_rounded(name, got, ref64):
    """one operation and one rounding: within 1 bf16 ulp of bf16(ref) everywhere, bit-equal on >= 99.9 %"""
    want = R.rnd_bf16(ref64).to(BF)
    u = R.bf16_ulps(got.detach().cpu().reshape(want.shape), want)
    share = float((u == 0).double().mean())
    print(f"  {name}: max ulp {int(u.max())}, bit-equal {100 * share:.3f} %")
    assert int(u.max()) <= 1 and share >= 0.999, f"{name}: max ulp {int(u.max())}, bit-equal share {share}"


def guarded(shape_rows, D, rows, fill=None):
    """a [rows, D] bf16 device tensor that is the head of a [rows + 4, D] buffer of sentinels (rows past the end)"""
    buf = torch.full((rows + 4, D), SENT, device=dev, dtype=BF)
    t = buf[:rows]
    if fill is not None:
        t.copy_(fill.reshape(rows, D))
    return buf, t.view(*shape_rows, D)


def tail_intact(buf, rows):
    return bool((buf[rows:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------
# a. the unary kernels over every bf16 bit pattern
# ------------------------------------------------------------------------------------------------------------------

def _all_bf16():
    z = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    z64 = z.double()
    finite = torch.isfinite(z64)
    inr = finite & (z64.abs() <= 2.0 ** 60)
    return z, z64, finite, inr


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_unary_forward_every_bf16(K, name):
    z, z64, finite, inr = _all_bf16()
    assert int((~finite).sum()) == 256  # inf and NaN patterns: the only inputs without a value check
    got = getattr(K, name)(z.to(dev)).cpu()
    ref = getattr(R, name + "_ref")(z)
    allowed = U8 * ref.abs() + 2.0 ** -118
    check(f"{name} |z| <= 2^60 ({int(inr.sum())} patterns)", got[inr], ref[inr], allowed[inr])
    # beyond 2^60: saturated exactly (vp_common.h: 2^(+big) = inf -> rcp = 0 -> -0; 2^(-big) = 0 -> z)
    big = finite & ~inr
    pos, neg = big & (z64 > 0), big & (z64 < 0)
    assert int(inr.sum()) + int(pos.sum()) + int(neg.sum()) + 256 == 65536
    assert _same_bits(got[pos], z[pos]), f"{name}: z > 2^60 must come back unchanged"
    assert bool((got[neg] == 0).all()), f"{name}: z < -2^60 must give +-0"
    print(f"  {name} |z| > 2^60: {int(pos.sum())} patterns returned exactly, {int(neg.sum())} gave +-0")


@pytest.mark.parametrize("dh", [1.0, -0.375, 3.0e3])
@pytest.mark.parametrize("name", ["gelu_bwd", "silu_bwd"])
def test_unary_backward_every_bf16(K, name, dh):
    z, z64, finite, inr = _all_bf16()
    assert int((~finite).sum()) == 256
    d = torch.full((65536,), dh).to(BF)
    got = getattr(K, name)(d.to(dev), z.to(dev)).cpu()
    ref = getattr(R, name + "_ref")(d, z)
    allowed = U8 * ref.abs() + 2.0 ** -118 * max(1.0, abs(float(d[0])))
    check(f"{name} dh = {float(d[0])} |z| <= 2^60", got[inr], ref[inr], allowed[inr])
    big = finite & ~inr
    if name == "silu_bwd":
        # s = 1 / (1 + exp(-z)) is exactly 1 / 0 there and z (1 - s) meets no inf: dy back unchanged, or +-0
        pos, neg = big & (z64 > 0), big & (z64 < 0)
        assert _same_bits(got[pos], d[pos]) and bool((got[neg] == 0).all())
        print(f"  silu_bwd |z| > 2^60: {int(big.sum())} patterns saturate exactly")
    else:
        # vp_gelu_bwd_bf16's domain is |z| <= 2^60 (include/vp_hip.h): from |z| >= 2^64 on z^2 overflows fp32 and
        # the polynomial factor is inf against a zero, as in torch's fp32 formula.  No value is asserted there.
        print(f"  gelu_bwd |z| > 2^60: {int(big.sum())} finite patterns outside the documented domain, "
              f"{int(torch.isnan(got[big].float()).sum())} of them NaN")


# ------------------------------------------------------------------------------------------------------------------
# b. axpy  c. rowscale  d. transpose  e. colsum
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [1.0, -0.5])
@pytest.mark.parametrize("n", [8, 8 * (256 * 3 + 5)])
def test_axpy(K, n, alpha):
    a, b = R.axpy_inputs(n)
    ref = R.axpy_ref(a, b, alpha)
    buf = torch.full((n + 16,), SENT, device=dev, dtype=BF)
    out = K.axpy(a.to(dev), b.to(dev), alpha, out=buf[8:8 + n])
    check_rounded(f"axpy n = {n} alpha = {alpha}", out, ref)
    assert bool((buf[:8] == SENT).all()) and bool((buf[8 + n:] == SENT).all())
    ad = a.to(dev)
    K.axpy(ad, b.to(dev), alpha, out=ad)  # out aliasing a (the residual accumulation)
    assert _same_bits(ad.cpu(), out.cpu())


@pytest.mark.parametrize("chunks", [(2, 5), (0, 0)])
@pytest.mark.parametrize("T", [0, 5, 37])
@pytest.mark.parametrize("D", [8, 136])
def test_rowscale(K, D, T, chunks):
    ntok = R.ROWSCALE_NTOK
    x, mod = R.rowscale_inputs(D)
    rows = x.shape[0]
    ref = R.rowscale_ref(x, mod, ntok, T, *chunks)
    xb = torch.full((rows + 2, D + 24), SENT, device=dev, dtype=BF)
    ob = torch.full((rows + 2, D + 24), SENT, device=dev, dtype=BF)
    xb[:rows, :D] = x.to(dev)
    md = mod.to(dev)
    assert md.stride(0) == 6 * D + 64
    K.rowscale(xb[:rows, :D], ob[:rows, :D], ntok, T, md, *chunks)
    got = ob[:rows, :D].cpu()
    check_rounded(f"rowscale D = {D} T = {T} chunks = {chunks}", got, ref)
    assert bool((ob[:, D:] == SENT).all()) and bool((ob[rows:] == SENT).all())
    # the two boundaries: text -> video inside batch 0, batch 0 -> batch 1
    m64 = mod.double()
    for row in (4, 5, 36, 37):
        bi, tok = divmod(row, ntok)
        ch = chunks[1] if tok < T else chunks[0]
        want = R.rnd_bf16(x[row].double() * m64[bi, ch * D:(ch + 1) * D]).to(BF)
        assert int(R.bf16_ulps(got[row], want).max()) <= 1, f"row {row}"
        if chunks[0] != chunks[1]:  # and the other chunk, or the other batch row, would not have passed
            other = chunks[0] if tok < T else chunks[1]
            for bj, cj in ((bi, other), (1 - bi, ch)):
                wrong = R.rnd_bf16(x[row].double() * m64[bj, cj * D:(cj + 1) * D]).to(BF)
                assert int(R.bf16_ulps(got[row], wrong).max()) > 1


@pytest.mark.parametrize("pad_to", [1, 64])
@pytest.mark.parametrize("nb,Rr,C", [(1, 1, 8), (1, 63, 65), (3, 77, 136), (2, 64, 64), (2, 130, 200)])
def test_transpose(K, nb, Rr, C, pad_to):
    g = torch.Generator().manual_seed(5000 + Rr)
    base = torch.randn(nb, Rr + 3, C + 8, generator=g).to(BF).to(dev)
    x = base[:, :Rr, :C]  # row stride C + 8, batch stride (R + 3) (C + 8) != R ld
    assert x.stride(1) == C + 8 and x.stride(0) != Rr * x.stride(1)
    cols = nb * Rr
    colp = (cols + pad_to - 1) // pad_to * pad_to
    off = 3
    wide = torch.full((C, off + colp + 5), SENT, device=dev, dtype=BF)
    out = K.transpose(x, out=wide[:, off:off + colp], pad_to=pad_to)
    want = R.transpose_ref(x, pad_to)
    assert want.shape == (C, colp) and torch.equal(want[:, :cols], x.cpu().reshape(cols, C).t())
    assert torch.equal(out.cpu(), want)
    assert not out[:, cols:].any()
    assert bool((wide[:, :off] == SENT).all()) and bool((wide[:, off + colp:] == SENT).all())
    assert torch.equal(K.transpose(x, pad_to=pad_to).cpu(), want)
    print(f"  transpose nb = {nb} R = {Rr} C = {C} pad_to = {pad_to}: equal, pad zero, outside untouched")


COLSUM_CASES = [(600, 96, 300, 8), (5 * 50, 2056, 50, 0), (5 * 50, 2056, 50, 50), (3 * 100, 4104, 100, 7),
                (257, 8, 257, 1)]


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("rows,cols,ntok,T", COLSUM_CASES)
def test_colsum(K, rows, cols, ntok, T, with_b):
    g = torch.Generator().manual_seed(6000 + cols + T)
    # a and b are column slices of wider buffers whose other columns hold a value that would wreck any sum
    ab = torch.full((rows, cols + 16), 1.0e4).to(BF)
    bb = torch.full((rows, cols + 8), 1.0e4).to(BF)
    ab[:, 8:8 + cols] = torch.randn(rows, cols, generator=g).to(BF)
    bb[:, :cols] = (torch.randn(rows, cols, generator=g) + 0.25).to(BF)
    a, b = ab[:, 8:8 + cols], (bb[:, :cols] if with_b else None)
    ad, bd = ab.to(dev)[:, 8:8 + cols], (bb.to(dev)[:, :cols] if with_b else None)
    ref, mag = R.colsum_ref(a, b, ntok, T)
    nb = rows // ntok
    stripes = (rows + 255) // 256
    tag = f"colsum {rows} x {cols} Ntok = {ntok} T = {T} b = {with_b}"
    got = K.colsum(ad, bd, tokens_per_batch=ntok, text_len=T)
    assert got.shape == (nb, 2, cols)
    check(tag, got, ref, 2.0 ** -24 * (256 + stripes + 2) * mag)
    if T == 0:
        assert not got[:, 1].any()
    if T == ntok:
        assert not got[:, 0].any()
    # accumulation into a non-zero out, itself inside a guarded buffer
    n = nb * 2 * cols
    before = torch.randn(n, generator=g) * 3
    obuf = torch.full((n + 8,), SENT, device=dev, dtype=torch.float32)
    obuf[4:4 + n] = before.to(dev)
    K.colsum(ad, bd, tokens_per_batch=ntok, text_len=T, out=obuf[4:4 + n].view(nb, 2, cols))
    b64 = before.double().view(nb, 2, cols)
    check(tag + " += ", obuf[4:4 + n], ref + b64, 2.0 ** -24 * (256 + stripes + 2) * mag + 2.0 ** -24 * b64.abs())
    assert bool((obuf[:4] == SENT).all()) and bool((obuf[4 + n:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------
# f. AdaLN backward  h. its forward twins
# ------------------------------------------------------------------------------------------------------------------

def _adaln_ref(c, T, chunks, cache={}):
    key = (c["x"].shape[-1], T, chunks)
    if key not in cache:
        cache[key] = R.adaln_bwd_ref(c["x"], c["dy"], c["mod"], c["lw"], c["lb"], R.EPS_ADALN, T, chunks)
    return cache[key]


@pytest.mark.parametrize("D", R.ADALN_DS)
def test_adaln_bwd(K, D):
    B, N = R.ADALN_B, R.ADALN_N
    rows = B * N
    cf = R.C_F32_ADALN
    worst = dict(n=0.0, dn=0.0, xhat=0.0, dx=0.0)  # per output, over the 12 cases below (each asserted on its own)
    ncase = 0
    for extra in (0, 64):
        c = R.adaln_case(D, extra)
        d = {k: v.to(dev) for k, v in c.items()}
        assert d["mod"].stride(0) == 6 * D + extra
        old64 = c["old"].double().reshape(rows, D)
        for T in R.ADALN_TEXT:
            for chunks in R.ADALN_CHUNKS:
                r = _adaln_ref(c, T, chunks)
                bufs = [guarded((B, N), D, rows) for _ in range(3)]
                dxb, dx = guarded((B, N), D, rows, d["old"])
                K.adaln_bwd(d["x"], d["dy"], dx, T, d["lw"], d["lb"], R.EPS_ADALN, d["mod"], chunks=chunks,
                            n_out=bufs[0][1], dn_out=bufs[1][1], xhat_out=bufs[2][1])
                dxb2, dx2 = guarded((B, N), D, rows, d["old"])
                K.adaln_bwd(d["x"], d["dy"], dx2, T, d["lw"], d["lb"], R.EPS_ADALN, d["mod"], chunks=chunks)
                assert _same_bits(dx.cpu(), dx2.cpu()), "dx must not depend on the optional outputs"
                assert all(tail_intact(bb, rows) for bb, _ in bufs) and tail_intact(dxb, rows) and tail_intact(dxb2, rows)
                tag = f"adaln_bwd D = {D} T = {T} chunks = {chunks} mod stride 6D+{extra}"
                for (_, t), k, e in zip(bufs, ("n", "dn", "xhat"), ("E_n", "E_dn", "E_xhat")):
                    worst[k] = max(worst[k], check(f"{tag} {k}_out", t, r[k], U8 * r[k].abs() + cf * r[e], quiet=True))
                want = old64 + r["delta"]
                worst["dx"] = max(worst["dx"], check(f"{tag} dx", dx, want, U8 * want.abs() + cf * r["E_dx"], quiet=True))
                ncase += 1
                # dx += : the same call on zeros differs from it wherever old is not zero
                assert float((dx.double().cpu().reshape(rows, D) - r["delta"]).abs().max()) > 0.5
    for k, v in worst.items():
        print(f"  adaln_bwd D = {D} {k}: worst error / allowed over {ncase} cases (text_len x chunks x mod stride) = {v:.4f}")


def test_adaln_bwd_against_autograd_at_production_width(K):
    """D = 3072 (NCH = 6): dx and the parameter sums against torch.autograd in float64"""
    D, T, B, N = 3072, 5, R.ADALN_B, R.ADALN_N
    rows = B * N
    c = R.adaln_case(D)
    d = {k: v.to(dev) for k, v in c.items()}
    x = c["x"].double().requires_grad_()
    w, b = c["lw"].double().requires_grad_(), c["lb"].double().requires_grad_()
    s1, shift = R.adaln_s1_shift(c["mod"], D, N, T, (0, 1, 3, 4), rows)
    s1.requires_grad_()
    y = F.layer_norm(x, (D,), w, b, R.EPS_ADALN).view(rows, D) * s1 + shift
    y.backward(c["dy"].double().view(rows, D))
    dx = torch.zeros(B, N, D, device=dev, dtype=BF)
    n_out, dn_out, xh_out = (torch.empty_like(dx) for _ in range(3))
    K.adaln_bwd(d["x"], d["dy"], dx, T, d["lw"], d["lb"], R.EPS_ADALN, d["mod"], n_out=n_out, dn_out=dn_out,
                xhat_out=xh_out)
    r = _adaln_ref(c, T, (0, 1, 3, 4))
    g = x.grad.view(rows, D)
    check("adaln_bwd D = 3072 dx against autograd", dx, g, U8 * g.abs() + R.C_F32_ADALN * r["E_dx"])

    # The parameter sums are column sums of products of the kernel's bf16 outputs.  Per output element, with
    # u = 2^-8 and each factor p = exact (1 + d), |d| <= u, plus its fp32 term cf E_p:
    #   |rnd(p) rnd(q) - p q| <= (2 u + u^2) |p q| + (1 + u)^2 cf (E_p |q| + |p| E_q)   (second order in cf dropped
    #   into the (1 + u)^2), summed over the rows of the sum, plus colsum's own fp32 accumulation (test_colsum's
    #   bound) on the sum of |terms| (1 + u)^2.  dy and 1 are exact factors (d = 0, E = 0).
    M, cf, u = rows, R.C_F32_ADALN, U8
    acc = 2.0 ** -24 * (256 + 1 + 2) * (1 + u) ** 2  # one 256-row stripe

    def sums(t, ntok, tl):
        return R.colsum_ref(t, None, ntok, tl)[0]
    dn, xh, n, dy64 = r["dn"].abs(), r["xhat"].abs(), r["n"].abs(), c["dy"].double().view(rows, D).abs()
    dw = K.colsum(dn_out.view(M, D), xh_out.view(M, D))[0, 0]
    a_w = sums((2 * u + u * u) * dn * xh + (1 + u) ** 2 * cf * (r["E_dn"] * xh + dn * r["E_xhat"]) + acc * dn * xh, M, 0)
    check("adaln_bwd D = 3072 dln_w = colsum(dn_out, xhat_out) against autograd", dw, w.grad, a_w[0, 0])
    db = K.colsum(dn_out.view(M, D))[0, 0]
    a_b = sums(u * dn + cf * r["E_dn"] + acc * dn, M, 0)
    check("adaln_bwd D = 3072 dln_b = colsum(dn_out) against autograd", db, b.grad, a_b[0, 0])
    dsc = K.colsum(d["dy"].view(M, D), n_out.view(M, D), tokens_per_batch=N, text_len=T)  # [B, 2, D]
    a_s = sums(dy64 * (u * n + cf * r["E_n"]) + acc * dy64 * n, N, T)
    check("adaln_bwd D = 3072 dscale = colsum(dy, n_out) per (batch, text / video) against autograd", dsc,
          sums(s1.grad, N, T), a_s)


def test_backward_argument_checks(K):
    """sizes and strides the kernels cannot take are refused on the host, before any launch"""
    def adaln(D, mod_stride=None):
        t = torch.zeros(2, 3, D, device=dev, dtype=BF)
        mod = torch.zeros(2, (mod_stride or 6 * D), device=dev, dtype=BF)
        p = torch.zeros(D, device=dev, dtype=BF)
        K.adaln_bwd(t, t.clone(), t.clone(), 1, p, p, 1e-5, mod[:, :6 * D])
    adaln(8)
    adaln(8, 6 * 8 + 64)
    for bad in ((4104, None), (12, None), (8, 6 * 8 + 4), (384, 6 * 384 + 1)):
        with pytest.raises(RuntimeError, match="VP_ERR_ARG"):
            adaln(*bad)
    x = torch.zeros(6, 16, device=dev, dtype=BF)
    mod = torch.zeros(2, 6 * 16 + 4, device=dev, dtype=BF)
    with pytest.raises(RuntimeError, match="VP_ERR_ARG"):
        K.rowscale(x, torch.empty_like(x), 3, 1, mod[:, :96], 2, 5)
    ln = SimpleNamespace(weight=torch.ones(64, device=dev, dtype=BF), bias=torch.zeros(64, device=dev, dtype=BF), eps=1e-6)
    flat = torch.zeros(4096, device=dev, dtype=BF)
    good = torch.as_strided(flat, (2, 3, 64), (3 * 128 + 4, 128, 1))
    bad = torch.as_strided(flat, (2, 3, 64), (3 * 128 + 2, 128, 1))  # row stride % 4 == 0, batch stride not
    K.head_norm_rope_bwd(good, good.clone(), torch.empty(2, 3, 64, device=dev, dtype=BF), 1, 3, ln)
    for args in ((bad, good, good), (good, bad, good), (good, good, bad)):
        with pytest.raises(RuntimeError, match="VP_ERR_ARG"):
            K.head_norm_rope_bwd(*args, 1, 3, ln)


@pytest.mark.parametrize("D", R.ADALN_DS)
def test_adaln_modulate_edges(K, D):
    B, N = R.ADALN_B, R.ADALN_N
    rows = B * N
    c = R.adaln_case(D, 64)
    d = {k: v.to(dev) for k, v in c.items()}
    for T in R.ADALN_TEXT:
        r = R.adaln_modulate_ref(c["x"], c["mod"], c["lw"], c["lb"], R.EPS_ADALN, T)
        buf, out = guarded((B, N), D, rows)
        K.adaln_modulate(d["x"], d["lw"], d["lb"], d["mod"], T, R.EPS_ADALN, out=out)
        check(f"adaln_modulate D = {D} T = {T}", out, r["y"], U8 * r["mag"] + R.C_F32_ADALN * r["E"])
        assert tail_intact(buf, rows)


@pytest.mark.parametrize("T", [0, 5])
@pytest.mark.parametrize("D", R.FINAL_DS)
def test_final_norm_edges(K, D, T):
    B, N = R.ADALN_B, R.ADALN_N
    c = R.adaln_case(D)
    d = {k: v.to(dev) for k, v in c.items()}
    rows = B * (N - T)
    mod2 = d["mod"][:, :2 * D]  # [B, 2 D] = shift | scale, at the row stride of the [B, 6 D] buffer
    a = (c["x"], T, c["lw"], c["lb"], c["lw2"], c["lb2"], R.EPS_ADALN, c["mod"][:, :2 * D])
    buf, out = guarded((B, N - T), D, rows)
    K.final_norm(d["x"], T, d["lw"], d["lb"], d["lw2"], d["lb2"], R.EPS_ADALN, mod2, out=out)
    r = R.final_norm_ref(*a)
    check(f"final_norm D = {D} T = {T}", out, r["y"], U8 * r["mag"] + R.C_F32_ADALN * r["E"])
    assert tail_intact(buf, rows)


# ------------------------------------------------------------------------------------------------------------------
# g. per-head LayerNorm(64) + RoPE backward on the fused-buffer views of its caller
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,T,kind", R.HEAD_CASES)
def test_head_norm_rope_bwd(K, H, T, kind):
    c = R.head_case(H, T, kind)
    B, N = R.HEAD_B, c["N"]
    nvec = B * N * H
    n_blocks = (nvec + 63) // 64
    assert nvec % 64 != 0
    ln = SimpleNamespace(weight=c["lw"].to(dev), bias=c["lb"].to(dev), eps=R.HEAD_EPS)
    rope_d = None
    if c["rope"] is not None:
        cos_d, sin_d = (t.to(dev) for t in c["rope"])
        rope_d = (cos_d[:c["rope_rows"]], sin_d[:c["rope_rows"]])
    qkv_d, dqkv_d = c["qkv"].to(dev), c["dqkv"].to(dev)
    g = torch.Generator().manual_seed(7000 + H + T)
    for which in (0, 1):  # the q and the k slice of the fused [B, N, 3 H 64] buffers
        sl = slice(which * H * 64, (which + 1) * H * 64)
        x_ref, dy_ref, rope_ref = R.head_operands(c, H, which)
        r = R.head_norm_rope_bwd_ref(x_ref, dy_ref, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope_ref)
        tag = f"head_norm_rope_bwd H = {H} T = {T} {kind} {'qk'[which]}"
        x_in, dy = qkv_d[..., sl], dqkv_d[..., sl]
        # 1: dx a slice of a fresh fused buffer of sentinels, no affine sums
        o1 = torch.full_like(dqkv_d, SENT)
        K.head_norm_rope_bwd(x_in, dy, o1[..., sl], H, T, ln, rope_d, None)
        check(tag + " dx", o1[..., sl], r["dx"], U8 * r["dx"].abs() + R.C_F32_HEAD * r["E"])
        keep = torch.ones(3 * H * 64, dtype=torch.bool)
        keep[sl] = False
        assert bool((o1[..., keep.to(dev)] == SENT).all())
        assert not r["dx"][1, 2].isnan().any()  # the zero row (LN(0)): rstd = eps^-1/2
        # 2: with the sums, into zeros: dx the same bits
        dw, db = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
        o2 = torch.empty(B, N, H * 64, device=dev, dtype=BF)
        K.head_norm_rope_bwd(x_in, dy, o2, H, T, ln, rope_d, (dw, db))
        assert _same_bits(o2.cpu(), o1[..., sl].cpu())
        bw = 2.0 ** -24 * (72 + n_blocks)
        check(tag + " dln_w", dw, r["dlw"], bw * r["S_w"])
        check(tag + " dln_b", db, r["dlb"], bw * r["S_b"])
        # 3: dx written over dy in place (the caller's form), the sums accumulated onto non-zero values
        dq = dqkv_d.clone()
        w0, b0 = torch.randn(64, generator=g) * 5, torch.randn(64, generator=g) * 5
        dw, db = w0.clone().to(dev), b0.clone().to(dev)
        K.head_norm_rope_bwd(x_in, dq[..., sl], dq[..., sl], H, T, ln, rope_d, (dw, db))
        assert _same_bits(dq[..., sl].cpu(), o1[..., sl].cpu()), "in place must give the same bits"
        assert torch.equal(dq[..., keep.to(dev)], dqkv_d[..., keep.to(dev)])
        check(tag + " dln_w +=", dw, r["dlw"] + w0.double(), bw * r["S_w"] + 2.0 ** -24 * w0.double().abs())
        check(tag + " dln_b +=", db, r["dlb"] + b0.double(), bw * r["S_b"] + 2.0 ** -24 * b0.double().abs())
