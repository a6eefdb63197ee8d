"""The references of tests/backward_refs.py checked against torch.autograd / one-line torch forms in float64 on the
CPU, and the measurement of the c_f32 constants the GPU tolerances use.  No tolerance of
tests/test_backward_kernels_gpu.py depends on the code under test: it depends on these functions, which are checked
here."""
import pytest
import torch
import torch.nn.functional as F

from tests import backward_refs as R

F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, rtol=1e-10):
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= rtol * scale, (float((a - b).abs().max()), scale)


def test_rnd_bf16_is_the_single_rounding():
    # 1 + 2^-8 + 2^-30 lies just above the tie between 1 and 1 + 2^-7: fp32 rounds it onto the tie (-> even = 1)
    x = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -30, -(1 + 2.0 ** -8 + 2.0 ** -30),
                      3 * 2.0 ** -8 + 1 - 2.0 ** -30], dtype=F64)
    want = torch.tensor([1 + 2.0 ** -7, 1.0, 1.0, -(1 + 2.0 ** -7), 1 + 2.0 ** -7], dtype=F64)
    assert torch.equal(R.rnd_bf16(x), want)
    a = torch.tensor([1.0, -1.0, 1.0, 2.0 ** -133]).bfloat16()
    b = torch.tensor([1 + 2.0 ** -7, -1.0, -2.0 ** -133, 0.0]).bfloat16()
    assert R.bf16_ulps(a, b).tolist() == [1, 0, 0x3F80 + 1, 1]


def test_elementwise_and_sum_refs_match_their_torch_forms():
    g = _g(1)
    x = torch.randn(3, 7, 10, generator=g, dtype=F64)
    t = R.transpose_ref(x, pad_to=8)
    assert t.shape == (10, 24) and torch.equal(t[:, :21], x.reshape(21, 10).t()) and not t[:, 21:].any()
    a, b = torch.randn(24, 16, generator=g, dtype=F64), torch.randn(24, 16, generator=g, dtype=F64)
    for bb in (b, None):
        s, sa = R.colsum_ref(a, bb, 8, 3)
        p = (a if bb is None else a * b).view(3, 8, 16)
        _close(s, torch.stack((p[:, 3:].sum(1), p[:, :3].sum(1)), 1), 1e-14)
        _close(sa, torch.stack((p[:, 3:].abs().sum(1), p[:, :3].abs().sum(1)), 1), 1e-14)
    s, _ = R.colsum_ref(a, None, 8, 0)
    assert not s[:, 1].any()
    s, _ = R.colsum_ref(a, None, 8, 8)
    assert not s[:, 0].any()
    mod = torch.randn(3, 6 * 16 + 8, generator=g, dtype=F64)
    y = R.rowscale_ref(a, mod, 8, 3, 2, 5)
    m = mod[:, :96].view(3, 6, 16)
    want = a.view(3, 8, 16) * torch.cat((m[:, 5:6].expand(3, 3, 16), m[:, 2:3].expand(3, 5, 16)), 1)
    assert torch.equal(y, want.view(24, 16))
    assert torch.equal(R.axpy_ref(a, b, -0.5), a - 0.5 * b)


def test_gelu_and_silu_refs_match_autograd():
    z = torch.linspace(-6, 6, 4001, dtype=F64).requires_grad_()
    dh = torch.randn(4001, generator=_g(2), dtype=F64)
    for fwd, ref, bwd in ((lambda t: F.gelu(t, approximate="tanh"), R.gelu_ref, R.gelu_bwd_ref),
                          (F.silu, R.silu_ref, R.silu_bwd_ref)):
        z.grad = None
        y = fwd(z)
        y.backward(dh)
        # absolute in units of the largest value: F.gelu's own 1 + tanh cancels on the negative side
        _close(ref(z), y.detach(), 1e-15)
        _close(bwd(dh, z), z.grad, 1e-14)
    # the negative tail, where the textbook form has no relative accuracy left: against the asymptote
    # gelu'(z) -> exp(2 u) (1 + 2 z u'),  silu'(z) -> exp(z) (1 + z)
    zt = torch.tensor([-7.0, -8.5, -9.75], dtype=F64)
    u = R.K0 * (zt + R.K1 * zt ** 3)
    up = R.K0 * (1 + 3 * R.K1 * zt ** 2)
    one = torch.ones_like(zt)
    assert float(((R.gelu_bwd_ref(one, zt) / (torch.exp(2 * u) * (1 + 2 * zt * up))) - 1).abs().max()) < 1e-12
    zs = torch.tensor([-40.0, -60.0, -90.0], dtype=F64)
    assert float(((R.silu_bwd_ref(torch.ones(3, dtype=F64), zs) / (torch.exp(zs) * (1 + zs))) - 1).abs().max()) < 1e-12
    # saturation of the references themselves at the largest finite bf16
    big = torch.tensor([3.3895e38, -3.3895e38], dtype=F64)
    for f in (R.gelu_ref, R.silu_ref):
        assert f(big).tolist() == [3.3895e38, -0.0]
    for f in (R.gelu_bwd_ref, R.silu_bwd_ref):
        assert f(torch.full((2,), 3.0, dtype=F64), big).abs().tolist() == [3.0, 0.0]


@pytest.mark.parametrize("chunks", R.ADALN_CHUNKS)
@pytest.mark.parametrize("T", (0, 3, 7))
def test_adaln_refs_match_autograd(T, chunks):
    g = _g(3)
    B, N, D = 2, 7, 24
    x = (torch.randn(B, N, D, generator=g, dtype=F64) * 3 + 1).requires_grad_()
    dy = torch.randn(B, N, D, generator=g, dtype=F64)
    w = (1 + 0.1 * torch.randn(D, generator=g, dtype=F64)).requires_grad_()
    b = (0.1 * torch.randn(D, generator=g, dtype=F64)).requires_grad_()
    mod = torch.randn(B, 6 * D + 8, generator=g, dtype=F64)
    s1, shift = R.adaln_s1_shift(mod, D, N, T, chunks, B * N)
    s1.requires_grad_()
    xhat = F.layer_norm(x, (D,), None, None, 1e-5).view(B * N, D)
    n = F.layer_norm(x, (D,), w, b, 1e-5).view(B * N, D)
    y = n * s1 + shift
    y.backward(dy.view(B * N, D))
    r = R.adaln_bwd_ref(x, dy, mod, w, b, 1e-5, T, chunks)
    _close(r["delta"], x.grad.view(B * N, D))
    _close(r["n"], n.detach())
    _close(r["xhat"], xhat.detach())
    _close(r["dn"], dy.view(B * N, D) * s1.detach())
    _close(dy.view(B * N, D) * r["n"], s1.grad)  # the scale gradient's terms
    _close(R.colsum_ref(r["dn"], r["xhat"], B * N, 0)[0][0, 0], w.grad)
    _close(R.colsum_ref(r["dn"], None, B * N, 0)[0][0, 0], b.grad)
    assert bool((r["E_dx"] >= r["delta"].abs() * (1 - 1e-12)).all()) and bool((r["E_n"] >= r["n"].abs() * (1 - 1e-12)).all())
    # the forward twin: the unrounded chain is the same graph
    f = R.adaln_modulate_ref(x, mod, w, b, 1e-5, T) if chunks == (0, 1, 3, 4) else None
    if f is not None:
        _close(f["y"], y.detach())
        assert bool((f["mag"] > 0).all()) and bool((f["E"] >= f["y"].abs() * (1 - 1e-12)).all())


def test_final_norm_ref_is_the_two_layer_norms():
    g = _g(4)
    B, N, D, T = 2, 6, 24, 2
    x = torch.randn(B, N, D, generator=g, dtype=F64) * 2
    w1, b1, w2, b2 = (torch.randn(D, generator=g, dtype=F64) * 0.2 + a for a in (1, 0, 1, 0))
    mod = torch.randn(B, 2 * D, generator=g, dtype=F64)
    r = R.final_norm_ref(x, T, w1, b1, w2, b2, 1e-5, mod)
    n1 = F.layer_norm(x[:, T:], (D,), w1, b1, 1e-5)
    _close(r["n1_exact"], n1.reshape(-1, D))
    n2 = F.layer_norm(R.rnd_bf16(n1), (D,), w2, b2, 1e-5)
    y = n2 * R.rnd_bf16(1 + mod[:, None, D:]) + mod[:, None, :D]
    _close(r["y"], y.reshape(-1, D))
    assert torch.equal(r["n1_rounded"], R.rnd_bf16(n1).reshape(-1, D))
    # n1_rounded given: the second norm runs on exactly those values
    other = R.rnd_bf16(n1 * 1.5).reshape(-1, D)
    r2 = R.final_norm_ref(x, T, w1, b1, w2, b2, 1e-5, mod, n1_rounded=other)
    y2 = F.layer_norm(other, (D,), w2, b2, 1e-5) * R.rnd_bf16(1 + mod[:, None, D:]).expand(B, N - T, D).reshape(-1, D) \
        + mod[:, None, :D].expand(B, N - T, D).reshape(-1, D)
    _close(r2["y"], y2)
    _close(r2["n1_exact"], n1.reshape(-1, D))


@pytest.mark.parametrize("T,rope", [(0, True), (3, True), (5, False)])
def test_head_norm_rope_bwd_ref_matches_autograd(T, rope):
    from oracle.cogvideox_oracle import apply_rotary_emb
    g = _g(5)
    cos, sin = (t.double() for t in R.head_rope())
    B, H = 2, 3
    N = T + cos.shape[0] if rope else T
    x = (torch.randn(B, N, H * 64, generator=g, dtype=F64) * 2 + 0.5)
    dy = torch.randn(B, N, H * 64, generator=g, dtype=F64)
    w = (1 + 0.2 * torch.randn(64, generator=g, dtype=F64)).requires_grad_()
    b = (0.1 * torch.randn(64, generator=g, dtype=F64)).requires_grad_()
    xh = x.view(B, N, H, 64).transpose(1, 2).clone().requires_grad_()  # [B, H, N, 64], the oracle's layout
    y = F.layer_norm(xh, (64,), w, b, 1e-6)
    if rope:
        # The oracle's apply_rotary_emb computes in fp32 whatever it is given.  It is linear, and on the 64 unit
        # vectors its fp32 arithmetic is exact (1 * cos, 0 * sin), so its matrix per row is read off exactly and
        # applied in float64: the same function, without the fp32 noise that would hide a 1e-10 error.
        Nv = cos.shape[0]
        eye = torch.eye(64).view(1, 64, 1, 64).expand(1, 64, Nv, 64).contiguous()
        M = apply_rotary_emb(eye, cos.float(), sin.float())[0].permute(1, 2, 0).double()  # [Nv, out, in]
        # and it agrees with the function itself on real data to fp32 accuracy
        probe = y[:, :, T:].detach()
        assert float((torch.einsum("noi,bhni->bhno", M, probe) - apply_rotary_emb(probe, cos, sin)).abs().max()) < 1e-5
        y = torch.cat([y[:, :, :T], torch.einsum("noi,bhni->bhno", M, y[:, :, T:])], 2)
    y.backward(dy.view(B, N, H, 64).transpose(1, 2))
    r = R.head_norm_rope_bwd_ref(x, dy, w, b, 1e-6, H, T, (cos, sin) if rope else None)
    _close(r["dx"], xh.grad.transpose(1, 2).reshape(B, N, H * 64))
    _close(r["dlw"], w.grad)
    _close(r["dlb"], b.grad)
    assert bool((r["E"] >= r["dx"].abs() * (1 - 1e-12)).all())
    assert bool((r["S_w"] >= r["dlw"].abs()).all()) and bool((r["S_b"] >= r["dlb"].abs()).all())


def test_head_cases_leave_a_ragged_last_block():
    for H, T, kind in R.HEAD_CASES:
        c = R.head_case(H, T, kind)
        assert (R.HEAD_B * c["N"] * H) % 64 != 0 and not c["qkv"][1, 2].any()
    assert R.head_rope()[0].shape == (12, 64)


def _f32_ratio(r64, r32, pairs):
    return max(R.worst_ratio((r32[k].double() - r64[k]).abs(), r64[e]) for k, e in pairs)


def measure_c_f32():
    """worst |fp32 - fp64| / E of the reference formulas evaluated in float32 torch, over every GPU case"""
    f32 = torch.float32
    worst_a = 0.0
    for D in R.ADALN_DS:
        c = R.adaln_case(D)
        for T in R.ADALN_TEXT:
            for ch in R.ADALN_CHUNKS:
                a = (c["x"], c["dy"], c["mod"], c["lw"], c["lb"], R.EPS_ADALN, T, ch)
                worst_a = max(worst_a, _f32_ratio(R.adaln_bwd_ref(*a), R.adaln_bwd_ref(*a, dt=f32),
                                                  (("n", "E_n"), ("dn", "E_dn"), ("xhat", "E_xhat"), ("delta", "E_dx"))))
            a = (c["x"], c["mod"], c["lw"], c["lb"], R.EPS_ADALN, T)
            worst_a = max(worst_a, _f32_ratio(R.adaln_modulate_ref(*a), R.adaln_modulate_ref(*a, dt=f32), (("y", "E"),)))
        if D in R.FINAL_DS:
            for T in (0, 5):
                a = (c["x"], T, c["lw"], c["lb"], c["lw2"], c["lb2"], R.EPS_ADALN, c["mod"])
                # the second norm from the float64 evaluation's rounded n1 (bf16 values, exact in float32): what is
                # measured is the fp32 arithmetic of each norm, not a rounding of n1 that fp32 decides the other way
                r64 = R.final_norm_ref(*a)
                r32 = R.final_norm_ref(*a, dt=f32, n1_rounded=r64["n1_rounded"])
                worst_a = max(worst_a, _f32_ratio(r64, r32, (("n1_exact", "E_n1"), ("y", "E"))))
    worst_h = 0.0
    for H, T, kind in R.HEAD_CASES:
        c = R.head_case(H, T, kind)
        for which in (0, 1):
            x, dy, rope = R.head_operands(c, H, which)
            a = (x, dy, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope)
            worst_h = max(worst_h, _f32_ratio(R.head_norm_rope_bwd_ref(*a), R.head_norm_rope_bwd_ref(*a, dt=f32),
                                              (("dx", "E"),)))
    return worst_a, worst_h


def test_c_f32_constants():
    """C_F32_* = 8 x the worst fp32-vs-fp64 error of the reference formulas in units of E (rounded up)."""
    wa, wh = measure_c_f32()
    print(f"c_f32 AdaLN rows: worst |fp32 - fp64| / E = {wa:.3e}, x 8 = {8 * wa:.3e}, constant {R.C_F32_ADALN:.3e}")
    print(f"c_f32 head vectors: worst |fp32 - fp64| / E = {wh:.3e}, x 8 = {8 * wh:.3e}, constant {R.C_F32_HEAD:.3e}")
    assert R.C_F32_ADALN / 2 <= 8 * wa <= R.C_F32_ADALN
    assert R.C_F32_HEAD / 2 <= 8 * wh <= R.C_F32_HEAD


def test_axpy_and_rowscale_fp32_emulation_meets_the_bit_equal_share():
    """The kernels do one fp32 fma (axpy) / one fp32 product (rowscale) and one rounding.  Emulated in fp32 torch on
    the GPU tests' inputs, that is within 1 bf16 ulp of bf16(fp64 form) everywhere and bit-equal on >= 99.9 %."""
    for n in (8, 8 * (256 * 3 + 5)):
        a, b = R.axpy_inputs(n)
        for alpha in (1.0, -0.5):
            emu = (a.float() + alpha * b.float()).bfloat16()  # alpha b is exact for these alphas: one fp32 rounding
            want = R.rnd_bf16(R.axpy_ref(a, b, alpha)).bfloat16()
            u = R.bf16_ulps(emu, want)
            assert int(u.max()) <= 1 and float((u == 0).float().mean()) >= 0.999
    for D in (8, 136):
        x, mod = R.rowscale_inputs(D)
        for T in (0, 5, 37):
            emu = R.rowscale_ref(x, mod, 37, T, 2, 5, dt=torch.float32).bfloat16()
            want = R.rnd_bf16(R.rowscale_ref(x, mod, 37, T, 2, 5)).bfloat16()
            assert torch.equal(emu, want)  # a product of two bf16 is exact in fp32
