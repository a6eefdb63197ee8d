"""The fp8 attention's two-segment form (ABI 24, GPU only): a second key segment with a per-row length and extra row
mass in the default kernel (variant 5, persistent and one workgroup per block), and its operand producers — the
masked / permuted e4m3 qk-norm and the V^T pack with a per-row length.

The loop has 64-key tiles, two tiles per superstep, a 3-slot ring (it wraps after 6 tiles) and 256-query blocks; the
shapes are the smallest that reach each of its paths.  Band against fp64: the 4e-2 of tests/test_attention_fp8_gpu.py
(the P rounding of this kernel); l_extra is exact mass next to the linearly coded P, whose summed bias a CPU
simulation of the codes puts at 1.4e-4, so the band is the same with and without it."""
import ctypes as C

import pytest
import torch

from tests.test_attention_fp8_gpu import _attn_case, _rope, e4m3, f8, rel, tile_key

pytestmark = pytest.mark.gpu
dev = "cuda"
Q_EXP, K_EXP = 5, 4


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videopainter_amd import _native
    _native.lib()


def _quant(q, k):
    from videopainter_amd import kernels as K
    return (e4m3(q.float() * 0.125 * K.LOG2E * 2.0 ** Q_EXP).to(dev), e4m3(k.float() * 2.0 ** K_EXP).to(dev))


def _unpack_v(vp, B, H):
    """The dequantised V of a pack, fp64 [B, H, npad, 64] (the unpacking of test_attention_fp8_gpu._ref_fp64)."""
    npad = vp.npad
    nt = npad // 64
    vtd = f8(vp.vt).view(B, H, 64, nt * 2, 32)
    sc = vp.vs.cpu().view(B, H, nt, 2, 32, 2).double()
    e = sc.permute(0, 1, 5, 4, 2, 3).reshape(B, H, 64, nt * 2) - 127
    vtd = (vtd * 2.0 ** e[..., None]).view(B, H, 64, npad)
    perm = torch.tensor([tile_key(k) for k in range(64)])
    keys = (torch.arange(nt)[:, None] * 64 + perm[None, :]).reshape(-1)
    vd = torch.zeros(B, H, npad, 64, dtype=torch.float64)
    vd[:, :, keys] = vtd.transpose(2, 3)
    return vd


def _ref2(q8, k8, vp, k2, vp2, lens, lx, H):
    """fp64 attention over the dequantised operands of both packs; denominator sum p + 2^l_extra."""
    B, Nq, _ = q8.shape
    qd = f8(q8).view(B, Nq, H, 64) * 2.0 ** -Q_EXP
    kd = f8(k8).view(B, -1, H, 64) * 2.0 ** -K_EXP
    k2d = f8(k2).view(B, -1, H, 64) * 2.0 ** -K_EXP
    v1, v2 = _unpack_v(vp, B, H), _unpack_v(vp2, B, H)
    out = torch.empty(B, Nq, H, 64, dtype=torch.float64)
    for b in range(B):
        n2 = min(int(lens[b]), k2d.shape[1])
        kk = torch.cat([kd[b], k2d[b, :n2]], dim=0)                       # [Nk, H, 64]
        vv = torch.cat([v1[b, :, :kd.shape[1]], v2[b, :, :n2]], dim=1)    # [H, Nk, 64]
        s = torch.einsum("qhd,khd->hqk", qd[b], kk)
        m = s.amax(dim=-1, keepdim=True)
        ex = torch.zeros_like(m)
        if lx is not None:
            l = lx[b].double().cpu()[..., None]
            m = torch.maximum(m, torch.where(torch.isinf(l), m, l))
            ex = torch.exp2(l - m)
        p = torch.exp2(s - m)
        out[b] = torch.einsum("hqk,hkd->qhd", p / (p.sum(dim=-1, keepdim=True) + ex), vv)
    return out.reshape(B, Nq, H * 64)


def _l_extra(q8, H, seed, n_null=300):
    """log2 of the summed exp2 scores of n_null synthetic null keys per query (fp64 from the dequantised q), with a
    scattering of -inf entries: fp32 [B, H, Nq]."""
    B, Nq, _ = q8.shape
    g = torch.Generator().manual_seed(seed)
    qd = f8(q8).view(B, Nq, H, 64) * 2.0 ** -Q_EXP
    nk = torch.randn(H, n_null, 64, generator=g, dtype=torch.float64)
    lx = torch.log2(torch.exp2(torch.einsum("bqhd,hkd->bhqk", qd, nk)).sum(dim=-1))
    lx[torch.rand(B, H, Nq, generator=g) < 0.1] = float("-inf")
    return lx.float().contiguous().to(dev)


def _case2(B, H, N1, Nk2, seed, spike2=None):
    """(q8, k8, vp, k2_8, v2 bf16 on the device) from _attn_case's distributions; spike2: a segment-2 row aligned
    with every query (the running max jumps inside segment 2)."""
    from videopainter_amd import kernels as K
    q, k, v = _attn_case(B, H, N1, seed)
    _, k2, v2 = _attn_case(B, H, Nk2, seed + 7)
    if spike2 is not None:
        k2[:, spike2] = (q.float().mean(dim=1) * 6).to(torch.bfloat16)
    q8, k8 = _quant(q, k)
    _, k2_8 = _quant(q[:, :1], k2)
    return q8, k8, K.v_pack_fp8(v.to(dev), H), k2_8, v2.to(dev)


def _lens(vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


def _eq(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


CASES = [(2, 3, 300, 300, [200, 37], None), (1, 2, 40, 64, [64], None), (2, 1, 130, 130, [1, 65], None),
         (1, 2, 64, 200, [63], None), (2, 2, 300, 300, [0, 300], None),
         (1, 2, 2000, 2000, [1500], 1400)]  # the late-spike key sits inside segment 2


@pytest.mark.parametrize("with_lx", [False, True], ids=["nolx", "lx"])
@pytest.mark.parametrize("B,H,N1,Nk2,lens,spike", CASES)
def test_two_segments_against_fp64(B, H, N1, Nk2, lens, spike, with_lx):
    from videopainter_amd import kernels as K
    q8, k8, vp, k2, v2 = _case2(B, H, N1, Nk2, 100 + N1 + Nk2 + lens[0], spike)
    ln = _lens(lens)
    vp2 = K.v_pack_fp8(v2, H, lens=ln)
    lx = _l_extra(q8, H, N1) if with_lx else None
    out = torch.empty(B, N1, H * 64, device=dev, dtype=torch.bfloat16)
    K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, k2=k2, vp2=vp2, k2_len=ln, l_extra=lx)
    # the reference unpacks a pack made without lens from zeroed rows (every tile written)
    v2z = v2.clone()
    for b in range(B):
        v2z[b, lens[b]:] = 0
    ref = _ref2(q8, k8, vp, k2, K.v_pack_fp8(v2z, H), lens, lx, H)
    r = rel(out, ref)
    print(f"fp8 two-segment B={B} H={H} N1={N1} Nk2={Nk2} k2_len={lens} l_extra={with_lx}: rel vs fp64 {r:.3e}")
    assert torch.isfinite(out.float()).all()
    assert r < 4e-2


def test_two_segments_blend_epilogue():
    from videopainter_amd import kernels as K
    B, H, N1, Nk2, lens = 2, 3, 300, 300, [200, 37]
    q8, k8, vp, k2, v2 = _case2(B, H, N1, Nk2, 11)
    ln = _lens(lens)
    vp2 = K.v_pack_fp8(v2, H, lens=ln)
    lx = _l_extra(q8, H, 5)
    kw = dict(k2=k2, vp2=vp2, k2_len=ln, l_extra=lx)
    out = torch.empty(B, N1, H * 64, device=dev, dtype=torch.bfloat16)
    K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, **kw)
    o2 = torch.empty_like(out)
    K.attention_fp8(q8, k8, vp, o2, H, Q_EXP, K_EXP, out_scale=0.7, **kw)
    K.attention_fp8(q8, k8, vp, o2, H, Q_EXP, K_EXP, out_scale=0.3, accumulate=True, **kw)
    assert rel(o2, out) < 1e-2


@pytest.mark.parametrize("lx_kind", ["none", "neginf"])
def test_zero_length_equals_single_segment(lx_kind):
    """(a) k2_len = 0 everywhere, l_extra None or all -inf: the single-segment call, bit for bit."""
    from videopainter_amd import kernels as K
    B, H, N1, Nk2 = 2, 3, 300, 130
    q8, k8, vp, k2, v2 = _case2(B, H, N1, Nk2, 21)
    ln = _lens([0, 0])
    vp2 = K.v_pack_fp8(v2, H, lens=ln)
    lx = None if lx_kind == "none" else torch.full((B, H, N1), float("-inf"), device=dev)
    one, two = (torch.empty(B, N1, H * 64, device=dev, dtype=torch.bfloat16) for _ in range(2))
    K.attention_fp8(q8, k8, vp, one, H, Q_EXP, K_EXP)
    K.attention_fp8(q8, k8, vp, two, H, Q_EXP, K_EXP, k2=k2, vp2=vp2, k2_len=ln, l_extra=lx)
    assert _eq(one, two)


@pytest.mark.parametrize("N", [300, 1000])
@pytest.mark.parametrize("a", [64, 192])
def test_split_equals_one_segment(a, N):
    """(b) K[0:N] as one segment equals K[:a] | K[a:]: the same tiles in the same order (a is a multiple of 64, so
    the 32-key scale blocks do not straddle the cut), also through the blend epilogue."""
    from videopainter_amd import kernels as K
    B, H = 2, 3
    q, k, v = _attn_case(B, H, N, 3000 + N + a, late_spike=N >= 1000)
    q8, k8 = _quant(q, k)
    vd = v.to(dev)
    vp = K.v_pack_fp8(vd, H)
    vpa, vpb = K.v_pack_fp8(vd[:, :a], H), K.v_pack_fp8(vd[:, a:], H)
    one, two = (torch.empty(B, N, H * 64, device=dev, dtype=torch.bfloat16) for _ in range(2))
    K.attention_fp8(q8, k8, vp, one, H, Q_EXP, K_EXP)
    K.attention_fp8(q8, k8[:, :a], vpa, two, H, Q_EXP, K_EXP, k2=k8[:, a:], vp2=vpb)
    assert _eq(one, two)
    K.attention_fp8(q8, k8, vp, one, H, Q_EXP, K_EXP, out_scale=0.7)
    K.attention_fp8(q8, k8, vp, one, H, Q_EXP, K_EXP, out_scale=0.3, accumulate=True)
    K.attention_fp8(q8, k8[:, :a], vpa, two, H, Q_EXP, K_EXP, out_scale=0.7, k2=k8[:, a:], vp2=vpb)
    K.attention_fp8(q8, k8[:, :a], vpa, two, H, Q_EXP, K_EXP, out_scale=0.3, accumulate=True, k2=k8[:, a:], vp2=vpb)
    assert _eq(one, two)


def test_garbage_past_the_length_is_not_read():
    """(c) K2 rows >= k2_len[b] of byte 0x7F (the e4m3 NaN) and bf16 V2 rows of NaN: the output of the same call with
    those rows zero, and finite."""
    from videopainter_amd import kernels as K
    B, H, N1, Nk2, lens = 2, 3, 300, 300, [200, 37]
    q8, k8, vp, k2, v2 = _case2(B, H, N1, Nk2, 31)
    ln = _lens(lens)
    lx = _l_extra(q8, H, 6)
    k2g, v2g, k2z, v2z = k2.clone(), v2.clone(), k2.clone(), v2.clone()
    for b in range(B):
        k2g[b, lens[b]:] = 0x7F
        v2g[b, lens[b]:] = float("nan")
        k2z[b, lens[b]:] = 0
        v2z[b, lens[b]:] = 0
    og, oz = (torch.empty(B, N1, H * 64, device=dev, dtype=torch.bfloat16) for _ in range(2))
    K.attention_fp8(q8, k8, vp, og, H, Q_EXP, K_EXP, k2=k2g, vp2=K.v_pack_fp8(v2g, H, lens=ln), k2_len=ln, l_extra=lx)
    K.attention_fp8(q8, k8, vp, oz, H, Q_EXP, K_EXP, k2=k2z, vp2=K.v_pack_fp8(v2z, H), k2_len=ln, l_extra=lx)
    assert torch.isfinite(og.float()).all()
    assert _eq(og, oz)


def test_length_past_nk2_behaves_as_nk2():
    """(d) k2_len[b] > Nk2 is Nk2 (and NULL k2_len is Nk2 for every row)."""
    from videopainter_amd import kernels as K
    B, H, N1, Nk2 = 2, 2, 130, 200
    q8, k8, vp, k2, v2 = _case2(B, H, N1, Nk2, 41)
    vp2 = K.v_pack_fp8(v2, H)
    outs = []
    for ln in (None, _lens([Nk2, Nk2]), _lens([Nk2 + 1, 1 << 30])):
        o = torch.empty(B, N1, H * 64, device=dev, dtype=torch.bfloat16)
        K.attention_fp8(q8, k8, vp, o, H, Q_EXP, K_EXP, k2=k2, vp2=vp2, k2_len=ln)
        outs.append(o)
    assert _eq(outs[0], outs[1]) and _eq(outs[0], outs[2])


def test_persistent_two_segments_bit_identical(knobs):
    """(e) The persistent two-segment instance against one workgroup per block (VP_ATTN_PERSIST=0)."""
    from videopainter_amd import kernels as K
    from videopainter_amd import _native as N_
    B, H, N, Nk2, lens = 2, 9, 15000, 15000, [7000, 123]
    q8, k8, vp, k2, v2 = _case2(B, H, N, Nk2, 51, spike2=6500)
    ln = _lens(lens)
    vp2 = K.v_pack_fp8(v2, H, lens=ln)
    lx = _l_extra(q8, H, 8, n_null=100)
    dd = N_.AttnFp8Desc()
    dd.base.B, dd.base.H, dd.base.Nq = B, H, N
    assert N_.lib().vp_attention_fp8_workspace_bytes(C.byref(dd)) > 0  # the persistent path is taken
    outs = []
    for persist in ("1", "0"):
        knobs.setenv("VP_ATTN_PERSIST", persist)
        o = torch.empty(B, N, H * 64, device=dev, dtype=torch.bfloat16)
        K.attention_fp8(q8, k8, vp, o, H, Q_EXP, K_EXP, k2=k2, vp2=vp2, k2_len=ln, l_extra=lx)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all()
    assert _eq(outs[0], outs[1])


@pytest.mark.parametrize("Nk,lens", [(300, [200, 37]), (130, [0, 130]), (64, [1, 64])])
def test_v_pack_with_lens_bit_exact(Nk, lens):
    """v_pack_fp8(v, H, lens) against v_pack_fp8 of the same v with rows >= lens zeroed: the vt and vs bytes of every
    tile below ceil(lens[b] / 64); the rows past lens hold NaN and must not be read."""
    from videopainter_amd import kernels as K
    B, H = 2, 3
    g = torch.Generator().manual_seed(Nk)
    v = (torch.randn(B, Nk, H * 64, generator=g) * 10.0 ** torch.empty(B, Nk, 1).uniform_(-2, 2, generator=g))
    v = v.to(torch.bfloat16).to(dev)
    vg, vz = v.clone(), v.clone()
    for b in range(B):
        vg[b, lens[b]:] = float("nan")
        vz[b, lens[b]:] = 0
    got, want = K.v_pack_fp8(vg, H, lens=_lens(lens)), K.v_pack_fp8(vz, H)
    assert got.npad == want.npad and got.n == want.n
    nt = got.npad // 64
    for b in range(B):
        t = (lens[b] + 63) // 64
        assert torch.equal(got.vt.view(B, H, 64, got.npad)[b, :, :, :t * 64],
                           want.vt.view(B, H, 64, got.npad)[b, :, :, :t * 64])
        assert torch.equal(got.vs.view(B, H, nt, 128)[b, :, :t], want.vs.view(B, H, nt, 128)[b, :, :t])


@pytest.mark.parametrize("pre_scale", [1.0, 0.5])
def test_masked_permuted_fp8_norm_bit_exact(pre_scale):
    """The masked / permuted fp8 norm against e4m3(the bf16 kernel with the same tok_mask, pre_scale, dst_rows x mul);
    rows whose dst_rows entry is negative leave a pre-filled sentinel untouched."""
    from videopainter_amd import kernels as K
    B, T, Nv, H = 2, 5, 70, 4
    N = T + Nv
    g = torch.Generator().manual_seed(13)
    x = (torch.randn(B, N, 3 * H * 64, generator=g) * 2 + 0.5).to(torch.bfloat16).to(dev)
    lw = (1 + 0.2 * torch.randn(64, generator=g)).to(torch.bfloat16).to(dev)
    lb = (0.2 * torch.randn(64, generator=g)).to(torch.bfloat16).to(dev)
    rope = _rope(Nv, 2)
    m = (torch.rand(B, N, generator=g) < 0.5).to(torch.uint8).to(dev)
    dst, cnt = K.partition_rows_index(m)
    dst = torch.where(m.bool(), dst, torch.full_like(dst, -1))
    kx = x[..., H * 64:2 * H * 64]
    ref = torch.full((B, N, H * 64), 7.0, device=dev, dtype=torch.bfloat16)
    K.head_norm_rope(kx, ref, H, T, lw, lb, 1e-6, rope, tok_mask=m, pre_scale=pre_scale, dst_rows=dst)
    mul = 2.0 ** K.qk_fp8_exponent(lw, lb)
    out = torch.full((B, N, H * 64), 0xAB, device=dev, dtype=torch.uint8)
    got = K.head_norm_rope_fp8(kx, H, T, lw, lb, 1e-6, rope, mul, out=out, tok_mask=m, pre_scale=pre_scale,
                               dst_rows=dst)
    assert got is out
    cnt = cnt.cpu()
    assert 0 < int(cnt.min()) and int(cnt.max()) < N
    for b in range(B):
        c = int(cnt[b])
        assert float(ref[b, :c].float().abs().max()) * mul <= 448
        assert torch.equal(out[b, :c].cpu(), e4m3(ref[b, :c].float().cpu() * mul))
        assert bool((out[b, c:] == 0xAB).all()) and bool((ref[b, c:] == 7.0).all())
    # without a mask or a permutation: the plain entry's bytes
    plain = K.head_norm_rope_fp8(kx, H, T, lw, lb, 1e-6, rope, mul)
    ident = torch.arange(N, dtype=torch.int32, device=dev).expand(B, N).contiguous()
    assert torch.equal(plain, K.head_norm_rope_fp8(kx, H, T, lw, lb, 1e-6, rope, mul, dst_rows=ident))


def test_rejections(knobs):
    """k2_full on the fp8 entry and a second segment / l_extra under variants 2 and 3 are refused before any launch;
    a valid call afterwards still runs."""
    from videopainter_amd import kernels as K
    from videopainter_amd import _native as N_
    B, H, N1, Nk2 = 1, 2, 130, 130
    q8, k8, vp, k2, v2 = _case2(B, H, N1, Nk2, 61)
    ln = _lens([65])
    vp2 = K.v_pack_fp8(v2, H, lens=ln)
    out = torch.empty(B, N1, H * 64, device=dev, dtype=torch.bfloat16)
    for var in ("2", "3"):
        if not K.attention_variant_built("fp8:" + var):
            continue
        knobs.setenv("VP_ATTN8_VARIANT", var)
        with pytest.raises(ValueError, match="two-segment"):
            K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, k2=k2, vp2=vp2, k2_len=ln)
        with pytest.raises(ValueError, match="two-segment"):
            K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, l_extra=torch.zeros(B, H, N1, device=dev))
    knobs.setenv("VP_ATTN8_VARIANT", "5")
    with pytest.raises(ValueError):
        K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, k2=k2)                   # k2 without vp2
    with pytest.raises(ValueError):
        K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, k2_len=ln)               # k2_len without a segment
    with pytest.raises(ValueError):
        K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, k2=k2[:, :100], vp2=vp2)  # pack of another length
    # k2_full: a descriptor field the Python entry does not offer — the C entry refuses it
    dd = N_.AttnFp8Desc()
    d = dd.base
    d.B, d.H, d.Nq, d.head_dim = B, H, N1, 64
    d.Q, d.q_sb, d.q_sn = q8.data_ptr(), q8.stride(0), q8.stride(1)
    d.K, d.k_sb, d.k_sn, d.Nk = k8.data_ptr(), k8.stride(0), k8.stride(1), N1
    d.V, d.O, d.o_sb, d.o_sn = vp.vt.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1)
    d.K2, d.k2_sb, d.k2_sn, d.Nk2, d.V2 = k2.data_ptr(), k2.stride(0), k2.stride(1), Nk2, vp2.vt.data_ptr()
    d.scale, d.out_scale = 1.0, 1.0
    dd.vs, dd.npad, dd.vs2, dd.npad2 = vp.vs.data_ptr(), vp.npad, vp2.vs.data_ptr(), vp2.npad
    dd.qk_scale = (127 - Q_EXP) | ((127 - K_EXP) << 8)
    d.k2_full = ln.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    assert N_.lib().vp_attention_fwd_fp8_ws(C.byref(dd), None, 0, stream) == N_.ERR_UNSUPPORTED
    d.k2_full = None
    d.k2_len = ln.data_ptr()
    o2 = torch.empty_like(out)
    d.O = o2.data_ptr()
    assert N_.lib().vp_attention_fwd_fp8_ws(C.byref(dd), None, 0, stream) == 0     # the same descriptor without it
    K.attention_fp8(q8, k8, vp, out, H, Q_EXP, K_EXP, k2=k2, vp2=vp2, k2_len=ln)
    torch.cuda.synchronize()
    assert _eq(out, o2) and torch.isfinite(out.float()).all()
