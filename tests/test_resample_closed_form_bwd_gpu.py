"""The kernels of the closed-form resample training backward (GPU): the flash backward with a per-batch key length,
the null-key mass backward, the gather-add of the compact second segment's gradients, and the statistics the
two-segment forward writes for them."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videopainter_amd import _native
    _native.lib()


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bf(x):
    return x.to(torch.bfloat16)


def rnd(*shape, std=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


# ---- 1 / 2: vp_attention_bwd_bf16 with k_len ----

def _truncated_forward(q, k, v, klen, H):
    """o [B, Nq, D], lse [B, H, Nq] of the attention of batch row b over its first klen[b] keys (B = 1 launches)."""
    from videopainter_amd import kernels as K
    B, Nq, D = q.shape
    o = torch.empty(B, Nq, D, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, Nq, device=dev, dtype=torch.float32)
    for b, n in enumerate(klen):
        K.attention(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], o[b:b + 1], H, lse=lse[b:b + 1])
    return o, lse


def _nan_grads(B, Nq, Nk, D):
    return [torch.full((B, n, D), float("nan"), device=dev, dtype=torch.bfloat16) for n in (Nq, Nk, Nk)]


def test_attention_bwd_k_len_bits(knobs):
    """Batch row b with k_len[b] keys against the B = 1 launch on the truncated k / v: the same tiles in the same
    order (a partial 64-key tile; a length on a 128-key block boundary with a whole empty block behind it; the full
    length), so the same bits; rows past the length come back zero in NaN-filled buffers; NULL = the full length;
    and the gradients against fp32 autograd over the truncated keys."""
    from videopainter_amd import kernels as K
    knobs.setenv("VP_ATTN_NO_SPLIT", "1")
    B, H, Nq, Nk = 3, 2, 700, 1600
    klen = [1000, 1536, 1600]
    D = H * 64
    q, k, v, do = (bf(rnd(B, n, D, seed=s)).to(dev) for n, s in ((Nq, 1), (Nk, 2), (Nk, 3), (Nq, 4)))
    o, lse = _truncated_forward(q, k, v, klen, H)
    kl = torch.tensor(klen, dtype=torch.int32, device=dev)
    dq, dk, dv = _nan_grads(B, Nq, Nk, D)
    delta = torch.empty(B, H, Nq, device=dev, dtype=torch.float32)
    K.attention_bwd(q, k, v, o, do, lse, H, dq=dq, dk=dk, dv=dv, k_len=kl, delta=delta)
    torch.cuda.synchronize()
    want_delta = (do.float() * o.float()).view(B, Nq, H, 64).sum(-1).transpose(1, 2)
    assert rel(delta, want_delta) < 1e-5
    for b, n in enumerate(klen):
        rq, rk, rv = K.attention_bwd(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], o[b:b + 1], do[b:b + 1],
                                     lse[b:b + 1], H)
        assert torch.equal(dq[b:b + 1], rq), b
        assert torch.equal(dk[b:b + 1, :n], rk), b
        assert torch.equal(dv[b:b + 1, :n], rv), b
        assert not dk[b, n:].float().ne(0).any() and not dv[b, n:].float().ne(0).any(), b
        assert not torch.isnan(dk[b, n:].float()).any() and not torch.isnan(dv[b, n:].float()).any(), b
        # fp32 autograd over the truncated keys (the rule of test_backward_gpu.py)
        qf, kf, vf = (t.float().view(1, t.shape[1], H, 64).transpose(1, 2).requires_grad_()
                      for t in (q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n]))
        of = torch.softmax((qf @ kf.transpose(-1, -2)) * 0.125, -1) @ vf
        of.backward(do[b:b + 1].float().view(1, Nq, H, 64).transpose(1, 2))
        for name, got, want in (("dq", dq[b:b + 1], qf.grad), ("dk", dk[b:b + 1, :n], kf.grad),
                                ("dv", dv[b:b + 1, :n], vf.grad)):
            r = rel(got.float(), want.transpose(1, 2).reshape(got.shape))
            print(f"k_len bwd b={b} len={n} {name}: rel {r:.3e}")
            assert r < 2e-2, (b, name)
    # NULL against the full length in every row
    o2, lse2 = _truncated_forward(q, k, v, [Nk] * B, H)
    none = K.attention_bwd(q, k, v, o2, do, lse2, H)
    full = K.attention_bwd(q, k, v, o2, do, lse2, H, k_len=torch.full((B,), Nk, dtype=torch.int32, device=dev))
    for name, a, b_ in zip(("dq", "dk", "dv"), none, full):
        assert torch.equal(a, b_), name


def test_attention_bwd_k_len_tail_split(knobs):
    """k_len under the grid-tail split (the pieces are planned from Nk; a short row leaves some with fewer tiles, and
    its key blocks past the length with none): against the unsplit launch at the split's own rule, rows past the
    length zero in both."""
    from videopainter_amd import _native as N_
    from videopainter_amd import kernels as K
    B, H, Nq, Nk = 2, 17, 8010, 7003
    klen = [7003, 4100]
    D = H * 64
    q, k, v, do = (bf(rnd(B, n, D, seed=s)).to(dev) for n, s in ((Nq, 11), (Nk, 12), (Nk, 13), (Nq, 14)))
    o, lse = _truncated_forward(q, k, v, klen, H)
    kl = torch.tensor(klen, dtype=torch.int32, device=dev)
    d = N_.AttnBwdDesc()
    d.B, d.H, d.Nq, d.Nk, d.head_dim = B, H, Nq, Nk, 64
    for nm, t in (("Q", q), ("K", k), ("V", v), ("O", o), ("dO", do), ("dQ", q), ("dK", k), ("dV", v)):
        setattr(d, nm, t.data_ptr())
    for nm, t in (("q", q), ("k", k), ("v", v), ("o", o), ("do", do), ("dq", q), ("dk", k), ("dv", v)):
        setattr(d, f"{nm}_sb", t.stride(0))
        setattr(d, f"{nm}_sn", t.stride(1))
    d.lse, d.delta, d.k_len = lse.data_ptr(), lse.data_ptr(), kl.data_ptr()
    assert N_.lib().vp_attention_bwd_workspace_bytes(C.byref(d)) > 0  # the split is active for this shape
    got = {}
    for name in ("split", "whole"):
        if name == "whole":
            knobs.setenv("VP_ATTN_NO_SPLIT", "1")
        dq, dk, dv = _nan_grads(B, Nq, Nk, D)
        K.attention_bwd(q, k, v, o, do, lse, H, dq=dq, dk=dk, dv=dv, k_len=kl)
        torch.cuda.synchronize()
        for b, n in enumerate(klen):
            assert not dk[b, n:].float().ne(0).any() and not dv[b, n:].float().ne(0).any(), (name, b)
            assert not torch.isnan(dk[b, n:].float()).any() and not torch.isnan(dv[b, n:].float()).any(), (name, b)
        got[name] = (dq, dk, dv)
    for name, a, b_ in zip(("dq", "dk", "dv"), got["split"], got["whole"]):
        assert torch.isfinite(a.float()).all() and torch.isfinite(b_.float()).all(), name
        r = rel(a.float(), b_.float())
        print(f"k_len bwd tail split {name}: rel {r:.3e}")
        assert r < 2e-3, name


# ---- 3: the lse of the two-segment forward with l_extra ----

@pytest.mark.parametrize("split", [True, False], ids=["tailsplit", "nosplit"])
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
def test_two_segment_forward_lse_includes_l_extra(bounded, split, knobs):
    """The statistics the training forward keeps: lse = log2(sum over both segments' keys of 2^s + 2^l_extra), from
    the default kernels (bounded and unbounded scores) with and without the tail split, against fp64 — rows whose
    l_extra is -inf included (the inputs of test_attention_k2_len_and_l_extra)."""
    from videopainter_amd import kernels as K
    if not split:
        knobs.setenv("VP_ATTN_NO_SPLIT", "1")
    B, H, Nn, N2 = 3, 2, 700, 900
    D = H * 64
    q, k, v = (bf(rnd(B, Nn, D, seed=s) * 0.5).to(dev) for s in (95, 96, 97))
    k2, v2 = bf(rnd(B, N2, D, seed=98) * 0.5).to(dev), bf(rnd(B, N2, D, seed=99)).to(dev)
    klen = torch.tensor([300, 0, 900], dtype=torch.int32)
    lx = rnd(B, H, Nn, seed=100) * 4.0 + 3.0
    lx[:, :, ::7] = float("-inf")
    o = torch.empty(B, Nn, D, device=dev, dtype=torch.bfloat16)
    lse = torch.full((B, H, Nn), float("nan"), device=dev, dtype=torch.float32)
    K.attention(q, k, v, o, H, k2=k2, v2=v2, k2_len=klen.to(dev), l_extra=lx.to(dev), lse=lse,
                bounded_scores=bounded)
    hd = lambda x: x.double().cpu().reshape(x.shape[0], -1, H, 64).transpose(1, 2)  # noqa: E731
    ref = torch.empty(B, H, Nn, dtype=torch.float64)
    for b in range(B):
        n2 = int(klen[b])
        kk = torch.cat([hd(k[b:b + 1]), hd(k2[b:b + 1, :n2])], 2)[0]
        s = (hd(q[b:b + 1])[0] @ kk.transpose(-1, -2)) * (0.125 * LOG2E)
        s = torch.cat([s, lx[b].double()[..., None]], -1)
        ref[b] = torch.logsumexp(s * math.log(2.0), -1) / math.log(2.0)
    assert torch.isfinite(lse).all()
    r = rel(lse, ref)
    print(f"two-segment lse bounded={bounded} split={split}: rel {r:.3e} max "
          f"{float((lse.double().cpu() - ref).abs().max()):.3e}")
    assert r < 1e-3, r


# ---- 4: vp_null_key_mass_bwd ----

def _grid_rope(F_, Hh, Ww):
    from oracle.cogvideox_oracle import prepare_rotary_positional_embeddings
    cos, sin = prepare_rotary_positional_embeddings(Hh * 16, Ww * 16, F_, 64)
    return cos.float(), sin.float()


def _null_keys(T, cos, sin, beta):
    """fp64 [T + Nv, 64]: beta (text rows) / RoPE(beta) rounded to bf16 (video rows), the keys the reference's bf16
    apply_rotary_emb writes for a zeroed row."""
    bt = beta.double().cpu()
    rot = torch.stack([-bt[1::2], bt[0::2]], -1).reshape(64)  # apply_rotary_emb's interleaved pairs
    kv = (bt[None] * cos.double() + rot[None] * sin.double()).to(torch.bfloat16).double()
    return torch.cat([bt[None].expand(T, 64), kv], 0)


def _run_null_key_mass_bwd(m, grid, T, B, H, seed):
    """-> (dq written into zeros, fp64 reference, lx, batch rows with a null key).  The reference: fp64 autograd of
    the explicit log-sum lx = log2 sum_{null j} 2^(c q.k_j), with dq = -scale D 2^(lx - lse) grad_q lx / c."""
    from videopainter_amd import kernels as K
    F_, Hh, Ww = grid
    scale = 0.125
    c = scale * LOG2E
    cos, sin = _grid_rope(*grid)
    Ntok = T + F_ * Hh * Ww
    m8 = m.to(torch.uint8).to(dev)
    q = bf(rnd(B, Ntok, H * 64, seed=seed) * 1.5).to(dev)
    beta = bf(rnd(64, seed=seed + 1) * 0.8).to(dev)
    axes = K.rope_axis_tables((cos.to(dev), sin.to(dev)), grid)
    assert axes is not None and K.null_key_mass_bwd_supported(grid)
    segments = K.mask_null_segments(m8, T, grid)
    lx = K.null_key_mass(q, H, T, grid, beta, axes, m8, segments, scale)
    has = [b for b in range(B) if not bool(m[b].all())]
    gap = torch.rand(B, H, Ntok, generator=torch.Generator().manual_seed(seed + 2)) * 3.0
    lse = torch.where(torch.isfinite(lx.cpu()), lx.cpu() + gap, gap).float()  # lse >= lx
    delta = rnd(B, H, Ntok, seed=seed + 3)
    dq = torch.zeros(B, Ntok, H * 64, device=dev, dtype=torch.bfloat16)
    K.null_key_mass_bwd(q, H, T, grid, beta, axes, m8, segments, scale, lse.to(dev), delta.to(dev), dq)
    torch.cuda.synchronize()
    keys = _null_keys(T, cos, sin, beta)
    ref = torch.zeros(B, Ntok, H, 64, dtype=torch.float64)
    for b in has:
        qh = q[b].double().cpu().view(Ntok, H, 64).requires_grad_()
        s = torch.einsum("nhd,kd->hnk", qh, keys) * c
        s = s.masked_fill(m[b].bool()[None, None, :], float("-inf"))
        lxr = torch.logsumexp(s * math.log(2.0), -1) / math.log(2.0)  # [H, Ntok]
        w = torch.exp2(lxr.detach() - lse[b].double()) * (-scale * delta[b].double()) / c
        lxr.backward(w)
        ref[b] = qh.grad
    return dq, ref.view(B, Ntok, H * 64), lx, has, (q, beta, axes, m8, segments, scale, lse, delta)


def test_null_key_mass_bwd_matches_explicit_null_keys():
    """The grid, mask and magnitudes of test_null_key_mass_matches_explicit_null_keys: an 8-run row (the per-column
    scan), an all-null and a no-null row, text rows all / partly null, and a batch row without any null key, whose
    dq stays bit-identical."""
    from videopainter_amd import kernels as K
    B, H, T, F_, Hh, Ww = 3, 3, 7, 3, 5, 16
    grid = (F_, Hh, Ww)
    Ntok = T + F_ * Hh * Ww
    g = torch.Generator().manual_seed(5)
    m = torch.rand(B, Ntok, generator=g) < 0.5
    m[0, :T] = False
    vid = m[:, T:].view(B, F_, Hh, Ww)
    vid[0, 1, 2] = torch.arange(Ww) % 2 == 1
    vid[1, 0, 0] = False
    vid[1, 2, 4] = True
    m[2] = True
    dq, ref, lx, has, args = _run_null_key_mass_bwd(m, grid, T, B, H, seed=60)
    assert has == [0, 1]
    assert int(args[4][0][(0 * F_ + 1) * Hh:(0 * F_ + 1) * Hh + int(args[4][1][1]), 2].eq(255).sum()) == 1
    assert torch.isfinite(dq.float()).all()
    for b in has:
        r = rel(dq[b].float(), ref[b])
        print(f"null_key_mass_bwd b={b}: rel {r:.3e}")
        assert r < 1e-2, (b, r)
    assert not dq[2].float().ne(0).any()
    # the batch row without a null key: a pre-filled dq stays as it is, bit for bit; the others accumulate
    q, beta, axes, m8, segments, scale, lse, delta = args
    pre = bf(rnd(B, Ntok, H * 64, seed=70)).to(dev)
    dq2 = pre.clone()
    K.null_key_mass_bwd(q, H, T, grid, beta, axes, m8, segments, scale, lse.to(dev), delta.to(dev), dq2)
    assert torch.equal(dq2[2], pre[2])
    # (one bf16 rounding of the sum, 2^-9 relative — 2^-8 allowed — on top of the kernel's own 1e-2 of its term)
    tot = pre[:2].double().cpu() + ref[:2]
    err = (dq2[:2].double().cpu() - tot).abs()
    assert bool((err <= 2.0 ** -8 * tot.abs() + 1e-2 * ref[:2].abs().max()).all())


def test_null_key_mass_bwd_box_mask():
    """A box mask — the same rectangle in every frame, the rows above and below it all null: merged multi-row
    segments of one and of two runs."""
    B, H, T, F_, Hh, Ww = 2, 2, 5, 4, 9, 14
    grid = (F_, Hh, Ww)
    m = torch.zeros(B, T + F_ * Hh * Ww, dtype=torch.bool)
    vid = m[:, T:].view(B, F_, Hh, Ww)
    vid[0, :, 2:6, 3:9] = True
    vid[1, :, 0:4, 0:5] = True  # a box in the corner: one run per row, no row above it
    dq, ref, lx, has, _ = _run_null_key_mass_bwd(m, grid, T, B, H, seed=80)
    assert has == [0, 1]
    for b in has:
        r = rel(dq[b].float(), ref[b])
        print(f"null_key_mass_bwd box b={b}: rel {r:.3e}")
        assert r < 1e-2, (b, r)


# ---- 5: vp_gather_add_rows_bf16 ----

def test_gather_add_rows_exact():
    """y[b, n] += x[b, rows[b, n]] on the masked rows with a source row: one fp32 add and one rounding, so equal to
    the index expression in torch; every other row bit-identical (strided views of wider buffers)."""
    from videopainter_amd import kernels as K
    B, N, D = 3, 333, 192
    g = torch.Generator().manual_seed(9)
    m = (torch.rand(B, N, generator=g) < 0.4)
    m[2] = False
    m8 = m.to(torch.uint8).to(dev)
    dst, cnt = K.partition_rows_index(m8)
    dst = torch.where(m8.bool(), dst, torch.full_like(dst, -1))
    buf = bf(rnd(B, 2 * N, D, seed=10)).to(dev)  # y = rows [0, N), x = rows [N, 2N): the backward's layout
    wide = bf(rnd(B, N, 3 * D, seed=11)).to(dev)
    for y, x in ((buf[:, :N], buf[:, N:]), (wide[..., D:2 * D], buf[:, N:].clone())):
        before = y.clone()
        want = before.clone()
        for b in range(B):
            idx = m[b].nonzero().flatten().to(dev)
            want[b, idx] = (before[b, idx].float() + x[b, dst[b, idx].long()].float()).to(torch.bfloat16)
        K.gather_add_rows(x, y, m8, dst)
        torch.cuda.synchronize()
        assert torch.equal(y, want)
        assert torch.equal(y[~m.to(dev)], before[~m.to(dev)])


# ---- 6 - 8: the block and the model with the switch on, against the oracle's autograd ----

GATE_MUL, GATE_ADD = 1.25, 1e-3  # the model tests' rule (tests/test_training_gpu.py)


def _check(name, got, want, ref16):
    r = rel(got.float(), want)
    r16 = rel(ref16.float(), want)
    print(f"{name:48s} HIP {r:.3e}  oracle-bf16 {r16:.3e}")
    assert r <= GATE_MUL * r16 + GATE_ADD, (name, r, r16)


def _resample_mask(T, tok_mask):
    m = torch.zeros(tok_mask.shape[0], T + tok_mask.shape[1], dtype=torch.bool)
    m[:, T:] = tok_mask.bool()
    return m


def _tiny_grid():
    from tests.golden.cases import TINY_F, TINY_H, TINY_W
    return (TINY_F, TINY_H // 2, TINY_W // 2)


def _resample_block(closed_form=True, freeze_beta=True):
    from tests.golden.cases import TINY_CFG, tiny_weights
    from videopainter_amd import CogVideoXTransformer3DModel, device_scope
    tsd, _ = tiny_weights()
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**dict(TINY_CFG, id_pool_resample_learnable=True))
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    tr.enable_closed_form_resample_backward(closed_form)
    blk = tr.transformer_blocks[0]
    blk.requires_grad_(True)
    if freeze_beta:
        blk.attn1.norm_k.bias.requires_grad_(False)
    return blk, tsd


@pytest.mark.parametrize("mask_kind", ["random", "box"])
def test_closed_form_resample_block_backward_matches_oracle(mask_kind):
    """The setting of test_resample_block_backward_matches_oracle with the closed-form backward on, norm_k.bias
    frozen and the grid on the rope: d x, d temb and every other parameter gradient against the oracle's autograd of
    the explicit 2N-key attention, the oracle's own bf16 run as the yardstick."""
    from oracle import cogvideox_oracle as O
    from tests.golden.cases import TINY_CFG, tiny_inputs
    from videopainter_amd.attention_processor import _rope_dev
    from videopainter_amd.autograd import block_apply
    from videopainter_amd.config import full_config
    blk, tsd = _resample_block()
    assert blk.attn1.closed_form_resample_backward
    cfg = dict(full_config(TINY_CFG), id_pool_resample_learnable=True)
    i = tiny_inputs()
    T = i["enc"].shape[1]
    D = 128
    Nv = i["rope"][0].shape[0]
    F_, Hh, Ww = grid = _tiny_grid()
    assert F_ * Hh * Ww == Nv
    g = torch.Generator().manual_seed(15)
    x = torch.randn(2, T + Nv, D, generator=g).bfloat16()
    temb = torch.randn(2, TINY_CFG["time_embed_dim"], generator=g).bfloat16()
    dout = torch.randn(2, T + Nv, D, generator=g).bfloat16()
    tm = (torch.rand(2, Nv, generator=g) < 0.4)
    if mask_kind == "box":  # the same rectangle in every frame
        tm = torch.zeros(2, F_, Hh, Ww, dtype=torch.bool)
        tm[0, :, 1:Hh - 1, 2:Ww - 1] = True
        tm[1, :, 0:Hh // 2, 0:Ww // 2] = True
        tm = tm.view(2, Nv)
    rm = _resample_mask(T, tm)
    xd = x.to(dev).requires_grad_()
    td = temb.to(dev).requires_grad_()
    rope = _rope_dev((i["rope"][0].to(dev), i["rope"][1].to(dev)), xd.device, grid)
    out = block_apply(blk, xd, T, td, rope, resample_mask=rm.to(dev).to(torch.uint8))
    out.backward(dout.to(dev))
    names = [n for n, p in blk.named_parameters() if p.requires_grad]
    assert "attn1.norm_k.bias" not in names and "attn1.norm_k.weight" in names
    ours = {n: p.grad for n, p in blk.named_parameters()}

    def oracle(dtype):
        sd = {k[len("transformer_blocks.0."):]: torch.from_numpy(v).to(dtype).requires_grad_()
              for k, v in tsd.items() if k.startswith("transformer_blocks.0.")}
        xo = x.to(dtype).requires_grad_()
        to = temb.to(dtype).requires_grad_()
        h, e = O.block_forward({f"b.{k}": v for k, v in sd.items()}, "b", cfg, xo[:, T:], xo[:, :T], to,
                               i["rope"], resample_mask=rm.to(dtype), resample=True)
        out_o = torch.cat([e, h], 1)
        out_o.backward(dout.to(dtype))
        return out_o.detach(), xo.grad, to.grad, {k: sd[k].grad for k in names}

    o32, gx32, gt32, gp32 = oracle(torch.float32)
    o16, gx16, gt16, gp16 = oracle(torch.bfloat16)
    _check("out", out.detach(), o32, o16)
    _check("dx", xd.grad, gx32, gx16)
    _check("dtemb", td.grad, gt32, gt16)
    for n in names:
        assert ours[n] is not None, n
        _check(n, ours[n], gp32[n], gp16[n])


def test_closed_form_resample_lora_training_step_matches_oracle(monkeypatch):
    """The LoRA step of test_resample_lora_training_step_matches_oracle with the switch on: the output and every
    LoRA factor gradient against the oracle's autograd; and the closed-form arm makes no attention launch during the
    backward (a counting wrapper round kernels.attention, here only)."""
    from oracle import cogvideox_oracle as O
    from tests.golden.cases import TINY_BRANCH_CFG, TINY_CFG, tiny_inputs, tiny_weights
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd import kernels as K
    from videopainter_amd.config import full_config
    tsd, bsd = tiny_weights()
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**dict(TINY_CFG, id_pool_resample_learnable=True))
        br = CogvideoXBranchModel(**TINY_BRANCH_CFG)
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    br.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()})
    br.requires_grad_(False)
    tr.add_adapter({"r": 4, "lora_alpha": 8, "init_lora_weights": True,
                    "target_modules": ["to_q", "to_k", "to_v", "to_out.0"]})
    tr.enable_closed_form_resample_backward()
    trainable = [n for n, p in tr.named_parameters() if p.requires_grad]
    assert len(trainable) == 2 * 4 * TINY_CFG["num_layers"]
    g = torch.Generator().manual_seed(7)
    facs = {}
    with torch.no_grad():  # PEFT starts B at 0 (dA = 0): a trained-looking pair instead
        for n, p in tr.named_parameters():
            if p.requires_grad:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
                facs[n] = p.detach().float().cpu()
    i = tiny_inputs()
    R = torch.randn(i["video"].shape, generator=g).bfloat16()
    samples = br(hidden_states=i["video"].to(dev).bfloat16(), encoder_hidden_states=i["enc"].to(dev).bfloat16(),
                 branch_cond=i["branch_cond"].to(dev).bfloat16(), timestep=i["timestep"].to(dev),
                 image_rotary_emb=i["rope"], return_dict=False)[0]
    calls = {"n": 0}
    real = K.attention

    def counting(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)
    monkeypatch.setattr(K, "attention", counting)
    out = tr(hidden_states=i["hidden"].to(dev).bfloat16(), encoder_hidden_states=i["enc"].to(dev).bfloat16(),
             timestep=i["timestep"].to(dev), image_rotary_emb=i["rope"], branch_block_samples=samples,
             branch_block_masks=i["mask"].to(dev), id_pool_resample_learnable=True, return_dict=False)[0]
    assert out.requires_grad
    forward_calls = calls["n"]
    assert forward_calls == TINY_CFG["num_layers"]
    out.backward(R.to(dev))
    assert calls["n"] == forward_calls, "the closed-form backward launched an attention forward"
    monkeypatch.setattr(K, "attention", real)
    ours = {n: p.grad for n, p in tr.named_parameters() if p.requires_grad}

    def oracle(dtype):
        tp = {k: torch.from_numpy(v).to(dtype) for k, v in tsd.items()}
        leaves = {n: v.detach().clone().to(dtype).requires_grad_() for n, v in facs.items()}
        for n in leaves:
            if n.endswith(".lora_A.weight"):
                mod = n[:-len(".lora_A.weight")]
                tp[mod + ".weight"] = tp[mod + ".weight"] + 2.0 * (leaves[mod + ".lora_B.weight"] @ leaves[n])
        bp = {k: torch.from_numpy(v).to(dtype) for k, v in bsd.items()}
        s = O.branch_forward(bp, full_config(TINY_BRANCH_CFG, True), i["video"].to(dtype), i["enc"].to(dtype),
                             i["branch_cond"].to(dtype), i["timestep"], i["rope"])
        o = O.transformer_forward(tp, dict(full_config(TINY_CFG), id_pool_resample_learnable=True),
                                  i["hidden"].to(dtype), i["enc"].to(dtype), i["timestep"], i["rope"],
                                  branch_block_samples=s, branch_block_masks=i["mask"].to(dtype),
                                  id_pool_resample_learnable=True)[0]
        o.backward(R.to(dtype))
        return o.detach(), {n: leaves[n].grad for n in leaves}

    missing = [n for n in trainable if ours[n] is None]
    assert not missing, missing
    o32, gp32 = oracle(torch.float32)
    o16, gp16 = oracle(torch.bfloat16)
    _check("output", out.detach(), o32, o16)
    for n in trainable:
        _check(n, ours[n], gp32[n], gp16[n])


def test_closed_form_resample_backward_refusals():
    """The opt-in does not fall back: a trainable norm_k.bias (its null-key gradient is not built) and a rope
    without the video grid (no closed-form plan) raise when the block is applied."""
    from tests.golden.cases import TINY_CFG, tiny_inputs
    from videopainter_amd.attention_processor import _rope_dev
    from videopainter_amd.autograd import block_apply
    i = tiny_inputs()
    T = i["enc"].shape[1]
    Nv = i["rope"][0].shape[0]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, T + Nv, 128, generator=g).bfloat16().to(dev).requires_grad_()
    temb = torch.randn(2, TINY_CFG["time_embed_dim"], generator=g).bfloat16().to(dev)
    rm = _resample_mask(T, torch.rand(2, Nv, generator=g) < 0.4).to(dev).to(torch.uint8)
    cs = (i["rope"][0].to(dev), i["rope"][1].to(dev))
    with_grid = _rope_dev(cs, x.device, _tiny_grid())
    blk, _ = _resample_block(freeze_beta=False)
    with pytest.raises(NotImplementedError, match="norm_k"):
        block_apply(blk, x, T, temb, with_grid, resample_mask=rm)
    blk.attn1.norm_k.bias.requires_grad_(False)
    with pytest.raises(ValueError, match="grid"):
        block_apply(blk, x, T, temb, cs, resample_mask=rm)
    with pytest.raises(ValueError, match="grid"):
        block_apply(blk, x, T, temb, _rope_dev(cs, x.device), resample_mask=rm)
    block_apply(blk, x, T, temb, with_grid, resample_mask=rm)  # (and the supported form goes through)
