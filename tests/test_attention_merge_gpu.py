"""The merge of two attention partials (vp_attention_merge_bf16) and the composed attention of the two
classifier-free-guidance halves built on it (attention_processor.cfg_shared_attention), GPU only.

Tolerances come from the number formats, not from what the kernels give:
  * the merge kernel evaluates its formula in fp32 (relative error about 2^-22) and rounds once to bf16, so it lies
    within one bf16 ulp of the exact value of the formula;
  * the composed attention keeps its partials in fp32 and rounds to bf16 once, in the merge, as a single call rounds
    once: the two fp32 values differ by the order of a few fp32 sums (relative 2^-20 at most, against the 2^-9 of
    a bf16 half-ulp), so an element's rounding flips with probability about 2^-11 and then moves by one ulp.  The
    issue's gate (the composed errors against fp64 may exceed the single call's by one bf16 ulp at the output
    scale) is kept; beside it the rel-L2 error may exceed the single call's by 5 % (the flips add about 0.6 % to the
    error's variance: 5 % is an order above that and far below the 14 % a second bf16 rounding adds).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp (8 significant bits) at the magnitude of every element of the fp64 tensor x."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_merge_kernel_matches_fp64_formula():
    """B = 2, H = 2, Nq = 450, input a one copy read by both batch rows (batch stride 0); lse gaps of 0, +-30 and
    +-150 log2 units across the queries, and rows where one input's lse is -inf (its values, NaN here, must not
    reach the output).  The output is a strided view (the video rows of a joint buffer)."""
    from videopainter_amd import kernels as K
    B, H, Nq, T = 2, 2, 450, 34
    D = H * 64
    g = torch.Generator().manual_seed(5)
    o_a = torch.randn(1, Nq, D, generator=g).to(BF16)
    o_b = torch.randn(B, Nq, D, generator=g).to(BF16)
    lse_b = (torch.randn(B, H, Nq, generator=g) * 3.0 + 9.0).float()
    gaps = torch.tensor([0.0, 30.0, -30.0, 150.0, -150.0])[torch.arange(Nq) % 5]
    lse_a = (lse_b[:1] + gaps).clone()  # the gaps hold for batch 0; batch 1 sees them shifted by its own lse_b
    dead_a = torch.arange(Nq) % 11 == 3  # input a empty (both heads, so that the whole row of O_a can be NaN)
    dead_b = torch.arange(Nq) % 13 == 5  # input b empty in batch 1, head 1
    lse_a[:, :, dead_a] = -math.inf
    o_a[:, dead_a] = float("nan")
    lse_b[1, 1, dead_b] = -math.inf
    o_b[1][dead_b, 64:] = float("nan")
    # fp64 evaluation of the formula
    la, lb = lse_a.double().expand(B, H, Nq), lse_b.double()
    both = torch.isinf(la) & torch.isinf(lb)  # (queries 135, 278, 421 of batch 1, head 1: no mass at all -> zeros)
    assert both.any() and not both[0].any()
    m = torch.where(both, torch.zeros_like(la), torch.maximum(la, lb))
    wa, wb = torch.pow(2.0, la - m), torch.pow(2.0, lb - m)
    oa64 = o_a.double().expand(B, Nq, D).reshape(B, Nq, H, 64).permute(0, 2, 1, 3)
    ob64 = o_b.double().reshape(B, Nq, H, 64).permute(0, 2, 1, 3)
    oa64 = torch.where((wa == 0)[..., None], torch.zeros_like(oa64), oa64)
    ob64 = torch.where((wb == 0)[..., None], torch.zeros_like(ob64), ob64)
    want = (wa[..., None] * oa64 + wb[..., None] * ob64) / (wa + wb).clamp_min(1e-300)[..., None]
    want = want.permute(0, 2, 1, 3).reshape(B, Nq, D)
    assert torch.isfinite(want).all()

    buf = torch.full((B, T + Nq, D), 7.0, device=dev, dtype=BF16)
    out = buf[:, T:]
    K.attention_merge(o_a.to(dev).expand(B, -1, -1), lse_a.to(dev).expand(B, -1, -1), o_b.to(dev), lse_b.to(dev), out,
                      H)
    torch.cuda.synchronize()
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    over = err > bf16_ulp(want)
    print(f"merge: max |err| / ulp {float((err / bf16_ulp(want)).max()):.3f}")
    assert not over.any(), (int(over.sum()), float(err.max()))
    assert torch.all(buf[:, :T] == 7.0)  # nothing written outside the view


def _attention_fp64(q, k, v, H, scale):
    B, N, D = q.shape
    qh, kh, vh = (t.double().reshape(B, N, H, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(B, N, D)


@pytest.mark.parametrize("T,Nv", [(34, 450), (130, 700)])
def test_composed_cfg_attention_matches_single_call(T, Nv):
    """Pieces (a)-(d) of cfg_shared_attention against one vp_attention_fwd_bf16 call on the joint sequence and
    against fp64.  T = 130, Nv = 700: a masked last key tile in the text and in the video segment, several query
    blocks.  Batch 1's video rows of q / k / v are NaN for the composed call: it may not read them."""
    from videopainter_amd import kernels as K
    from videopainter_amd.attention_processor import cfg_shared_attention
    H, scale = 2, 0.125
    D, N = H * 64, T + Nv
    g = torch.Generator().manual_seed(1000 + T)
    qkv = torch.randn(2, N, 3 * D, generator=g)
    qkv[1, T:] = qkv[0, T:]  # the halves' video rows are equal, the text rows differ
    qkv = qkv.to(BF16)
    ref = _attention_fp64(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], H, scale)

    qd = qkv.to(dev)
    single = torch.empty(2, N, D, device=dev, dtype=BF16)
    K.attention(qd[..., :D], qd[..., D:2 * D], qd[..., 2 * D:], single, H, scale=scale)
    qp = qd.clone()
    qp[1, T:] = float("nan")
    comp = torch.empty(2, N, D, device=dev, dtype=BF16)
    cfg_shared_attention(qp[..., :D], qp[..., D:2 * D], qp[..., 2 * D:], comp, H, T, scale=scale)
    torch.cuda.synchronize()
    single, comp = single.double().cpu(), comp.double().cpu()
    assert torch.isfinite(comp).all()

    def errs(x):
        return float((x - ref).abs().max()), float((x - ref).norm() / ref.norm())

    (ms, rs), (mc, rc) = errs(single), errs(comp)
    omax = float(ref.abs().max())
    ulp = float(bf16_ulp(torch.tensor(omax, dtype=torch.float64)))
    print(f"T={T} Nv={Nv}: single max {ms:.3e} rel-L2 {rs:.3e} | composed max {mc:.3e} rel-L2 {rc:.3e} | "
          f"bf16 ulp at max|O|={omax:.3f}: {ulp:.3e}")
    assert mc <= ms + ulp, (mc, ms, ulp)
    assert rc <= rs + ulp / omax, (rc, rs, ulp / omax)
    assert rc <= 1.05 * rs, (rc, rs)


def test_merge_kernel_fp32_partials_round_once():
    """fp32 partials (the attention's VP_ATTN_OUT_F32 outputs) with one input at batch stride 0: the merge is the
    fp64 formula rounded to bf16 once (within one bf16 ulp; at most a half-ulp plus fp32 noise)."""
    from videopainter_amd import kernels as K
    B, H, Nq = 2, 2, 450
    D = H * 64
    g = torch.Generator().manual_seed(6)
    o_a, o_b = torch.randn(1, Nq, D, generator=g), torch.randn(B, Nq, D, generator=g)
    lse_a = torch.randn(1, H, Nq, generator=g) * 3.0 + 9.0
    gaps = torch.tensor([0.0, 5.0, -5.0, 30.0, -30.0])[torch.arange(Nq) % 5]
    lse_b = lse_a + gaps + torch.randn(B, H, Nq, generator=g)
    la, lb = lse_a.double().expand(B, H, Nq), lse_b.double()
    m = torch.maximum(la, lb)
    wa, wb = torch.pow(2.0, la - m), torch.pow(2.0, lb - m)
    heads = lambda x: x.double().expand(B, Nq, D).reshape(B, Nq, H, 64).permute(0, 2, 1, 3)  # noqa: E731
    want = ((wa[..., None] * heads(o_a) + wb[..., None] * heads(o_b)) / (wa + wb)[..., None]).permute(0, 2, 1, 3)
    want = want.reshape(B, Nq, D)
    out = torch.empty(B, Nq, D, device=dev, dtype=BF16)
    K.attention_merge(o_a.to(dev).expand(B, -1, -1), lse_a.to(dev).expand(B, -1, -1), o_b.to(dev), lse_b.to(dev), out,
                      H)
    err = (out.double().cpu() - want).abs() / bf16_ulp(want)
    print(f"merge fp32: max |err| / ulp {float(err.max()):.3f}")
    assert float(err.max()) <= 0.51


def test_composed_cfg_attention_large_grid_matches_single_call():
    """A grid of more than two rounds of workgroups in every piece (H = 2, 131203 video rows, 130 text rows: 1026
    query blocks in piece (a), 2052 in (b)), where the attention runs its persistent instance with the remainder
    blocks as key-range pieces and the combine pass — with lse and fp32 outputs, q_sb = 0 and k2_sb = 0.  No fp64
    reference at this size: the composed output against the single call's.  Both round to bf16 once, from fp32
    values that differ in summation order and, where a piece takes another reference point, in the bf16 rounding
    of P; an error in the tail pieces, the combine or the strides would show as whole rows or blocks off by the
    size of the output.  Gate, in the issue's form: no element differs by more than one bf16 ulp at the output
    scale (max |O|), and at most 1 % of the elements differ at all (bound chosen before the first run, which gave
    0.65 %)."""
    from videopainter_amd import kernels as K
    from videopainter_amd.attention_processor import cfg_shared_attention
    H, scale, T, Nv = 2, 0.125, 130, 131203
    D, N = H * 64, T + Nv
    g = torch.Generator(device=dev).manual_seed(9)
    qkv = torch.randn(2, N, 3 * D, generator=g, device=dev, dtype=torch.float32).to(BF16)
    qkv[1, T:] = qkv[0, T:]
    single = torch.empty(2, N, D, device=dev, dtype=BF16)
    K.attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], single, H, scale=scale)
    qp = qkv.clone()
    qp[1, T:] = float("nan")
    comp = torch.empty(2, N, D, device=dev, dtype=BF16)
    cfg_shared_attention(qp[..., :D], qp[..., D:2 * D], qp[..., 2 * D:], comp, H, T, scale=scale)
    torch.cuda.synchronize()
    assert torch.isfinite(comp.float()).all()
    a, b = comp.float(), single.float()
    diff = (a - b).abs()
    omax = float(b.abs().max())
    ulp = 2.0 ** (math.floor(math.log2(omax)) - 7)
    frac, dmax = float((diff > 0).float().mean()), float(diff.max())
    print(f"large grid: elements differing {frac:.3e}, max |diff| {dmax:.3e}, bf16 ulp at max|O|={omax:.4f}: "
          f"{ulp:.3e}, rel-L2 {float(diff.norm() / b.norm()):.3e}")
    assert dmax <= ulp, (dmax, ulp)
    assert frac <= 1e-2, frac
