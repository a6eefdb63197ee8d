"""The forward GEMM's epilogues (csrc/gemm.hip: vp_gemm_bf16, vp_gemm_bf16_ws, vp_gemm_mx_fp8) and
vp_head_norm_rope_bf16, every output element against the references of tests/gemm_refs.py (each checked on the CPU by
tests/test_gemm_refs_cpu.py, where the mutants are run against the same gate, gemm_refs.check_output).

Integer-valued operands make the accumulator exact for every main loop, K split and summation order, so BIAS, SCALE,
GATED, ADDROWS and the aux outputs are compared bit for bit with the chain include/vp_hip.h documents, and GELU,
GELU_BWD and QKNORM_ROPE per element with float64 of the exactly known rnd(acc + bias).  Every output buffer carries
sentinel rows after its last row and sentinel columns in [N, ld); the whole buffer is compared, so rows the remap must
not touch are part of the check.  A's padding columns [K, lda) hold NaN.  A second, smaller part bounds the
accumulation error with real-valued operands.  A run with -s prints, per case, "bit-equal" or the worst
error / allowed: profiles/gemm_epilogue_tests.log is that record.

Pinned beyond the GEMM: a zeroed row behind vp_head_norm_rope_bf16 is the rotated LayerNorm bias bit for bit
(gemm_refs.rot_bias_bits), and the AdaLN modulation y = rnd(rnd(n s1) + shift) of vp_adaln_modulate_bf16 and
vp_final_norm_bf16 is compared bit for bit on rows whose LayerNorm is exact (gemm_refs.adaln_exact_case): the product
rounding of that chain and of the gated residual, rnd(R + rnd(gate y)), is one the compiler drops when it is written
as a plain bf16 round trip (vp_common.h rbf_prod)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from tests import backward_refs as R
from tests import gemm_refs as G
from tests import mx_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
U8 = G.U8


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videopainter_amd import _native, kernels
    _native.lib()
    print(f"\nc_f32 of the forward head vectors (tests/gemm_refs.py; measured on the CPU by "
          f"tests/test_gemm_refs_cpu.py::test_c_f32_head_fwd): {G.C_F32_HEAD_FWD:.2e}")
    return kernels


def _sent(rows, cols):
    return torch.full((rows, cols), G.SENT, device=dev, dtype=BF)


def workspace_bytes(c):
    from videopainter_amd import _native as N
    d = N.GemmDesc()
    d.M, d.N, d.K, d.epilogue, d.n_seg, d.lda = c.M, c.N, c.K, c.epi, c.n_seg, c.lda
    return N.lib().vp_gemm_bf16_workspace_bytes(C.byref(d))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def fill_desc(K, d, c, t, cbuf, abuf, keep):
    """every vp_gemm_desc field of case c but A / lda / W (the entry point's operand format), written directly: the
    launch below is the C ABI itself, with nothing of the Python front end in between.  keep: the device tensors the
    descriptor points into."""
    o, N = t.ops, c.N

    def up(x):
        keep.append(x.to(dev))
        return keep[-1]

    d.M, d.N, d.K, d.epilogue, d.n_seg = c.M, N, c.K, c.epi, c.n_seg
    for s in range(c.nsegs):
        d.bias[s] = up(o.bias[s]).data_ptr()
    d.C, d.ldc = cbuf.data_ptr(), cbuf.stride(0)
    d.rows_per_group, d.group_stride, d.row_offset, d.alpha = c.rpg, c.gs, c.ro, c.alpha
    if c.epi == G.GATED:
        if c.alias_R:
            cbuf[:c.out_rows] = t.R.to(dev)
            d.R, d.ldr = cbuf.data_ptr(), cbuf.stride(0)
        else:
            R_ = up(t.R)  # ldr = N + 8
            d.R, d.ldr = R_.data_ptr(), R_.stride(0)
        mod = up(t.mod)  # gate = chunk 2, gate_text = chunk 5 of [B, 6 N + 8]
        d.gate, d.gate_text = mod.data_ptr() + 2 * N * 2, mod.data_ptr() + 5 * N * 2
        d.gate_bstride, d.tokens_per_batch, d.text_len = mod.stride(0), c.tpb, c.T
        if c.inject is not None:
            inj = up(t.inject)
            d.inject, d.inject_ld, d.inject_bstride = inj.data_ptr(), inj.stride(1), inj.stride(0)
            if t.inject_mask is not None:
                m = up(t.inject_mask)
                d.inject_mask, d.inject_mask_bstride = m.data_ptr(), m.stride(0)
    if c.epi == G.ADDROWS:
        ar = up(t.addrows)
        d.addrows, d.addrows_ld, d.addrows_offset = ar.data_ptr(), ar.stride(0), c.addrows_offset
    if c.epi == G.GELU_BWD:
        z = up(t.z)
        d.R, d.ldr = z.data_ptr(), z.stride(0)
    if abuf is not None:
        d.aux, d.ld_aux = abuf.data_ptr(), abuf.stride(0)
    if c.epi == G.QKNORM:
        for s in range(2):
            d.qk_ln_w[s], d.qk_ln_b[s], d.qk_eps[s] = up(t.lnw[s]).data_ptr(), up(t.lnb[s]).data_ptr(), t.eps[s]
        d.tokens_per_batch, d.text_len = c.tpb, c.T
        if t.rope is not None:
            # (no video row: a non-NULL table of which no row may be read)
            cos, sin = (up(torch.cat([x, torch.zeros(1, 64)]))[:c.Nv] for x in t.rope)
            d.rope_cos, d.rope_sin = cos.data_ptr(), sin.data_ptr()
            if c.rope == "sep":
                from videopainter_amd.attention_processor import RopeTables
                rp = RopeTables((cos, sin))
                axes = K.rope_axis_tables(rp, c.grid)
                assert axes is not None
                keep.extend(axes)
                hw, w = c.grid[1] * c.grid[2], c.grid[2]
                for i, ax in enumerate(axes):
                    d.rope_ax[i] = ax.data_ptr()
                d.rope_hw, d.rope_w = hw, w
                d.rope_mhw, d.rope_mw = ((1 << 32) + hw - 1) // hw, ((1 << 32) + w - 1) // w
    if c.a_tail is not None:
        d.a_tail_k = c.a_tail[0]
        for s in range(c.nsegs):
            d.a_tail_off[s] = s * c.a_tail[1]


def _buffers(c):
    cbuf = _sent(c.out_rows + G.GUARD, c.ldc)
    abuf = None
    if c.aux:
        width = 2 * c.n_seg if c.epi == G.QKNORM else c.N
        abuf = _sent(c.M + G.GUARD, width + 8)
    return cbuf, abuf


def launch(K, c, t):
    """one vp_gemm_bf16 (c.ws == "none": the main loop runs the whole K range) or vp_gemm_bf16_ws launch of case c;
    returns the whole C and aux buffers"""
    from videopainter_amd import _native as N
    L, keep = N.lib(), []
    cbuf, abuf = _buffers(c)
    d = N.GemmDesc()
    fill_desc(K, d, c, t, cbuf, abuf, keep)
    a = t.a.to(dev)  # [M, lda]; the columns [Ka, lda) hold NaN
    d.A, d.lda = a.data_ptr(), a.stride(0)
    for s, w in enumerate(t.ops.w):
        keep.append(w.to(dev))
        d.W[s] = keep[-1].data_ptr()
    if c.ws == "none":
        N.check(L.vp_gemm_bf16(C.byref(d), _stream()), "vp_gemm_bf16")
    else:
        nb = L.vp_gemm_bf16_workspace_bytes(C.byref(d))
        if c.ws == "split":
            assert nb >= 2 * c.M * c.N * 4, f"{c.name}: split-K is not active ({nb} workspace bytes)"
        else:
            assert nb >= 16 * 2 * 256 * 256 * 4, f"{c.name}: tail mode is not active ({nb} workspace bytes)"
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        N.check(L.vp_gemm_bf16_ws(C.byref(d), ws.data_ptr(), nb, _stream()), "vp_gemm_bf16_ws")
    torch.cuda.synchronize()
    return cbuf.cpu(), None if abuf is None else abuf.cpu()


def run_cases(K, cases, fn=launch, tag=""):
    """every case runs and prints its line; the cases that miss are raised together at the end"""
    assert cases
    missed = []
    for c in cases:
        t = G.inputs(c)
        ex = G.expected(c, t)
        got_c, got_aux = fn(K, c, t)
        for key, got in (("C", got_c), ("aux", got_aux)):
            if ex[key] is None or (key == "C" and c.epi == G.GELU_MX):
                continue
            try:
                G.check_output(f"{tag}{c.name}: {key}", ex[key], got)
            except AssertionError as e:
                print(f"  MISSES {e}")
                missed.append(str(e))
    assert not missed, "\n".join(missed)


def plain(cases):
    return [c for c in cases if c.epi != G.GATED]


def gated(cases):
    return [c for c in cases if c.epi == G.GATED]


@pytest.fixture(params=G.VARIANTS, ids=[f"gemm_v{v}" for v in G.VARIANTS])
def variant(request, knobs, K):
    assert K.gemm_variant_built(request.param)
    knobs.setenv("VP_GEMM_VARIANT", request.param)
    return request.param


# ------------------------------------------------------------------------------------------------------------------
# integer-valued operands: indexing and the rounding chains
# ------------------------------------------------------------------------------------------------------------------

def test_main_loops(K, variant):
    run_cases(K, plain(G.main_loop_cases()), tag=f"v{variant} ")


def test_main_loops_gated(K, variant):
    run_cases(K, gated(G.main_loop_cases()), tag=f"v{variant} ")


def test_row_and_column_edges(K):
    run_cases(K, G.row_col_cases())


def test_gated(K):
    run_cases(K, G.gated_cases())


def test_addrows(K):
    run_cases(K, G.addrows_cases())


def test_splitk(K):
    run_cases(K, plain(G.splitk_cases()))


def test_splitk_gated(K):
    run_cases(K, gated(G.splitk_cases()))


@pytest.mark.parametrize("i", range(3), ids=["bias", "gated_inject", "gelu_aux"])
def test_tail_mode(K, i):
    run_cases(K, [G.tail_cases()[i]])


def test_a_tail(K):
    run_cases(K, plain(G.a_tail_cases()))


def test_a_tail_gated(K):
    run_cases(K, gated(G.a_tail_cases()))


def test_qknorm_rope(K, variant):
    cases = G.qknorm_cases()
    if variant == "11":
        # the A/B loop 11 is built without the aux instances: where it would run (whole K-tiles, at least 8 of them)
        # the launch is VP_ERR_UNSUPPORTED and nothing runs; the other K fall to loops 1 / 5 as for every variant
        no11 = [c for c in cases if c.aux and c.K % 64 == 0 and c.K >= 512]
        assert no11
        for c in no11:
            with pytest.raises(RuntimeError, match="VP_ERR_UNSUPPORTED"):
                launch(K, c, G.inputs(c))
        cases = [c for c in cases if c not in no11]
    run_cases(K, cases, tag=f"v{variant} ")


def test_two_segments_of_n_seg_12_are_rejected(K):
    """n_seg % 8 == 4 with two segments has N % 8 == 0, but an 8-row weight block of the DMA and an 8-column chunk
    of the split-K reduce would straddle the segment boundary: VP_ERR_ARG from both entry points (include/vp_hip.h),
    before anything is launched; the output stays untouched."""
    from videopainter_amd import _native as N
    M, Kk, n_seg = 37, 1024, 12
    o = G.exact_operands(M, Kk, n_seg, 2, 1, 0.25, 4.0)
    a, ws, bs = o.a.to(dev), [w.to(dev) for w in o.w], [b.to(dev) for b in o.bias]
    out = _sent(M, 2 * n_seg)
    d = N.GemmDesc()
    d.M, d.N, d.K, d.epilogue, d.n_seg = M, 2 * n_seg, Kk, N.EPI_BIAS, n_seg
    d.A, d.lda, d.C, d.ldc, d.rows_per_group = a.data_ptr(), Kk, out.data_ptr(), 2 * n_seg, M
    for s in range(2):
        d.W[s], d.bias[s] = ws[s].data_ptr(), bs[s].data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    assert N.lib().vp_gemm_bf16(C.byref(d), stream) == N.ERR_ARG
    nb = N.lib().vp_gemm_bf16_workspace_bytes(C.byref(d))
    assert nb > 0  # the split-K reduce would run
    wsb = torch.empty(nb, device=dev, dtype=torch.uint8)
    assert N.lib().vp_gemm_bf16_ws(C.byref(d), wsb.data_ptr(), nb, stream) == N.ERR_ARG
    with pytest.raises(RuntimeError, match="VP_ERR_ARG"):
        K.gemm(a, ws, bs, out)
    torch.cuda.synchronize()
    assert bool((out == G.SENT).all())
    # the neighbouring legal shape (n_seg = 16) on the same path is bit-equal to its reference
    run_cases(K, [G.case("splitk bias 2 x 16", G.BIAS, M, Kk, 16, nsegs=2, ws="split", seed=2)])
    print("  2 segments of n_seg = 12: VP_ERR_ARG from vp_gemm_bf16 and vp_gemm_bf16_ws")


# ------------------------------------------------------------------------------------------------------------------
# MX-FP8
# ------------------------------------------------------------------------------------------------------------------

def _mx(K, x):
    """an MXTensor of the host quantiser's bytes, after asserting that they dequantise to x exactly"""
    q, s = mx_ref.quantize(x)
    assert torch.equal(mx_ref.dequantize(q, s, x.shape[0], x.shape[1]), x.float())
    t = K.MXTensor(x.shape[0], x.shape[1], dev)
    assert t.scales.numel() == s.numel()
    t.q[:x.shape[0]] = q.to(dev)
    t.scales.copy_(s.to(dev))
    return t


def launch_mx(K, c, t):
    """one vp_gemm_mx_fp8 launch of case c"""
    from videopainter_amd import _native as N
    keep = []
    cbuf, abuf = _buffers(c)
    x = N.GemmMxDesc()
    d = x.base
    fill_desc(K, d, c, t, cbuf, abuf, keep)
    am = _mx(K, t.ops.a)
    d.A, d.lda, x.a_scale = am.q.data_ptr(), am.q.stride(0), am.scales.data_ptr()
    for s, w in enumerate(t.ops.w):
        keep.append(_mx(K, w))
        d.W[s], x.w_scale[s] = keep[-1].q.data_ptr(), keep[-1].scales.data_ptr()
    if c.epi == G.GELU_MX:  # C is MX-quantised (not compared); aux = z
        out = K.MXTensor(c.M, c.N, dev)
        d.C, d.ldc, x.c_scale = out.q.data_ptr(), out.q.stride(0), out.scales.data_ptr()
    N.check(N.lib().vp_gemm_mx_fp8(C.byref(x), _stream()), "vp_gemm_mx_fp8")
    torch.cuda.synchronize()
    return cbuf.cpu(), None if abuf is None else abuf.cpu()


@pytest.mark.parametrize("loop", ["13", "5"], ids=["gemm8_v13", "gemm8_v5"])
def test_mx_fp8(K, loop, knobs):
    knobs.setenv("VP_GEMM8_VARIANT", loop)
    run_cases(K, plain(G.mx_cases()), fn=launch_mx, tag=f"gemm8 v{loop} ")


@pytest.mark.parametrize("loop", ["13", "5"], ids=["gemm8_v13", "gemm8_v5"])
def test_mx_fp8_gated(K, loop, knobs):
    knobs.setenv("VP_GEMM8_VARIANT", loop)
    run_cases(K, gated(G.mx_cases()), fn=launch_mx, tag=f"gemm8 v{loop} ")


# ------------------------------------------------------------------------------------------------------------------
# accumulation precision, real-valued operands (VP_EPI_BIAS)
# ------------------------------------------------------------------------------------------------------------------

def _accum(K, name, M, N, Kk, seed, split=False):
    """split=False: vp_gemm_bf16 itself, so that the main loop under test sums the whole K range"""
    from videopainter_amd import _native as NAT
    a, w, b = G.accum_case(M, N, Kk, seed)
    out = _sent(M + G.GUARD, N)
    ad, wd, bd = a.to(dev), w.to(dev), b.to(dev)
    if split:
        K.gemm(ad, [wd], [bd], out[:M])
    else:
        d = NAT.GemmDesc()
        d.M, d.N, d.K, d.epilogue, d.n_seg, d.rows_per_group = M, N, Kk, G.BIAS, N, M
        d.A, d.lda, d.C, d.ldc = ad.data_ptr(), Kk, out.data_ptr(), N
        d.W[0], d.bias[0] = wd.data_ptr(), bd.data_ptr()
        NAT.check(NAT.lib().vp_gemm_bf16(C.byref(d), _stream()), "vp_gemm_bf16")
    torch.cuda.synchronize()
    y64, allowed = G.accum_bound(a, w, b)
    got = out.cpu()
    assert bool((got[M:] == G.SENT).all())
    g64 = got[:M].double()
    assert bool(torch.isfinite(g64).all())
    ratio = R.worst_ratio((g64 - y64).abs(), allowed)
    print(f"  {name}: worst error / allowed = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio}"


@pytest.mark.parametrize("Kk", G.ACCUM_KS)
def test_accumulation_real_operands(K, variant, Kk):
    _accum(K, f"v{variant} accum 300 x 264 x {Kk}", 300, 264, Kk, 400 + Kk)


def test_accumulation_real_operands_splitk_and_tail(K):
    c = SimpleNamespace(M=37, N=264, K=2560, epi=G.BIAS, n_seg=264, lda=2560, a_tail=None)
    assert workspace_bytes(c) > 0
    _accum(K, "split-K accum 37 x 264 x 2560", 37, 264, 2560, 410, split=True)
    c = SimpleNamespace(M=4352, N=4096, K=1024, epi=G.BIAS, n_seg=4096, lda=1024, a_tail=None)
    assert workspace_bytes(c) >= 16 * 2 * 256 * 256 * 4
    _accum(K, "tail-mode accum 4352 x 4096 x 1024", 4352, 4096, 1024, 411, split=True)


# ------------------------------------------------------------------------------------------------------------------
# vp_head_norm_rope_bf16 forward
# ------------------------------------------------------------------------------------------------------------------

def _head_check(name, got, r):
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    ratio = R.worst_ratio((got - r["y"]).abs(), G.head_allowed(r))
    print(f"  {name}: worst error / allowed = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: error / allowed = {ratio}"


def _rope_dev(c):
    if c["rope"] is None:
        return None
    return tuple(t.to(dev)[:c["rope_rows"]] for t in c["rope"])


@pytest.mark.parametrize("H,T,kind", R.HEAD_CASES)
def test_head_norm_rope_fwd(K, H, T, kind):
    """q and k slices of a fused [B, N, 3 H 64] buffer, strided in and out (the other slices of the output buffer keep
    their sentinels), then in place."""
    c = R.head_case(H, T, kind)
    D = H * 64
    lw, lb = c["lw"].to(dev), c["lb"].to(dev)
    qkv = c["qkv"].to(dev)
    for which in (0, 1):
        sl = slice(which * D, (which + 1) * D)
        x, _, rope = R.head_operands(c, H, which)
        r = G.head_norm_rope_ref(x, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope)
        tag = f"head_norm_rope H = {H} T = {T} {kind} {'qk'[which]}"
        out = torch.full_like(qkv, G.SENT)
        K.head_norm_rope(qkv[..., sl], out[..., sl], H, T, lw, lb, R.HEAD_EPS, _rope_dev(c))
        _head_check(tag + " strided", out[..., sl], r)
        keep = torch.ones(3 * D, dtype=torch.bool)
        keep[sl] = False
        assert bool((out[..., keep.to(dev)] == G.SENT).all())
        buf = qkv.clone()
        K.head_norm_rope(buf[..., sl], buf[..., sl], H, T, lw, lb, R.HEAD_EPS, _rope_dev(c))
        _head_check(tag + " in place", buf[..., sl], r)
        assert torch.equal(buf[..., keep.to(dev)], qkv[..., keep.to(dev)])


def test_head_norm_rope_fwd_mask_and_dst_rows(K):
    H, T, kind = 3, 8, "rope"
    c = R.head_case(H, T, kind)
    B, N, D = R.HEAD_B, c["N"], H * 64
    lw, lb = c["lw"].to(dev), c["lb"].to(dev)
    qkv = c["qkv"].to(dev)
    x, _, rope = R.head_operands(c, H, 1)
    mask = G.head_fwd_mask(B, N)
    assert bool((mask[:, :T] == 0).any()) and bool((mask[:, T:] == 0).any()) and bool((mask != 0).any())
    r = G.head_norm_rope_ref(x, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope, mask=mask, pre_scale=0.5)
    out = _sent(B * N + G.GUARD, D)
    o3 = out[:B * N].view(B, N, D)
    K.head_norm_rope(qkv[..., D:2 * D], o3, H, T, lw, lb, R.HEAD_EPS, _rope_dev(c), tok_mask=mask.to(dev),
                     pre_scale=0.5)
    _head_check("head_norm_rope tok_mask pre_scale = 0.5", o3, r)
    # a zeroed row is the LayerNorm bias exactly: the bias's bits on text rows, and on video rows the bits of its
    # rotation in the kernel's fp32 order (gemm_refs.rot_bias_bits), whatever the batch and the head
    got = o3.cpu()
    zero = (mask == 0)
    zero_text, zero_video = zero.clone(), zero.clone()
    zero_text[:, T:] = False
    zero_video[:, :T] = False
    assert int(zero_text.sum()) > 0 and int(zero_video.sum()) > 0
    assert torch.equal(got[zero_text], c["lb"].repeat(H).expand(int(zero_text.sum()), D))
    rot = G.rot_bias_bits(c["lb"], H, rope)  # [Nv, D]
    want = rot[None].expand(B, N - T, D)[zero_video[:, T:]]
    assert torch.equal(got[zero_video].float(), want.float()), "zeroed video rows are not the rotated bias's bits"
    print(f"  head_norm_rope tok_mask: {int(zero_text.sum())} zeroed text rows = the bias, {int(zero_video.sum())} "
          f"zeroed video rows = the rotated bias, bit-equal")
    assert bool((out[B * N:] == G.SENT).all())
    # dst_rows: a permutation of the kept rows, the others negative (neither read nor written)
    g = torch.Generator().manual_seed(6)
    dst = torch.full((B, N), -1, dtype=torch.int32)
    for b in range(B):
        kept = (torch.rand(N, generator=g) > 0.3).nonzero().flatten()
        dst[b, kept] = torch.randperm(len(kept), generator=g).to(torch.int32)
    assert bool((dst < 0).any())
    r = G.head_norm_rope_ref(x, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope)
    out = _sent(B * N + G.GUARD, D)
    o3 = out[:B * N].view(B, N, D)
    K.head_norm_rope(qkv[..., D:2 * D], o3, H, T, lw, lb, R.HEAD_EPS, _rope_dev(c), dst_rows=dst.to(dev))
    got = o3.cpu()
    perm = {k: torch.zeros(B, N, D, dtype=torch.float64) for k in ("y", "mag", "E")}
    written = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        src = (dst[b] >= 0).nonzero().flatten()
        to = dst[b, src].long()
        written[b, to] = True
        for k in perm:
            perm[k][b, to] = r[k][b, src]
    _head_check("head_norm_rope dst_rows", got[written], {k: v[written] for k, v in perm.items()})
    assert bool((got[~written] == G.SENT).all()) and bool((out[B * N:] == G.SENT).all())


# ------------------------------------------------------------------------------------------------------------------
# the AdaLN modulation's chain bit for bit (rows whose LayerNorm is exact)
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", G.ADALN_EXACT_DS)
def test_adaln_modulation_chain_bit_exact(K, D):
    c = G.adaln_exact_case(D)
    B, N = G.ADALN_EXACT_B, G.ADALN_EXACT_N
    d = {k: v.to(dev) for k, v in c.items()}
    for T in (0, 5, N):
        out = _sent(B * N + G.GUARD, D)
        K.adaln_modulate(d["x"], d["lw"], d["lb"], d["mod"], T, G.ADALN_EXACT_EPS, out=out[:B * N].view(B, N, D))
        want = torch.cat([G.adaln_exact_ref(c, T), torch.full((G.GUARD, D), G.SENT, dtype=BF)])
        G.check_output(f"adaln_modulate exact rows D = {D} T = {T}", SimpleNamespace(buf=want, ref=None), out)
    ones, zeros = torch.ones(D, device=dev, dtype=BF), torch.zeros(D, device=dev, dtype=BF)
    for T in (0, 5):
        rows = B * (N - T)
        out = _sent(rows + G.GUARD, D)
        K.final_norm(d["x"], T, ones, zeros, d["lw"], d["lb"], G.ADALN_EXACT_EPS, d["mod"][:, :2 * D],
                     out=out[:rows].view(B, N - T, D))
        want = torch.cat([G.adaln_exact_ref(c, T, final=True), torch.full((G.GUARD, D), G.SENT, dtype=BF)])
        G.check_output(f"final_norm exact rows D = {D} T = {T}", SimpleNamespace(buf=want, ref=None), out)
