"""The MX-FP8 kernels of the training step through frozen fp8 blocks (GPU only): the row-scale that writes MX rows,
the FF1 GEMM's aux output (the pre-activation z beside the MX GELU output) and the FF2 dgrad epilogue
EPI_GELU_BWD_MXFP8 — each byte for byte against the composition of existing kernels it replaces, and the dgrad's
values against the host reference `tests/mx_ref.py`.

Shapes: M = 592 rows as B = 2 x 296 tokens with 8 text tokens (two full 256-row tiles and an 80-row tail, the batch
boundary inside the second tile); widths 256 and 1024: K = 256 is 2 K-steps (main loop 5 whatever the knob says),
K = 1024 is 8 K-steps (main loop 13 unless VP_GEMM8_VARIANT=5)."""
import ctypes as C

import pytest
import torch

from tests import mx_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
BT, NTOK, T = 2, 296, 8
M = BT * NTOK
VP_ERR_ARG = 1000


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videopainter_amd import _native
    _native.lib()


@pytest.fixture(params=["5", "13"], ids=["gemm8_v5", "gemm8_v13"])
def gemm8_variant(request, knobs):
    """fp8 GEMM main loop, as tests/test_mx_gpu.py parametrises it."""
    knobs.setenv("VP_GEMM8_VARIANT", request.param)
    return request.param


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _operands(Kk, Nn, seed):
    """(a, w, bias, z) bf16 on the device: a [M, K] with block magnitudes over a few octaves, w [N, K], z [M, N] a
    pre-activation spread over GELU's curved range and its two flat ends."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, Kk, generator=g) * (2.0 ** torch.randint(-3, 4, (M, Kk // 32), generator=g)
                                           ).repeat_interleave(32, dim=1)
    w = torch.randn(Nn, Kk, generator=g) * Kk ** -0.5
    b = torch.randn(Nn, generator=g) * 0.1
    z = torch.randn(M, Nn, generator=g) * 3.0
    return tuple(t.to(torch.bfloat16).to(dev) for t in (a, w, b, z))


def _same_mx(a, b):
    assert torch.equal(a.q[:a.rows], b.q[:b.rows])
    assert torch.equal(a.scales, b.scales)


@pytest.mark.parametrize("D", [256, 1024])
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row_stride"])
def test_rowscale_mx_equals_quantised_rowscale(D, strided):
    """q bytes and scale bytes equal mx_quantize(rowscale(x)); also with x the columns of a wider buffer."""
    from videopainter_amd import kernels as K
    g = torch.Generator().manual_seed(D)
    buf = (torch.randn(M, D + 64 if strided else D, generator=g) * 4).to(torch.bfloat16).to(dev)
    x = buf[:, :D]
    mod = (torch.randn(BT, 6 * D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    mod[0, 2 * D:2 * D + 32] = 0  # an all-zero block (video rows of batch 0)
    y = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    K.rowscale(x, y, NTOK, T, mod, 2, 5)
    want = K.mx_quantize(y)
    got = K.rowscale_mx(x, NTOK, T, mod, 2, 5, out=K.MXTensor(M, D, dev))
    _same_mx(got, want)
    # and the host quantiser, so the pair cannot be wrong together
    q_ref, s_ref = R.quantize(y.cpu())
    assert torch.equal(got.q[:M].cpu(), q_ref)
    assert torch.equal(got.scales.cpu(), s_ref)


@pytest.mark.parametrize("Kk,Nn", [(256, 1024), (1024, 256)])
def test_ff1_aux_is_bias_output_and_leaves_mx_bytes(Kk, Nn, gemm8_variant):
    """EPI_BIAS_GELU_MXFP8 with aux: the MX bytes are those without aux (the GELU moved to the row pass, on the bf16 z
    it stores), and aux is torch.equal to EPI_BIAS of the same operands."""
    from videopainter_amd import kernels as K
    from videopainter_amd import _native as N
    a, w, b, _ = _operands(Kk, Nn, 11 + Kk)
    A, W = K.mx_quantize(a), K.mx_quantize(w)
    plain = K.gemm_mx(A, [W], [b], K.MXTensor(M, Nn, dev), epilogue=N.EPI_BIAS_GELU_MXFP8)
    # aux as the first columns of a wider buffer, poisoned: the store keeps to its N columns and M rows
    auxbuf = torch.full((M + 3, Nn + 8), 7.0, device=dev, dtype=torch.bfloat16)
    aux = auxbuf[:M, :Nn]
    with_aux = K.gemm_mx(A, [W], [b], K.MXTensor(M, Nn, dev), epilogue=N.EPI_BIAS_GELU_MXFP8, aux=aux)
    _same_mx(with_aux, plain)
    z = torch.empty(M, Nn, device=dev, dtype=torch.bfloat16)
    K.gemm_mx(A, [W], [b], z)
    assert torch.equal(aux, z)
    assert bool((auxbuf[M:] == 7.0).all()) and bool((auxbuf[:, Nn:] == 7.0).all())


@pytest.mark.parametrize("Kk,Nn", [(256, 1024), (1024, 256)])
def test_gelu_bwd_mx_equals_composition_and_host(Kk, Nn, gemm8_variant):
    """EPI_GELU_BWD_MXFP8 == mx_quantize(gelu_bwd(gemm_mx(EPI_BIAS, no bias), z)) byte for byte; its values against
    the float64 product of the dequantised operands times gelu'(z), to the MX-output tolerance of
    tests/test_mx_gpu.py::test_gemm_mx_gelu_to_mx_and_gated (4e-2: one e4m3 re-quantisation of the result)."""
    from videopainter_amd import kernels as K
    from videopainter_amd import _native as N
    a, w, _, z = _operands(Kk, Nn, 23 + Kk)
    A, W = K.mx_quantize(a), K.mx_quantize(w)
    got = K.gemm_mx(A, [W], [None], K.MXTensor(M, Nn, dev), epilogue=N.EPI_GELU_BWD_MXFP8, z=z)
    dh = torch.empty(M, Nn, device=dev, dtype=torch.bfloat16)
    K.gemm_mx(A, [W], [None], dh)
    want = K.mx_quantize(K.gelu_bwd(dh, z))
    _same_mx(got, want)
    zz = z.double().cpu().requires_grad_()
    torch.nn.functional.gelu(zz, approximate="tanh").sum().backward()
    ref = (R.dequantize(A.q, A.scales, M, Kk).double() @ R.dequantize(W.q, W.scales, Nn, Kk).double().T) * zz.grad
    r = rel(R.dequantize(got.q, got.scales, M, Nn), ref)
    print(f"gelu_bwd_mx K={Kk} N={Nn}: rel {r:.3e}")
    assert r < 4e-2


def _desc(epilogue, *, aux=False, z=True, c_scale=True):
    """A valid vp_gemm_mx_desc of the M x 256 x 256 product (and what must stay alive), minus what a case drops."""
    from videopainter_amd import kernels as K
    from videopainter_amd import _native as N
    a, w, _, zt = _operands(256, 256, 5)
    A, W = K.mx_quantize(a), K.mx_quantize(w)
    mx_out = epilogue in (N.EPI_BIAS_GELU_MXFP8, N.EPI_GELU_BWD_MXFP8)
    out = K.MXTensor(M, 256, dev) if mx_out else torch.empty(M, 256, device=dev, dtype=torch.bfloat16)
    auxt = torch.empty(M, 256, device=dev, dtype=torch.bfloat16)
    x = N.GemmMxDesc()
    d = x.base
    d.M, d.N, d.K, d.epilogue = M, 256, 256, epilogue
    d.A, d.lda, x.a_scale = A.q.data_ptr(), 256, A.scales.data_ptr()
    d.W[0], x.w_scale[0], d.n_seg, d.rows_per_group = W.q.data_ptr(), W.scales.data_ptr(), 256, M
    d.C, d.ldc = (out.q if mx_out else out).data_ptr(), 256
    if mx_out and c_scale:
        x.c_scale = out.scales.data_ptr()
    if aux:
        d.aux, d.ld_aux = auxt.data_ptr(), 256
    if epilogue == N.EPI_GELU_BWD_MXFP8 and z:
        d.R, d.ldr = zt.data_ptr(), 256
    return x, (A, W, out, auxt, zt)


def test_argument_errors():
    """aux with another epilogue, a missing Z (R) and a missing c_scale are VP_ERR_ARG (nothing is launched)."""
    from videopainter_amd import _native as N
    L = N.lib()
    s = torch.cuda.current_stream().cuda_stream
    ok = [_desc(N.EPI_BIAS_GELU_MXFP8, aux=True), _desc(N.EPI_GELU_BWD_MXFP8)]
    bad = [_desc(N.EPI_BIAS, aux=True), _desc(N.EPI_GATED, aux=True), _desc(N.EPI_GELU_BWD_MXFP8, aux=True),
           _desc(N.EPI_GELU_BWD_MXFP8, z=False), _desc(N.EPI_GELU_BWD_MXFP8, c_scale=False),
           _desc(N.EPI_BIAS_GELU_MXFP8, aux=True, c_scale=False), _desc(N.EPI_GELU_BWD), _desc(9)]
    for x, _alive in ok:
        assert L.vp_gemm_mx_fp8(C.byref(x), s) == 0
    for x, _alive in bad:
        assert L.vp_gemm_mx_fp8(C.byref(x), s) == VP_ERR_ARG
    x, _alive = _desc(N.EPI_BIAS_GELU_MXFP8, aux=True)
    x.base.ld_aux = 128  # narrower than N
    assert L.vp_gemm_mx_fp8(C.byref(x), s) == VP_ERR_ARG
    x, _alive = _desc(N.EPI_GELU_BWD_MXFP8)
    x.base.ldr = 260  # not a multiple of 8
    assert L.vp_gemm_mx_fp8(C.byref(x), s) == VP_ERR_ARG
    torch.cuda.synchronize()


def test_rowscale_mx_argument_errors():
    from videopainter_amd import kernels as K
    x = torch.zeros(M, 192, device=dev, dtype=torch.bfloat16)
    mod = torch.zeros(BT, 6 * 256, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        K.rowscale_mx(x, NTOK, T, mod, 2, 5)  # D % 128
    x = torch.zeros(M, 256, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        K.rowscale_mx(x, NTOK, T, mod, 2, 6)  # a chunk past mod's width
    with pytest.raises(ValueError):
        K.rowscale_mx(x, NTOK, T, mod, 2, 5, out=K.MXTensor(M, 512, dev))
