"""Prodigy and plain Adam (videopainter_amd/optim.py, csrc/prodigy.hip, csrc/optim.hip) — the parts that need no GPU:
host-side argument validation of the new C entry points, the constructors' validation, the exported names and the
d block's layout."""
import ctypes as C

import pytest
import torch

from videopainter_amd import _native as N
from videopainter_amd.optim import FusedAdam, FusedProdigy

VP_ERR_ARG = 1000
NAN, INF = float("nan"), float("inf")
P = 4096  # a non-null "pointer": every call below must return before any launch


def _finalize(L, phase=1, partials=P, n=1, lr=1.0, b1=0.9, b2=0.95, b3=0.97, d0=1e-6, d_coef=1.0, growth=INF,
              scalars=P, dstate=P):
    return L.vp_prodigy_finalize(phase, partials, n, lr, b1, b2, b3, d0, d_coef, growth, 0, scalars, dstate, None)


def _moments(L, tensors=P, chunks=P, c0=0, n=1, master=P, p0=P, m=P, v=P, s=P, partials=P, scalars=P, dstate=P,
             b1=0.9, b2=0.95, b3=0.97, wd=0.0, d0=1e-6):
    return L.vp_mt_prodigy_moments_bf16(tensors, chunks, c0, n, master, p0, m, v, s, partials, scalars, dstate, b1, b2,
                                        b3, wd, d0, 0, 1, None)


def _update(L, tensors=P, chunks=P, c0=0, n=1, master=P, m=P, v=P, scalars=P, dstate=P, eps=1e-8, wd=1e-4):
    return L.vp_mt_prodigy_update_bf16(tensors, chunks, c0, n, master, m, v, scalars, dstate, eps, wd, 0, None)


def _adam(L, tensors=P, chunks=P, c0=0, n=1, master=P, m=P, v=P, scalars=P, lr=1e-5, b1=0.9, b2=0.95, eps=1e-8,
          wd=1e-4):
    return L.vp_mt_adam_bf16(tensors, chunks, c0, n, master, m, v, scalars, lr, b1, b2, eps, wd, 1, 0, None)


def test_finalize_rejects_bad_arguments_without_a_gpu():
    L = N.lib()
    for kw in (dict(phase=2), dict(phase=-1), dict(scalars=None), dict(dstate=None), dict(partials=None),
               dict(n=-1), dict(lr=-1.0), dict(lr=NAN), dict(lr=INF), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.5),
               dict(b2=NAN), dict(b3=1.0), dict(b3=NAN), dict(b3=-0.5), dict(d0=0.0), dict(d0=-1e-6), dict(d0=NAN),
               dict(d0=INF), dict(d_coef=0.0), dict(d_coef=-1.0), dict(d_coef=NAN), dict(growth=0.5),
               dict(growth=NAN), dict(growth=-INF)):
        assert _finalize(L, **kw) == VP_ERR_ARG, kw
    assert _finalize(L, phase=0, scalars=None) == VP_ERR_ARG
    assert _finalize(L, phase=0, d0=0.0) == VP_ERR_ARG


def test_passes_reject_bad_arguments_without_a_gpu():
    L = N.lib()
    for kw in (dict(tensors=None), dict(chunks=None), dict(master=None), dict(p0=None), dict(m=None), dict(v=None),
               dict(s=None), dict(partials=None), dict(scalars=None), dict(dstate=None), dict(c0=-1), dict(n=-1),
               dict(b1=1.0), dict(b2=-0.1), dict(b2=NAN), dict(b3=1.0), dict(b3=NAN), dict(wd=-1.0), dict(wd=NAN),
               dict(d0=0.0), dict(d0=-1.0), dict(d0=NAN)):
        assert _moments(L, **kw) == VP_ERR_ARG, kw
    for kw in (dict(tensors=None), dict(chunks=None), dict(master=None), dict(m=None), dict(v=None),
               dict(scalars=None), dict(dstate=None), dict(c0=-1), dict(n=-1), dict(eps=-1.0), dict(eps=NAN),
               dict(wd=-1.0), dict(wd=NAN)):
        assert _update(L, **kw) == VP_ERR_ARG, kw
    for kw in (dict(tensors=None), dict(chunks=None), dict(master=None), dict(m=None), dict(v=None),
               dict(scalars=None), dict(c0=-1), dict(n=-1), dict(lr=-1.0), dict(lr=NAN), dict(b1=1.0), dict(b2=1.5),
               dict(eps=NAN), dict(eps=-1.0), dict(wd=-1.0), dict(wd=NAN)):
        assert _adam(L, **kw) == VP_ERR_ARG, kw


def test_empty_lists_are_accepted_without_a_launch():
    L = N.lib()
    assert _moments(L, tensors=None, chunks=None, n=0, partials=None) == 0
    assert _update(L, tensors=None, chunks=None, n=0) == 0
    assert _adam(L, tensors=None, chunks=None, n=0) == 0


def test_wrappers_check_their_tensors():
    """kernels.py refuses host tensors, wrong dtypes and a d block / pair workspace that is too small."""
    from videopainter_amd import kernels as K
    f32, i32s, blk = torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.float64)
    fin = dict(lr=1.0, betas=(0.9, 0.95), beta3=0.97, d0=1e-6, d_coef=1.0, growth_rate=INF, use_bias_correction=False)
    with pytest.raises(ValueError):
        K.prodigy_finalize(2, f32, 1, i32s, blk, **fin)
    with pytest.raises(ValueError):
        K.prodigy_finalize(0, None, 0, i32s, blk, **fin)  # host scalars
    with pytest.raises(ValueError):
        K.mt_prodigy_update(None, None, 0, 0, f32, f32, f32, i32s, blk, eps=1e-8, weight_decay=0.0, zero_grads=False)
    with pytest.raises(ValueError):
        K.mt_adam(None, None, 0, 0, f32, f32, f32, i32s, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0,
                  use_clip=False, zero_grads=False)


def test_d_block_matches_the_c_struct():
    L = N.lib()  # (compares every struct size with the library's, the d block's among them)
    sizes = (N.i64 * 15)()
    L.vp_struct_sizes(sizes)
    assert sizes[14] == C.sizeof(N.ProdigyScalars) == 56 and sizes[9] == C.sizeof(N.OptimScalars)
    assert [f[0] for f in N.ProdigyScalars._fields_[:6]] == ["d", "d_max", "d_hat", "d_numerator", "d_denom", "dlr"]
    assert N.ProdigyScalars.no_progress.offset == 48  # int32 slot 12 of the float64[7] tensor behind it
    assert L.vp_abi_version() >= 27


def _bf(*s):
    return torch.nn.Parameter(torch.zeros(*s, dtype=torch.bfloat16))


@pytest.mark.parametrize("cls", [FusedProdigy, FusedAdam])
def test_constructor_validation(cls):
    with pytest.raises(TypeError):
        cls([torch.nn.Parameter(torch.zeros(4))])  # fp32
    with pytest.raises(ValueError):
        cls([torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.bfloat16).t())])  # not contiguous
    with pytest.raises(ValueError):
        cls([])
    sp = _bf(4, 4)
    sp.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.ones(1, dtype=torch.bfloat16), (4, 4))
    with pytest.raises(ValueError):
        cls([sp])
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-1.0),
               dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            cls([_bf(4)], **kw)
    with pytest.raises(ValueError):
        cls([_bf(4)])  # valid dtype and layout, but not on a device: nothing is allocated for it


def test_prodigy_constructor_validation():
    for kw in (dict(d0=0.0), dict(d0=-1e-6), dict(d0=NAN), dict(d0=INF), dict(d_coef=0.0), dict(d_coef=-1.0),
               dict(d_coef=NAN), dict(growth_rate=0.99), dict(growth_rate=NAN), dict(beta3=1.0), dict(beta3=-0.1)):
        with pytest.raises(ValueError, match="Invalid"):
            FusedProdigy([_bf(4)], **kw)
    with pytest.raises(ValueError, match="same in every parameter group"):
        FusedProdigy([dict(params=[_bf(4)]), dict(params=[_bf(4)], lr=0.5)])
    with pytest.raises(ValueError, match="same in every parameter group"):
        FusedProdigy([dict(params=[_bf(4)]), dict(params=[_bf(4)], beta3=0.5)])


def test_public_names_are_exported():
    import videopainter_amd as V
    from videopainter_amd import optim
    assert V.FusedProdigy is optim.FusedProdigy and V.FusedAdam is optim.FusedAdam
    assert issubclass(V.FusedAdam, V.FusedAdamW) and issubclass(V.FusedProdigy, torch.optim.Optimizer)
    for name in ("vp_mt_adam_bf16", "vp_prodigy_finalize", "vp_mt_prodigy_moments_bf16", "vp_mt_prodigy_update_bf16"):
        assert name in N.EXPORTS
