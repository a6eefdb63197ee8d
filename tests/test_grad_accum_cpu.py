"""fp32 gradient accumulation without a GPU: the host-side argument checks of the new entry points (ABI 30), the
wrappers' checks, and what is exported."""
import ctypes as C

import pytest
import torch

from videopainter_amd import _native as N

VP_ERR_ARG = 1000


def test_abi_and_struct_sizes():
    L = N.lib()  # (checks the struct sizes against the library's)
    assert L.vp_abi_version() >= 30 and N.ABI_VERSION >= 30
    assert C.sizeof(N.MtTensor) == 32 and C.sizeof(N.MtChunk) == 8  # the tables the folds run over: unchanged
    assert C.sizeof(N.OptimScalars) == 32 and C.sizeof(N.ProdigyScalars) == 56 and C.sizeof(N.ZeroRange) == 16
    for name in ("vp_mt_accumulate_bf16", "vp_mt_grad_sqnorm_f32", "vp_mt_adamw_f32", "vp_mt_adam_f32",
                 "vp_mt_prodigy_moments_f32"):
        assert name in N.EXPORTS and hasattr(L, name), name


def test_accumulate_rejects_bad_arguments_without_a_gpu():
    L = N.lib()
    p = 4096  # a non-null "pointer": every call below must return before any launch
    acc = L.vp_mt_accumulate_bf16
    assert acc(None, None, 1, p, 64, 1, 1.0, 0, None) == VP_ERR_ARG  # NULL tables with work to do
    assert acc(p, None, 1, p, 64, 1, 1.0, 0, None) == VP_ERR_ARG
    assert acc(None, p, 1, p, 64, 1, 1.0, 0, None) == VP_ERR_ARG
    assert acc(p, p, 1, None, 64, 1, 1.0, 0, None) == VP_ERR_ARG  # NULL accumulator
    assert acc(p, p, -1, p, 64, 1, 1.0, 0, None) == VP_ERR_ARG
    assert acc(p, p, 1, p, -8, 1, 1.0, 0, None) == VP_ERR_ARG
    for scale in (0.0, -0.5, float("inf"), float("nan")):
        assert acc(p, p, 1, p, 64, 0, scale, 0, None) == VP_ERR_ARG, scale
        assert acc(None, None, 0, None, 0, 0, scale, 0, None) == VP_ERR_ARG, scale  # (even with nothing to do)
    assert acc(None, None, 0, None, 0, 1, 1.0, 0, None) == 0  # empty work is accepted without a launch
    assert acc(None, None, 0, p, 64, 0, 0.125, 1, None) == 0


def test_f32_gradient_passes_reject_bad_arguments_without_a_gpu():
    L = N.lib()
    p = 4096
    norm = L.vp_mt_grad_sqnorm_f32
    assert norm(None, None, 1, p, p, p, None) == VP_ERR_ARG
    assert norm(p, p, 1, None, p, p, None) == VP_ERR_ARG  # NULL accumulator
    assert norm(p, p, 1, p, None, p, None) == VP_ERR_ARG
    assert norm(p, p, 1, p, p, None, None) == VP_ERR_ARG
    assert norm(p, p, -1, p, p, p, None) == VP_ERR_ARG
    assert norm(None, None, 0, None, None, None, None) == 0
    for entry in (L.vp_mt_adamw_f32, L.vp_mt_adam_f32):
        adam = lambda *a, lr=1e-5, b1=0.9, b2=0.95, eps=1e-8, wd=1e-4: entry(  # noqa: E731
            *a, lr, b1, b2, eps, wd, 1, None)
        assert adam(None, None, 0, 1, p, p, p, p, p) == VP_ERR_ARG
        assert adam(p, p, 0, 1, None, p, p, p, p) == VP_ERR_ARG  # NULL accumulator
        assert adam(p, p, 0, 1, p, None, p, p, p) == VP_ERR_ARG
        assert adam(p, p, 0, 1, p, p, None, p, p) == VP_ERR_ARG
        assert adam(p, p, 0, 1, p, p, p, None, p) == VP_ERR_ARG
        assert adam(p, p, 0, 1, p, p, p, p, None) == VP_ERR_ARG
        assert adam(p, p, -1, 1, p, p, p, p, p) == VP_ERR_ARG
        assert adam(p, p, 0, -1, p, p, p, p, p) == VP_ERR_ARG
        assert adam(p, p, 0, 1, p, p, p, p, p, lr=-1.0) == VP_ERR_ARG
        assert adam(p, p, 0, 1, p, p, p, p, p, b1=1.0) == VP_ERR_ARG
        assert adam(p, p, 0, 1, p, p, p, p, p, eps=float("nan")) == VP_ERR_ARG
        assert adam(None, None, 0, 0, p, p, p, p, p) == 0
    mom = lambda *a, b1=0.9, b2=0.95, b3=0.97, wd=0.0, d0=1e-6: L.vp_mt_prodigy_moments_f32(  # noqa: E731
        *a, b1, b2, b3, wd, d0, 0, 1, None)
    ok = [p, p, 0, 1, p, p, p, p, p, p, p, p, p]  # tensors chunks begin n acc master p0 m v s partials scalars dstate
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        bad = list(ok)
        bad[i] = None
        assert mom(*bad) == VP_ERR_ARG, i
    assert mom(p, p, -1, 1, *ok[4:]) == VP_ERR_ARG
    assert mom(p, p, 0, -1, *ok[4:]) == VP_ERR_ARG
    assert mom(*ok, b3=1.0) == VP_ERR_ARG
    assert mom(*ok, d0=0.0) == VP_ERR_ARG
    assert mom(None, None, 0, 0, *ok[4:10], None, p, p) == 0


def test_wrappers_check_dtype_shape_length_and_device():
    from videopainter_amd import kernels as K
    f = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt)  # noqa: E731
    tab = torch.zeros(64, dtype=torch.uint8)
    sc, ds = torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.float64)
    with pytest.raises(TypeError, match="acc must be torch.float32"):
        K.mt_accumulate(tab, tab, 1, f(16, torch.bfloat16), first=True)
    with pytest.raises(ValueError, match="contiguous 1-D"):
        K.mt_accumulate(tab, tab, 1, torch.zeros(4, 4), first=True)
    with pytest.raises(ValueError, match="device tensor"):
        K.mt_accumulate(tab, tab, 1, f(16), first=True)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            K.mt_accumulate(tab, tab, 1, f(16), first=False, scale=scale)
    with pytest.raises(TypeError, match="acc must be torch.float32"):
        K.mt_grad_sqnorm_f32(tab, tab, 1, f(16, torch.float64), f(4), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="device tensor"):
        K.mt_grad_sqnorm_f32(tab, tab, 1, f(16), f(4), torch.zeros(4, dtype=torch.int32))
    hyper = dict(lr=1e-5, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, use_clip=False)
    for fn in (K.mt_adamw_f32, K.mt_adam_f32):
        with pytest.raises(TypeError, match="exp_avg must be torch.float32"):
            fn(tab, tab, 0, 1, f(16), f(16), f(16, torch.bfloat16), f(16), sc, **hyper)
        with pytest.raises(ValueError, match="master must have the accumulator's length 16"):
            fn(tab, tab, 0, 1, f(16), f(24), f(16), f(16), sc, **hyper)
        with pytest.raises(ValueError, match="device tensor"):
            fn(tab, tab, 0, 1, f(16), f(16), f(16), f(16), sc, **hyper)
    mom = dict(betas=(0.9, 0.95), beta3=0.97, weight_decay=0.0, d0=1e-6, safeguard_warmup=False, use_clip=False)
    with pytest.raises(ValueError, match="s must have the accumulator's length 16"):
        K.mt_prodigy_moments_f32(tab, tab, 0, 1, f(16), f(16), f(16), f(16), f(16), f(8), f(4), sc, ds, **mom)
    with pytest.raises(TypeError, match="p0 must be torch.float32"):
        K.mt_prodigy_moments_f32(tab, tab, 0, 1, f(16), f(16), f(16, torch.float16), f(16), f(16), f(16), f(4), sc, ds,
                                 **mom)


def test_public_names():
    import videopainter_amd as V
    from videopainter_amd import kernels as K
    for name in ("mt_accumulate", "mt_grad_sqnorm_f32", "mt_adamw_f32", "mt_adam_f32", "mt_prodigy_moments_f32"):
        assert callable(getattr(K, name)), name
    for cls in (V.FusedAdamW, V.FusedAdam, V.FusedProdigy, V.ShardedFusedAdamW, V.ShardedFusedAdam,
                V.ShardedFusedProdigy):
        for name in ("accumulate", "reset_accumulation"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
        for name in ("pending", "grad_accumulator"):
            assert isinstance(getattr(cls, name), property), (cls.__name__, name)
