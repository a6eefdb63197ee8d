"""Sharded Adam and Prodigy (videopainter_amd/zero.py, csrc/zero.hip) — the parts that need no GPU: host-side argument
validation of the new C entry points, the checks of their kernels.py wrappers, the constructors' validation and the
exported names.  (tests/test_abi.py compares the header with the binding and the library.)"""
import pytest
import torch

from videopainter_amd import _native as N

VP_ERR_ARG = 1000
NAN, INF = float("nan"), float("inf")
P = 4096  # a non-null "pointer": every call below must return before any launch


def _adam(L, ranges=P, r0=0, n=1, grad=P, master=P, m=P, v=P, param=P, per=64, scalars=P, lr=1e-5, b1=0.9, b2=0.95,
          eps=1e-8, wd=1e-4):
    return L.vp_zero_shard_adam(ranges, r0, n, grad, master, m, v, param, per, scalars, lr, b1, b2, eps, wd, 1, None)


def _moments(L, ranges=P, r0=0, n=1, grad=P, master=P, p0=P, m=P, v=P, s=P, per=64, partials=P, scalars=P, dstate=P,
             b1=0.9, b2=0.95, b3=0.97, wd=0.0, d0=1e-6):
    return L.vp_zero_shard_prodigy_moments(ranges, r0, n, grad, master, p0, m, v, s, per, partials, scalars, dstate,
                                           b1, b2, b3, wd, d0, 0, 1, None)


def _record(L, partials=P, n=1, scalars=P, record=P):
    return L.vp_zero_prodigy_record(partials, n, scalars, record, None)


def _finalize(L, phase=1, records=P, world=2, lr=1.0, b1=0.9, b2=0.95, b3=0.97, d0=1e-6, d_coef=1.0, growth=INF,
              scalars=P, dstate=P):
    return L.vp_zero_prodigy_finalize(phase, records, world, lr, b1, b2, b3, d0, d_coef, growth, 0, scalars, dstate,
                                      None)


def _update(L, ranges=P, r0=0, n=1, master=P, m=P, v=P, param=P, per=64, scalars=P, dstate=P, eps=1e-8, wd=1e-4):
    return L.vp_zero_shard_prodigy_update(ranges, r0, n, master, m, v, param, per, scalars, dstate, eps, wd, None)


def _unpack(L, tensors=P, chunks=P, n=1, flat=P, flat_len=64, scalars=P, dstate=P):
    return L.vp_zero_unpack_gated_bf16(tensors, chunks, n, flat, flat_len, scalars, dstate, None)


def test_shard_passes_reject_bad_arguments_without_a_gpu():
    L = N.lib()
    assert L.vp_abi_version() >= 29
    for kw in (dict(ranges=None), dict(grad=None), dict(master=None), dict(m=None), dict(v=None), dict(param=None),
               dict(scalars=None), dict(r0=-1), dict(n=-1), dict(per=-1), dict(lr=-1.0), dict(lr=NAN), dict(b1=1.0),
               dict(b2=1.5), dict(b2=NAN), dict(eps=-1.0), dict(eps=NAN), dict(wd=-1.0), dict(wd=NAN)):
        assert _adam(L, **kw) == VP_ERR_ARG, kw
    for kw in (dict(ranges=None), dict(grad=None), dict(master=None), dict(p0=None), dict(m=None), dict(v=None),
               dict(s=None), dict(partials=None), dict(scalars=None), dict(dstate=None), dict(r0=-1), dict(n=-1),
               dict(per=-1), dict(b1=1.0), dict(b1=-0.1), dict(b2=-0.1), dict(b2=NAN), dict(b3=1.0), dict(b3=NAN),
               dict(wd=-1.0), dict(wd=NAN), dict(d0=0.0), dict(d0=-1.0), dict(d0=NAN), dict(d0=INF)):
        assert _moments(L, **kw) == VP_ERR_ARG, kw
    for kw in (dict(ranges=None), dict(master=None), dict(m=None), dict(v=None), dict(param=None), dict(scalars=None),
               dict(dstate=None), dict(r0=-1), dict(n=-1), dict(per=-1), dict(eps=-1.0), dict(eps=NAN),
               dict(wd=-1.0), dict(wd=NAN)):
        assert _update(L, **kw) == VP_ERR_ARG, kw
    for kw in (dict(tensors=None), dict(chunks=None), dict(flat=None), dict(scalars=None), dict(dstate=None),
               dict(n=-3), dict(flat_len=-8)):
        assert _unpack(L, **kw) == VP_ERR_ARG, kw


def test_record_and_finalize_reject_bad_arguments_without_a_gpu():
    L = N.lib()
    for kw in (dict(partials=None), dict(scalars=None), dict(record=None), dict(n=-1)):
        assert _record(L, **kw) == VP_ERR_ARG, kw
    assert _record(L, partials=None, n=0, record=None) == VP_ERR_ARG  # an empty rank still needs its record
    for kw in (dict(phase=2), dict(phase=-1), dict(scalars=None), dict(dstate=None), dict(records=None),
               dict(world=0), dict(world=-2), dict(lr=-1.0), dict(lr=NAN), dict(lr=INF), dict(b1=1.0),
               dict(b1=-0.1), dict(b2=1.5), dict(b2=NAN), dict(b3=1.0), dict(b3=NAN), dict(b3=-0.5), dict(d0=0.0),
               dict(d0=-1e-6), dict(d0=NAN), dict(d0=INF), dict(d_coef=0.0), dict(d_coef=-1.0), dict(d_coef=NAN),
               dict(growth=0.5), dict(growth=NAN), dict(growth=-INF)):
        assert _finalize(L, **kw) == VP_ERR_ARG, kw
    assert _finalize(L, phase=0, scalars=None) == VP_ERR_ARG
    assert _finalize(L, phase=0, dstate=None) == VP_ERR_ARG
    assert _finalize(L, phase=0, d0=0.0) == VP_ERR_ARG
    assert _finalize(L, phase=0, b1=1.0) == VP_ERR_ARG


def test_empty_work_is_accepted_without_a_launch():
    L = N.lib()
    assert _adam(L, ranges=None, n=0) == 0
    assert _moments(L, ranges=None, n=0, partials=None) == 0
    assert _update(L, ranges=None, n=0) == 0
    assert _unpack(L, tensors=None, chunks=None, n=0, flat=None, flat_len=0) == 0


def test_struct_sizes_are_unchanged():
    """The Prodigy record is a plain double[2]: no new struct, vp_struct_sizes still writes exactly 15 entries."""
    L = N.lib()
    sizes = (N.i64 * 16)(*([-7] * 16))
    L.vp_struct_sizes(sizes)
    assert sizes[15] == -7 and all(s > 0 for s in sizes[:15])


def test_wrappers_check_their_tensors():
    """kernels.py refuses host tensors (every test tensor here is one), and with them wrong dtypes and short
    workspaces, before the library is called."""
    from videopainter_amd import kernels as K
    f32, i32s, blk = torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.float64)
    bf, rec = torch.zeros(8, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.float64)
    fin = dict(lr=1.0, betas=(0.9, 0.95), beta3=0.97, d0=1e-6, d_coef=1.0, growth_rate=INF, use_bias_correction=False)
    mom = dict(betas=(0.9, 0.95), beta3=0.97, weight_decay=0.0, d0=1e-6, safeguard_warmup=False, use_clip=False)
    with pytest.raises(ValueError):
        K.zero_shard_adam(None, 0, 0, f32, f32, f32, f32, bf, i32s, lr=1e-3, betas=(0.9, 0.95), eps=1e-8,
                          weight_decay=0.0, use_clip=False)
    with pytest.raises(ValueError):
        K.zero_shard_prodigy_moments(None, 0, 0, f32, f32, f32, f32, f32, f32, f32, i32s, blk, **mom)
    with pytest.raises(ValueError):
        K.zero_prodigy_record(f32, 1, i32s, rec)
    with pytest.raises(ValueError):
        K.zero_prodigy_finalize(2, rec, 1, i32s, blk, **fin)
    with pytest.raises(ValueError):
        K.zero_prodigy_finalize(0, None, 1, i32s, blk, **fin)  # host scalars
    with pytest.raises(ValueError):
        K.zero_prodigy_finalize(1, rec, 1, i32s, blk, **fin)
    with pytest.raises(ValueError):
        K.zero_shard_prodigy_update(None, 0, 0, f32, f32, f32, bf, i32s, blk, eps=1e-8, weight_decay=0.0)
    with pytest.raises(ValueError):
        K.zero_unpack_gated(None, None, 0, bf, i32s, blk)
    # the checks that come after the device check, on their own
    with pytest.raises(ValueError, match="fewer than"):
        K._chk_pairs(_FakeDevice(torch.zeros(3)), 2, "t")
    with pytest.raises(ValueError, match="fewer than"):
        K._chk_records(_FakeDevice(torch.zeros(3, dtype=torch.float64)), 2, "t")
    with pytest.raises(TypeError):
        K._chk_records(_FakeDevice(torch.zeros(4)), 2, "t")
    with pytest.raises(ValueError, match="differ in length"):
        K._chk_shards("t", (("a", _FakeDevice(torch.zeros(8))), ("b", _FakeDevice(torch.zeros(16)))))
    with pytest.raises(ValueError, match="differ in length"):
        K._chk_shards("t", (("a", _FakeDevice(torch.zeros(8))),), _FakeDevice(torch.zeros(16, dtype=torch.bfloat16)))


class _FakeDevice:
    """A host tensor that answers is_cuda with True: lets the size and dtype checks behind the device check run."""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _bf(*s):
    return torch.nn.Parameter(torch.zeros(*s, dtype=torch.bfloat16))


@pytest.mark.parametrize("name", ["ShardedFusedAdam", "ShardedFusedProdigy"])
def test_constructor_validation(name):
    import videopainter_amd as V
    from videopainter_amd.distributed import LocalComm
    S, comm = getattr(V, name), LocalComm(2)
    with pytest.raises(TypeError):
        S([torch.nn.Parameter(torch.zeros(4))], comm=comm, rank=0)  # fp32
    with pytest.raises(ValueError):
        S([torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.bfloat16).t())], comm=comm, rank=0)  # not contiguous
    with pytest.raises(ValueError):
        S([], comm=comm, rank=0)
    sp = _bf(4, 4)
    sp.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.ones(1, dtype=torch.bfloat16), (4, 4))
    with pytest.raises(ValueError):
        S([sp], comm=comm, rank=0)
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-1.0),
               dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            S([_bf(4)], comm=comm, rank=0, **kw)
    with pytest.raises(ValueError):
        S([_bf(4)], comm=comm, rank=0)  # valid dtype and layout, but not on a device: nothing is allocated for it
    with pytest.raises(ValueError, match="needs rank"):
        S([_bf(4)], comm=comm)  # comm= without rank=
    for rank in (2, -1):
        with pytest.raises(ValueError, match="outside world size"):
            S([_bf(4)], comm=comm, rank=rank)
    with pytest.raises(ValueError, match="not both"):
        S([_bf(4)], comm=comm, rank=0, process_group=object())
    with pytest.raises(ValueError):
        S([_bf(4)])  # neither a communicator nor an initialised process group


def test_prodigy_constructor_validation():
    from videopainter_amd import ShardedFusedProdigy
    from videopainter_amd.distributed import LocalComm
    comm = LocalComm(2)
    for kw in (dict(d0=0.0), dict(d0=-1e-6), dict(d0=NAN), dict(d0=INF), dict(d_coef=0.0), dict(d_coef=-1.0),
               dict(d_coef=NAN), dict(growth_rate=0.99), dict(growth_rate=NAN), dict(beta3=1.0), dict(beta3=-0.1)):
        with pytest.raises(ValueError, match="Invalid"):
            ShardedFusedProdigy([_bf(4)], comm=comm, rank=0, **kw)
    with pytest.raises(ValueError, match="same in every parameter group"):
        ShardedFusedProdigy([dict(params=[_bf(4)]), dict(params=[_bf(4)], lr=0.5)], comm=comm, rank=0)
    with pytest.raises(ValueError, match="same in every parameter group"):
        ShardedFusedProdigy([dict(params=[_bf(4)]), dict(params=[_bf(4)], beta3=0.5)], comm=comm, rank=0)


def test_public_names_are_exported_lazily():
    import videopainter_amd as V
    from videopainter_amd import optim, zero
    assert "ShardedFusedProdigy" not in vars(V) and "ShardedFusedAdam" not in vars(V)  # resolved on first use
    assert V.ShardedFusedProdigy is zero.ShardedFusedProdigy and V.ShardedFusedAdam is zero.ShardedFusedAdam
    assert issubclass(V.ShardedFusedAdam, V.ShardedFusedAdamW) and issubclass(V.ShardedFusedProdigy, optim._FlatAdamW)
    assert issubclass(V.ShardedFusedProdigy, torch.optim.Optimizer)
    assert not issubclass(V.ShardedFusedProdigy, V.ShardedFusedAdamW)
    for p in ("d", "d_max", "d_hat", "d_numerator", "d_denom", "dlr", "no_progress", "d_block", "master_shard",
              "exp_avg_shard", "exp_avg_sq_shard", "s_shard", "p0_shard"):
        assert isinstance(getattr(V.ShardedFusedProdigy, p), property), p
    for name in ("vp_zero_shard_adam", "vp_zero_shard_prodigy_moments", "vp_zero_prodigy_record",
                 "vp_zero_prodigy_finalize", "vp_zero_shard_prodigy_update", "vp_zero_unpack_gated_bf16"):
        assert name in N.EXPORTS
