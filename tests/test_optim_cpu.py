"""Training tail (videopainter_amd/optim.py, csrc/optim.hip) — the parts that need no GPU: the chunk-table builder,
host-side argument validation of the C entry points, and the optimizer's constructor validation."""
import ctypes as C

import numpy as np
import pytest
import torch

from videopainter_amd import _native as N
from videopainter_amd.optim import CHUNK, FusedAdamW, build_chunk_table, build_tensor_table

VP_ERR_ARG = 1000


def _coverage(sizes, chunk):
    tab = build_chunk_table(sizes, chunk)
    assert tab.dtype == np.int32 and tab.shape[1] == 2
    seen = [np.zeros(n, dtype=np.int64) for n in sizes]
    for t, c in tab:
        lo, hi = int(c) * chunk, min(sizes[t], (int(c) + 1) * chunk)
        assert 0 <= lo < hi <= sizes[t], "an empty chunk, or one that leaves its tensor"
        seen[t][lo:hi] += 1
    for n, s in zip(sizes, seen):
        assert (s == 1).all()  # every element exactly once (vacuous for an empty tensor)
    return tab


def test_chunk_table_covers_every_element_once():
    sizes = [1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 0]
    tab = _coverage(sizes, CHUNK)
    per_tensor = np.bincount(tab[:, 0], minlength=len(sizes)).tolist()
    assert per_tensor == [1, 1, 1, 1, 1, 1, 2, 4, 0]  # the zero-size tensor has no chunk
    assert (np.diff(tab[:, 0]) >= 0).all()  # list order: a parameter group's chunks are one contiguous range
    assert build_chunk_table([]).shape == (0, 2)
    assert build_chunk_table([0, 0]).shape == (0, 2)
    _coverage([5, 0, 17, 4], 4)  # a small chunk size: boundaries at multiples and non-multiples


def test_tables_match_the_c_structs():
    assert CHUNK == N.MT_CHUNK
    tt = build_tensor_table([16, 32], [48, 64], [0, 8], [3, 5])
    assert tt.dtype == np.int64 and tt.shape == (2, 4) and tt.flags["C_CONTIGUOUS"]
    assert tt.itemsize * tt.shape[1] == C.sizeof(N.MtTensor)
    e = N.MtTensor.from_buffer_copy(tt[1].tobytes())
    assert (e.grad, e.param, e.state_off, e.numel) == (32, 64, 8, 5)
    ct = build_chunk_table([CHUNK + 1])
    assert ct.itemsize * ct.shape[1] == C.sizeof(N.MtChunk)
    c = N.MtChunk.from_buffer_copy(ct[1].tobytes())
    assert (c.tensor, c.chunk) == (0, 1)
    L = N.lib()  # (checks the three struct sizes against the library's)
    import re
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vp_hip.h")).read()
    assert int(re.search(r"#define VP_MT_CHUNK (\d+)", hdr).group(1)) == CHUNK
    assert L.vp_abi_version() >= 21


def test_pack_tables_places_every_table_on_a_16_byte_boundary():
    from videopainter_amd.optim import pack_tables
    from videopainter_amd.zero import RANGE_DTYPE
    numels = [3, CHUNK + 1, 5]  # 3 tensor rows of 32 bytes, 4 chunk rows of 8 bytes, 3 range rows of 16 bytes
    tt = build_tensor_table([16, 32, 48], [64, 80, 96], [0, 8, CHUNK + 16], numels)
    ct = build_chunk_table(numels)
    rt = np.zeros(3, dtype=RANGE_DTYPE)
    rt["start"], rt["n"] = [0, 8, 24], [3, 9, 5]
    odd = np.arange(5, dtype=np.uint8)  # a table whose size is no multiple of 16
    tables = [tt, odd, ct, rt]
    image, offs = pack_tables(tables)
    assert image.dtype == np.uint8 and image.ndim == 1 and len(offs) == len(tables)
    assert all(o % 16 == 0 for o in offs)
    for a, o in zip(tables, offs):
        assert image[o:o + a.nbytes].tobytes() == a.tobytes()  # byte for byte, no overlap with the next table
    assert offs == sorted(offs) and all(o + a.nbytes <= n for a, o, n in zip(tables, offs, offs[1:] + [image.size]))
    _, two = pack_tables([tt, ct])
    assert two == [0, len(numels) * 32]  # the single-GPU layout: the chunk table right behind the tensor rows
    image, offs = pack_tables([])
    assert image.size == 0 and offs == []
    image, offs = pack_tables([build_tensor_table([], [], [], []), build_chunk_table([]), np.zeros(0, RANGE_DTYPE)])
    assert image.size == 0 and offs == [0, 0, 0]


def test_entry_points_reject_bad_arguments_without_a_gpu():
    L = N.lib()
    p = 4096  # a non-null "pointer": every call below must return before any launch
    assert L.vp_mt_grad_sqnorm_bf16(None, None, 1, None, None, None) == VP_ERR_ARG
    assert L.vp_mt_grad_sqnorm_bf16(p, p, -1, p, p, None) == VP_ERR_ARG
    assert L.vp_mt_grad_sqnorm_bf16(p, p, 3, None, p, None) == VP_ERR_ARG
    assert L.vp_optim_finalize(p, p, 1, 1.0, 0.9, 0.95, 0, 1, None, None) == VP_ERR_ARG
    assert L.vp_optim_finalize(None, p, 1, 1.0, 0.9, 0.95, 0, 1, p, None) == VP_ERR_ARG
    assert L.vp_optim_finalize(p, p, -1, 1.0, 0.9, 0.95, 0, 1, p, None) == VP_ERR_ARG
    assert L.vp_optim_finalize(p, p, 1, float("nan"), 0.9, 0.95, 0, 1, p, None) == VP_ERR_ARG
    assert L.vp_optim_finalize(p, p, 1, 1.0, 1.0, 0.95, 0, 1, p, None) == VP_ERR_ARG  # beta1 = 1
    assert L.vp_mt_scale_bf16(None, None, 1, p, None) == VP_ERR_ARG
    assert L.vp_mt_scale_bf16(p, p, 1, None, None) == VP_ERR_ARG
    assert L.vp_mt_scale_bf16(p, p, -2, p, None) == VP_ERR_ARG
    adam = lambda *a, lr=1e-5, b1=0.9, b2=0.95, eps=1e-8, wd=1e-4: L.vp_mt_adamw_bf16(  # noqa: E731
        *a, lr, b1, b2, eps, wd, 1, 0, None)
    assert adam(None, None, 0, 1, p, p, p, p) == VP_ERR_ARG
    assert adam(p, p, 0, 1, None, p, p, p) == VP_ERR_ARG
    assert adam(p, p, 0, 1, p, p, p, None) == VP_ERR_ARG
    assert adam(p, p, -1, 1, p, p, p, p) == VP_ERR_ARG
    assert adam(p, p, 0, -1, p, p, p, p) == VP_ERR_ARG
    assert adam(p, p, 0, 1, p, p, p, p, lr=-1.0) == VP_ERR_ARG
    assert adam(p, p, 0, 1, p, p, p, p, b2=1.5) == VP_ERR_ARG
    assert adam(p, p, 0, 1, p, p, p, p, eps=float("nan")) == VP_ERR_ARG
    assert L.vp_scale_dev_bf16(None, p, 8, p, None) == VP_ERR_ARG
    assert L.vp_scale_dev_bf16(p, p, 8, None, None) == VP_ERR_ARG
    assert L.vp_scale_dev_bf16(p, p, 0, p, None) == VP_ERR_ARG
    assert L.vp_v_loss_partials(0, 1, 1, 1) == -1
    assert L.vp_v_loss_partials(1, 2, 3, 35) == 1
    assert L.vp_v_loss_partials(2, 1, 1, CHUNK + 1) == 4
    assert L.vp_v_loss_partials(1, 4096, 4096, 4096) == -1  # a sample of 2^36 elements
    loss = lambda out=p, mask=None, ts=p, ac=p, na=1000, B=1, lam=1.0, part=p: L.vp_v_loss_bf16(  # noqa: E731
        out, p, p, mask, 0, ts, ac, na, B, 2, 3, 35, lam, part, p, p, None)
    assert loss(out=None) == VP_ERR_ARG
    assert loss(ts=None) == VP_ERR_ARG
    assert loss(ac=None) == VP_ERR_ARG
    assert loss(na=0) == VP_ERR_ARG  # timestep table length <= 0
    assert loss(na=-5) == VP_ERR_ARG
    assert loss(B=0) == VP_ERR_ARG
    assert loss(B=-1) == VP_ERR_ARG
    assert loss(part=None) == VP_ERR_ARG
    assert loss(lam=float("nan")) == VP_ERR_ARG


def test_empty_lists_are_accepted_without_a_launch():
    L = N.lib()
    assert L.vp_mt_grad_sqnorm_bf16(None, None, 0, None, None, None) == 0
    assert L.vp_mt_scale_bf16(None, None, 0, 4096, None) == 0
    assert L.vp_mt_adamw_bf16(None, None, 0, 0, 4096, 4096, 4096, 4096, 1e-5, 0.9, 0.95, 1e-8, 1e-4, 1, 0, None) == 0


def test_fused_adamw_constructor_validation():
    bf = lambda *s: torch.nn.Parameter(torch.zeros(*s, dtype=torch.bfloat16))  # noqa: E731
    with pytest.raises(TypeError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4))])  # fp32
    with pytest.raises(TypeError):
        FusedAdamW([bf(4), torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.bfloat16).t())])  # not contiguous
    with pytest.raises(ValueError):
        FusedAdamW([])  # empty
    frozen = bf(4)
    frozen.requires_grad_(False)
    with pytest.raises(ValueError):
        FusedAdamW([frozen])  # empty after dropping what needs no gradient
    sp = bf(4, 4)
    sp.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.ones(1, dtype=torch.bfloat16), (4, 4))
    with pytest.raises(ValueError):
        FusedAdamW([sp])
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-1.0),
               dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            FusedAdamW([bf(4)], **kw)
    with pytest.raises(ValueError):
        FusedAdamW([bf(4)])  # valid dtype and layout, but not on a device: nothing is allocated for it


def test_public_names_are_exported():
    import videopainter_amd as V
    from videopainter_amd import optim, training
    assert V.FusedAdamW is optim.FusedAdamW and V.clip_grad_norm_ is optim.clip_grad_norm_
    assert V.get_gradient_norm is optim.get_gradient_norm and V.inpainting_v_loss is training.inpainting_v_loss
