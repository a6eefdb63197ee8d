"""The launches of a resample block's training forward with the closed-form backward switched off and on (CPU, the
recorders of tests/launch_recorder.py): off, exactly what it issues today; on, the inference plan's launches with the
attention's `lse` requested — and the refusals of the opt-in, which need no device."""
import json
import os

import pytest
import torch

from tests.launch_recorder import recording

GOLD = os.path.join(os.path.dirname(__file__), "golden", "block_launches.json")
B, T, D, H = 2, 8, 128, 2
GRID = (2, 12, 12)
NV = GRID[0] * GRID[1] * GRID[2]
N = T + NV


def _block():
    from tests.golden.cases import TINY_CFG, tiny_weights
    from videopainter_amd import CogVideoXTransformer3DModel
    tr = CogVideoXTransformer3DModel(**dict(TINY_CFG, num_layers=1, id_pool_resample_learnable=True))
    tsd, _ = tiny_weights()
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()
                                  if not k.startswith("transformer_blocks.") or k.startswith("transformer_blocks.0.")})
    tr.requires_grad_(False)
    return tr, tr.transformer_blocks[0]


def _inputs():
    """x, temb and the rope of tests/test_block_launches_cpu.py (no grid: the k2_full plan), the same token mask, and
    a separable table that carries its grid (the closed-form plan)."""
    from oracle.cogvideox_oracle import prepare_rotary_positional_embeddings
    from videopainter_amd.attention_processor import _rope_dev
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    x = torch.randn(B, N, D, generator=g).to(bf)
    temb = torch.randn(B, 32, generator=g).to(bf)
    plain = _rope_dev((torch.randn(NV, 64, generator=g), torch.randn(NV, 64, generator=g)), x.device)
    g = torch.Generator().manual_seed(6)
    rmask = torch.zeros(B, N, dtype=torch.uint8)
    rmask[:, T:] = (torch.rand(B, NV, generator=g) < 0.5).to(torch.uint8)
    cos, sin = prepare_rotary_positional_embeddings(GRID[1] * 16, GRID[2] * 16, GRID[0], 64)
    grid = _rope_dev((cos.float(), sin.float()), x.device, GRID)
    return x, temb, plain, grid, rmask


def _record(fn, monkeypatch):
    from videopainter_amd import attention_processor as AP
    from videopainter_amd import kernels as K
    AP._MASK_PLANS.clear()  # (every record builds the mask plan, as a forward's first block does)
    with recording() as log:
        # (host-side size predicate of the backward kernel: it asks the library, which the recorders stand in for)
        monkeypatch.setattr(K, "null_key_mass_bwd_supported", lambda grid: True)
        fn()
    return json.loads(json.dumps(log))


def test_switch_off_records_todays_training_forward(monkeypatch):
    from videopainter_amd import autograd as AG
    x, temb, plain, grid, rmask = _inputs()
    tr, blk = _block()
    assert not getattr(blk.attn1, "closed_form_resample_backward", False)  # the default
    with open(GOLD) as f:
        golden = json.load(f)
    for enable in (None, False):
        if enable is not None:
            tr.enable_closed_form_resample_backward(enable)
        with torch.enable_grad():
            got = _record(lambda: AG.block_apply(blk, x.clone().requires_grad_(), T, temb, plain,
                                                 resample_mask=rmask), monkeypatch)
        assert got == golden["e_resample_k2_full"]
    # with the grid: the inference plan's launches, no statistics kept
    with torch.no_grad():
        infer = _record(lambda: blk.forward_joint(x, T, temb, grid, resample_mask=rmask), monkeypatch)
    with torch.enable_grad():
        got = _record(lambda: AG.block_apply(blk, x.clone().requires_grad_(), T, temb, grid, resample_mask=rmask),
                      monkeypatch)
    assert got == infer
    assert [l["args"]["lse"] for l in got if l["entry"] == "attention"] == [None]


def test_switch_on_records_the_inference_plan_with_lse(monkeypatch):
    from videopainter_amd import autograd as AG
    x, temb, plain, grid, rmask = _inputs()
    tr, blk = _block()
    with torch.no_grad():
        infer = _record(lambda: blk.forward_joint(x, T, temb, grid, resample_mask=rmask), monkeypatch)
    assert "null_key_mass" in [l["entry"] for l in infer]
    tr.enable_closed_form_resample_backward()
    assert blk.attn1.closed_form_resample_backward
    with torch.enable_grad():
        got = _record(lambda: AG.block_apply(blk, x.clone().requires_grad_(), T, temb, grid, resample_mask=rmask),
                      monkeypatch)
    assert [l["entry"] for l in got] == [l["entry"] for l in infer]
    lse = {"shape": [B, H, N], "stride": [H * N, N, 1], "dtype": "float32"}
    for g_, w in zip(got, infer):
        if g_["entry"] == "attention":
            assert w["args"]["lse"] is None and g_["args"]["lse"] == lse
            assert g_["args"]["k2_len"] is not None and g_["args"]["l_extra"] is not None
            g_ = {"entry": g_["entry"], "args": dict(g_["args"], lse=None)}
        assert g_ == w, g_["entry"]
    # inference with the switch on is the same trace: the switch acts on a training forward only
    with torch.no_grad():
        assert _record(lambda: blk.forward_joint(x, T, temb, grid, resample_mask=rmask), monkeypatch) == infer


def test_opt_in_does_not_fall_back(monkeypatch):
    from videopainter_amd import autograd as AG
    x, temb, plain, grid, rmask = _inputs()
    tr, blk = _block()
    tr.enable_closed_form_resample_backward()
    xg = x.clone().requires_grad_()
    with recording():
        monkeypatch.setattr("videopainter_amd.kernels.null_key_mass_bwd_supported", lambda grid: True)
        with pytest.raises(ValueError, match="grid"):
            AG.block_apply(blk, xg, T, temb, plain, resample_mask=rmask)
        from videopainter_amd import attention_processor as AP
        for sw in ("VP_RESAMPLE_NULLMASS", "VP_RESAMPLE_PARTITION"):
            prev = AP.set_switch(sw, "0")
            try:
                with pytest.raises(ValueError, match="closed-form"):
                    AG.block_apply(blk, xg, T, temb, grid, resample_mask=rmask)
            finally:
                AP.set_switch(sw, prev)
        blk.attn1.norm_k.bias.requires_grad_(True)
        with pytest.raises(NotImplementedError, match="norm_k"):
            AG.block_apply(blk, xg, T, temb, grid, resample_mask=rmask)
