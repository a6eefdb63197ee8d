"""The launch sequences of one CogVideoXBlock on the CPU: inference (`forward_joint` in its bf16 forms), the training
forward (`autograd.block_apply` in its three keep modes) and the backward's recompute front issue the kernel
launches recorded from the commit BEFORE the block forward was written once as stages
(tests/golden/block_launches.json) — entry, every scalar argument, and shape / strides / dtype of every tensor
argument (so "AdaLN wrote into the augmented operand" and "aux present" are part of the trace).

The `videopainter_amd.kernels` entry points the block calls are replaced, inside the launch-trace tests only, by the
recorders of tests/launch_recorder.py; the product path has no such substitute.

To record the fixture (against a checkout of the commit the traces are to be compared with, from its root):
    python -c "from tests.test_block_launches_cpu import write_fixture; write_fixture('block_launches.json')"
"""
import json
import os

import pytest
import torch

from tests.launch_recorder import _RETURNS, _describe, _empty, recording  # noqa: F401 (other tests take them here)

GOLD = os.path.join(os.path.dirname(__file__), "golden", "block_launches.json")
B, T, NV, D, H = 2, 8, 288, 128, 2
N = T + NV
MODES = {"all": (True, True), "attention": (False, True), "recompute": (False, False)}  # (SAVE_ACTIVATIONS, _ATTENTION)


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------

def _block(resample=False, lora=False, trainable=False):
    from tests.golden.cases import TINY_CFG, tiny_weights
    from videopainter_amd import CogVideoXTransformer3DModel
    tr = CogVideoXTransformer3DModel(**dict(TINY_CFG, num_layers=1, id_pool_resample_learnable=resample))
    tsd, _ = tiny_weights()
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()
                                  if not k.startswith("transformer_blocks.") or k.startswith("transformer_blocks.0.")})
    tr.requires_grad_(False)
    if lora:
        tr.add_adapter({"r": 8, "lora_alpha": 8, "target_modules": ["to_q", "to_k", "to_v", "to_out.0"]})
    blk = tr.transformer_blocks[0]
    if trainable:
        blk.requires_grad_(True)
    return blk


def _inputs():
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    x = torch.randn(B, N, D, generator=g).to(bf)
    temb = torch.randn(B, 32, generator=g).to(bf)
    # the tables as a model's forward hands them to its blocks, without a video grid (the resample processor then
    # keeps its null keys as row-sum-only keys, k2_full)
    from videopainter_amd.attention_processor import _rope_dev
    rope = _rope_dev((torch.randn(NV, 64, generator=g), torch.randn(NV, 64, generator=g)), x.device)
    return x, temb, rope


def _recompute_front(AG, block, x, temb, rope, resample_mask, attn_saved, with_h):
    """The backward's recompute of the block's front (the one-line adapter between commits)."""
    return AG._block_front(block, x, T, temb, rope, resample_mask, attn_saved, with_h=with_h)


def record_all() -> dict:
    """{case: [launch, ...]} of every case, from the code importable as `videopainter_amd`."""
    from videopainter_amd import autograd as AG
    x, temb, rope = _inputs()
    g = torch.Generator().manual_seed(6)
    bf = torch.bfloat16
    mask = (torch.rand(B, NV, generator=g) < 0.5).to(torch.uint8)
    rmask = torch.zeros(B, N, dtype=torch.uint8)
    rmask[:, T:] = mask
    out = {}

    def run(name, fn):
        with recording() as log:
            fn()
        out[name] = log

    plain = _block()
    with torch.no_grad():
        run("a_plain", lambda: plain.forward_joint(x, T, temb, rope))
        mod1, mod2 = torch.randn(B, 6 * D, generator=g).to(bf), torch.randn(B, 6 * D, generator=g).to(bf)
        inject = torch.randn(B, NV, D, generator=g).to(bf)
        run("b_mods_inject", lambda: plain.forward_joint(x, T, temb, rope, inject=inject, inject_mask=mask,
                                                         mod1=mod1, mod2=mod2))
        run("c_cfg_shared", lambda: plain.forward_joint(x, T, temb, rope, cfg_shared_video=True))
        prev = torch.randn(B, N, D, generator=g).to(bf)
        run("d_prev_clip", lambda: plain.forward_joint(x, T, temb, rope, prev_joint=prev, prev_clip_weight=0.3))
        run("e_resample_k2_full", lambda: _block(resample=True).forward_joint(x, T, temb, rope, resample_mask=rmask))
        run("f_lora", lambda: _block(lora=True).forward_joint(x, T, temb, rope))
        run("g_attend_hook", lambda: plain.forward_joint(x, T, temb, rope,
                                                         attend=lambda attn, xn, *rest: torch.empty_like(xn)))

    room = AG._room_for
    saved = AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION
    AG._room_for = lambda *a, **k: True
    try:
        for kind in ("frozen", "trainable"):
            blk = _block(trainable=kind == "trainable")
            for mode, (AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION) in MODES.items():
                with torch.enable_grad():
                    run(f"h_{kind}_{mode}", lambda: AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope))
    finally:
        AG._room_for = room
        AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION = saved

    with torch.no_grad():
        attn_saved = (torch.empty(B, N, D, dtype=bf), torch.empty(B, H, N, dtype=torch.float32))
        for sv, saved_name in ((None, "attn_recomputed"), (attn_saved, "attn_saved")):
            for with_h in (False, True):
                run(f"i_front_{saved_name}_{'h' if with_h else 'z'}",
                    lambda: _recompute_front(AG, plain, x, temb, rope, None, sv, with_h))
        # (the resample recompute front too: its explicit 2N-key construction is autograd's own)
        run("i_front_resample", lambda: _recompute_front(AG, _block(resample=True), x, temb, rope, rmask, None,
                                                         True))
    return out


def write_fixture(path: str = GOLD) -> None:
    with open(path, "w") as f:
        json.dump(record_all(), f, indent=0, sort_keys=True)
        f.write("\n")


# ------------------------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def traces():
    return record_all()


@pytest.fixture(scope="module")
def golden():
    with open(GOLD) as f:
        return json.load(f)


def test_same_cases_as_the_fixture(traces, golden):
    assert sorted(traces) == sorted(golden)
    assert len(golden["a_plain"]) == 9 and len(golden["h_frozen_all"]) == 9


@pytest.mark.parametrize("case", [
    "a_plain", "b_mods_inject", "c_cfg_shared", "d_prev_clip", "e_resample_k2_full", "f_lora", "g_attend_hook",
    "h_frozen_all", "h_frozen_attention", "h_frozen_recompute", "h_trainable_all", "h_trainable_attention",
    "h_trainable_recompute", "i_front_attn_recomputed_z", "i_front_attn_recomputed_h", "i_front_attn_saved_z",
    "i_front_attn_saved_h", "i_front_resample"])
def test_trace_equals_the_recorded_one(traces, golden, case):
    got = json.loads(json.dumps(traces[case]))  # (tuples -> lists, as the fixture went through JSON)
    want = golden[case]
    assert [l["entry"] for l in got] == [l["entry"] for l in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: launch {i} ({g['entry']}) differs"


def _core(trace):
    """A trace without what the design lets the paths differ in: the outputs a keep level adds (the GEMMs' `aux`, the
    attention's `lse`) and where the norm2 modulation launch sits (the modulation launches leave; their number is
    returned)."""
    core = [{"entry": l["entry"], "args": {k: v for k, v in l["args"].items() if k not in ("aux", "lse")}}
            for l in trace if l["entry"] != "linear_small"]
    return core, sum(l["entry"] == "linear_small" for l in trace)


def test_inference_training_forward_and_recompute_agree(traces):
    """(a), (h) and (i) issue the same launches except for the aux arguments, the position of the norm2
    linear_small, and the launches a mode skips."""
    a, n_mod = _core(traces["a_plain"])
    assert n_mod == 2 and [l["entry"] for l in a] == ["adaln_modulate", "gemm", "attention", "gemm", "adaln_modulate",
                                                      "gemm", "gemm"]
    for kind in ("frozen", "trainable"):
        for mode in MODES:
            assert _core(traces[f"h_{kind}_{mode}"]) == (a, 2), (kind, mode)
        # the aux outputs are requested by the keep-all forward alone
        for mode, want in (("all", True), ("attention", False), ("recompute", False)):
            aux = [l["args"]["aux"] is not None for l in traces[f"h_{kind}_{mode}"] if l["entry"] == "gemm"]
            assert aux == [want, False, want, False], (kind, mode)
            lse = [l["args"]["lse"] is not None for l in traces[f"h_{kind}_{mode}"] if l["entry"] == "attention"]
            assert lse == [mode != "recompute"], (kind, mode)
    assert all(l["args"].get("aux") is None and l["args"].get("lse") is None for l in traces["a_plain"])
    no_attention = [l for l in a if l["entry"] != "attention"]
    for name, want in (("attn_recomputed", a), ("attn_saved", no_attention)):
        # with h: the front is the forward up to FF1 (the GELU epilogue, z as its aux output)
        assert _core(traces[f"i_front_{name}_h"]) == (want[:-1], 2), name
        # without: FF1 stores the pre-activation alone — the one launch that differs, in its epilogue only
        z, n_mod = _core(traces[f"i_front_{name}_z"])
        assert n_mod == 2 and z[:-1] == want[:-2], name
        ff1_z, ff1_h = z[-1]["args"], want[-2]["args"]
        assert {k: v for k, v in ff1_z.items() if k != "epilogue"} == {k: v for k, v in ff1_h.items()
                                                                       if k != "epilogue"}
        assert ff1_z["epilogue"] != ff1_h["epilogue"]
