"""The launch sequence of one frozen CogVideoXBlock on the MX-FP8 GEMMs through a training step, on the CPU: the
rehearsal of the host logic of the fp8 training path (transformer.py's stages, autograd.py's MX arms) on a machine
without a GPU.

The recorder of tests/launch_recorder.py, extended INSIDE THIS TEST ONLY with recorders for the MX entries (and a
device-free stand-in for kernels.MXTensor).  Pinned: the training forward of an fp8 block is the inference fp8
forward's launch sequence — identical without a keep level, with the attention's lse output at "attention", and at
"all" also FF1's aux output and the two q / k norm launches' destination (beside the handed-over qkv instead of over
it, where the attention then reads them); and the backward's sequence for each `autograd.FP8_DGRAD` setting.
"""
import contextlib
import inspect
import json

import pytest
import torch

from tests.launch_recorder import _describe, recording
from tests.test_block_launches_cpu import MODES

B, T, NV, D, H, F4 = 2, 8, 288, 256, 4, 1024
N = T + NV
M = B * N
ALL = ("ff2", "ff1", "out", "qkv")


class _MX:  # kernels.MXTensor without a device or the library
    def __init__(self, rows, K, device=None, q=None, scales=None, zero=True):
        self.rows, self.K = rows, K
        self.q = torch.empty((rows + 255) // 256 * 256, K, dtype=torch.uint8)
        self.scales = torch.empty((rows + 255) // 256 * (K // 128) * 1024, dtype=torch.uint8)


def _describe_x(v):
    if isinstance(v, _MX):
        return {"mx": [v.rows, v.K]}
    if isinstance(v, (list, tuple)) and any(isinstance(e, _MX) for e in v):
        return [_describe_x(e) for e in v]
    return _describe(v)


def _rows(t):
    return t.numel() // t.shape[-1]


_RETURNS_X = {
    "mx_quantize": lambda a: a["out"] if a["out"] is not None else _MX(_rows(a["x"]), a["x"].shape[-1]),
    "adaln_modulate_mx": lambda a: a["out"] if a["out"] is not None else _MX(_rows(a["x"]), a["x"].shape[-1]),
    "rowscale_mx": lambda a: a["out"] if a["out"] is not None else _MX(_rows(a["x"]), a["x"].shape[-1]),
    "gemm_mx": lambda a: a["out"],
    "gelu_bwd": lambda a: a["out"] if a["out"] is not None else torch.empty_like(a["z"]),
}


@contextlib.contextmanager
def recording_mx():
    from videopainter_amd import kernels as K
    saved = {}
    with recording() as log:
        def recorder(name, real):
            sig = inspect.signature(real)

            def rec(*args, **kw):
                ba = sig.bind(*args, **kw)
                ba.apply_defaults()
                log.append({"entry": name, "args": {k: _describe_x(v) for k, v in ba.arguments.items()}})
                return _RETURNS_X[name](ba.arguments)
            return rec
        try:
            for n in _RETURNS_X:
                saved[n] = getattr(K, n)
                setattr(K, n, recorder(n, saved[n]))
            saved["MXTensor"] = K.MXTensor
            K.MXTensor = _MX
            yield log
        finally:
            for n, f in saved.items():
                setattr(K, n, f)


def _block(ffn=True, qkv=True, out=True):
    """A frozen D = 256 block; the enable_fp8_* calls run under the recorder (they quantise the weights)."""
    from videopainter_amd.transformer import CogVideoXBlock
    torch.manual_seed(3)
    blk = CogVideoXBlock(dim=D, num_attention_heads=H, attention_head_dim=64, time_embed_dim=32, attention_bias=True)
    blk.requires_grad_(False)
    with recording_mx() as log:
        if ffn:
            blk.enable_fp8_ffn()
        if qkv:
            blk.enable_fp8_qkv()
        if out:
            blk.enable_fp8_out()
    # the forward weights only: the transposed dgrad weights are built at the first backward, so inference pays nothing
    assert [l["entry"] for l in log] == ["mx_quantize"] * (2 * ffn + 3 * qkv + out)
    return blk


def _inputs():
    from videopainter_amd.attention_processor import _rope_dev
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, N, D, generator=g).to(torch.bfloat16)
    temb = torch.randn(B, 32, generator=g).to(torch.bfloat16)
    rope = _rope_dev((torch.randn(NV, 64, generator=g), torch.randn(NV, 64, generator=g)), x.device)
    inject = torch.randn(B, NV, D, generator=g).to(torch.bfloat16)
    mask = (torch.rand(B, NV, generator=g) < 0.5).to(torch.uint8)
    return x, temb, rope, inject, mask


def _plain(log):
    """The trace through JSON, without the two modulation linears (a keep-all forward and the backward's recompute
    compute both up front, inference each before its norm: tests/test_block_launches_cpu.py pins that order)."""
    return [l for l in json.loads(json.dumps(log)) if l["entry"] != "linear_small"]


def _names(log):
    return [l["entry"] for l in log]


def _step(blk, mode, dgrad=ALL, twice=True):
    """(forward trace, backward trace) of block_apply + backward at a keep mode; twice: of the second step on the
    block (the transposed-weight caches filled by the first)."""
    from videopainter_amd import autograd as AG
    x, temb, rope, inject, mask = _inputs()
    saved = AG._room_for, AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION, AG.FP8_DGRAD
    AG._room_for = lambda *a, **k: True
    AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION = MODES[mode]
    AG.FP8_DGRAD = set(dgrad)
    try:
        for _ in range(2 if twice else 1):
            with recording_mx() as log, torch.enable_grad():
                y = AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope, inject.clone().requires_grad_(), mask)
                n_fwd = len(log)
                y.backward(torch.ones_like(y))
    finally:
        AG._room_for, AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION, AG.FP8_DGRAD = saved
    return _plain(log[:n_fwd]), _plain(log[n_fwd:])


def _inference(blk):
    x, temb, rope, inject, mask = _inputs()
    with torch.no_grad(), recording_mx() as log:
        blk.forward_joint(x, T, temb, rope, inject=inject, inject_mask=mask)
    return _plain(log)


INFERENCE = ["adaln_modulate_mx", "gemm_mx",                      # norm1 -> MX, QKV (pre-norm q | k | v in bf16)
             "head_norm_rope", "head_norm_rope", "attention",     # the q / k norms as launches of their own, bf16 flash
             "mx_quantize", "gemm_mx",                            # o -> MX, to_out + gated residual 1
             "adaln_modulate_mx", "gemm_mx", "gemm_mx"]           # norm2 -> MX, FF1 (GELU -> MX), FF2 + gate + inject


def test_inference_trace_is_the_fp8_forward():
    from videopainter_amd import _native as NAT
    log = _inference(_block())
    assert _names(log) == INFERENCE
    epi = [l["args"]["epilogue"] for l in log if l["entry"] == "gemm_mx"]
    assert epi == [NAT.EPI_BIAS, NAT.EPI_GATED, NAT.EPI_BIAS_GELU_MXFP8, NAT.EPI_GATED]
    assert all(l["args"]["aux"] is None and l["args"]["z"] is None for l in log if l["entry"] == "gemm_mx")


@pytest.mark.parametrize("mode", MODES)
def test_training_forward_is_the_inference_forward_plus_aux(mode):
    blk = _block()
    want = _inference(blk)
    got, _ = _step(blk, mode)
    assert _names(got) == INFERENCE
    diffs = [(i, k) for i, (g, w) in enumerate(zip(got, want)) for k in w["args"] if g["args"][k] != w["args"][k]]
    if mode == "recompute":
        assert diffs == []
        return
    if mode == "attention":  # the softmax statistics beside the attention output, as in bf16 training
        assert diffs == [(4, "lse")]
        return
    # keep-all: z as FF1's aux output; the normed q / k beside the pre-norm projection (the LayerNorm backward's input)
    # and the attention reading them there
    assert diffs == [(2, "x_out"), (3, "x_out"), (4, "q"), (4, "k"), (4, "lse"), (8, "aux")]
    assert got[4]["args"]["q"] == got[2]["args"]["x_out"] and got[4]["args"]["k"] == got[3]["args"]["x_out"]
    assert got[8]["args"]["aux"] == {"shape": [M, F4], "stride": [F4, 1], "dtype": "bfloat16"}
    for i in (2, 3):
        assert got[i]["args"]["x_in"] == want[i]["args"]["x_in"]  # (the columns of the [B, N, 3D] projection)
        assert want[i]["args"]["x_out"] == want[i]["args"]["x_in"]  # inference: in place
        assert got[i]["args"]["x_out"] == {"shape": [B, N, D], "stride": [N * 2 * D, 2 * D, 1], "dtype": "bfloat16"}


# the backward after a keep-all forward (nothing recomputed), per FP8_DGRAD setting
ATTN = ["attention_bwd", "head_norm_rope_bwd", "head_norm_rope_bwd"]
BACKWARD = {
    ALL: ["mask_scale_rows", "rowscale_mx", "gemm_mx", "gemm_mx", "adaln_bwd", "rowscale_mx", "gemm_mx", *ATTN,
          "mx_quantize", "gemm_mx", "adaln_bwd"],
    (): ["mask_scale_rows", "rowscale", "gemm", "gemm", "adaln_bwd", "rowscale", "gemm", *ATTN, "gemm", "adaln_bwd"],
    ("ff1", "out", "qkv"): ["mask_scale_rows", "rowscale", "gemm", "mx_quantize", "gemm_mx", "adaln_bwd",
                            "rowscale_mx", "gemm_mx", *ATTN, "mx_quantize", "gemm_mx", "adaln_bwd"],
    ("ff2", "out", "qkv"): ["mask_scale_rows", "rowscale_mx", "gemm_mx", "gelu_bwd", "gemm", "adaln_bwd",
                            "rowscale_mx", "gemm_mx", *ATTN, "mx_quantize", "gemm_mx", "adaln_bwd"],
    ("ff2", "ff1", "qkv"): ["mask_scale_rows", "rowscale_mx", "gemm_mx", "gemm_mx", "adaln_bwd", "rowscale", "gemm",
                            *ATTN, "mx_quantize", "gemm_mx", "adaln_bwd"],
    ("ff2", "ff1", "out"): ["mask_scale_rows", "rowscale_mx", "gemm_mx", "gemm_mx", "adaln_bwd", "rowscale_mx",
                            "gemm_mx", *ATTN, "gemm", "adaln_bwd"],
}


@pytest.mark.parametrize("dgrad", BACKWARD, ids=lambda d: "+".join(d) or "none")
def test_backward_sequence_per_dgrad_setting(dgrad):
    from videopainter_amd import _native as NAT
    _, bwd = _step(_block(), "all", dgrad)
    assert _names(bwd) == BACKWARD[dgrad]
    mx = [l["args"] for l in bwd if l["entry"] == "gemm_mx"]
    assert all(a["biases"] == [None] for a in mx)
    if "ff2" in dgrad:
        # FF2 dgrad: dY quantised after the gate-2 row-scale; with the FF1 dgrad in fp8 too, dz stays in MX
        rs = next(l["args"] for l in bwd if l["entry"] == "rowscale_mx")
        assert (rs["chunk_v"], rs["chunk_t"], rs["tokens_per_batch"], rs["text_len"]) == (2, 5, N, T)
        assert mx[0]["a"] == {"mx": [M, D]} and mx[0]["weights"] == [{"mx": [F4, D]}]
        if "ff1" in dgrad:
            assert mx[0]["epilogue"] == NAT.EPI_GELU_BWD_MXFP8 and mx[0]["out"] == {"mx": [M, F4]}
            assert mx[0]["z"] == {"shape": [M, F4], "stride": [F4, 1], "dtype": "bfloat16"}
            assert mx[1]["a"] == {"mx": [M, F4]} and mx[1]["weights"] == [{"mx": [D, F4]}]
        else:
            assert mx[0]["epilogue"] == NAT.EPI_BIAS and mx[0]["z"] is None
    if "qkv" in dgrad:
        assert mx[-1]["a"] == {"mx": [M, 3 * D]} and mx[-1]["weights"] == [{"mx": [D, 3 * D]}]
        assert mx[-1]["epilogue"] == NAT.EPI_BIAS


def test_transposed_mx_weights_are_built_at_the_first_backward_only():
    blk = _block()
    fwd, first = _step(blk, "all", twice=False)
    assert "transpose" not in _names(fwd) and _names(fwd) == INFERENCE
    extra = _names(first)
    assert extra.count("transpose") == 6 and extra.count("mx_quantize") == 1 + 4  # W2, W1, W_out, Wq | Wk | Wv
    _, again = _step(blk, "all", twice=False)
    assert _names(again) == BACKWARD[ALL]


@pytest.mark.parametrize("mode", ["attention", "recompute"])
def test_recompute_front_runs_the_fp8_stages(mode):
    """What the forward did not keep the backward recomputes with the fp8 stages: FF1 under EPI_BIAS into z alone, the
    q / k norms beside the recomputed projection, the attention only where its output was not kept."""
    from videopainter_amd import _native as NAT
    _, bwd = _step(_block(), mode)
    front = ["adaln_modulate_mx", "gemm_mx", "head_norm_rope", "head_norm_rope",
             *(["attention"] if mode == "recompute" else []), "mx_quantize", "gemm_mx", "adaln_modulate_mx", "gemm_mx"]
    assert _names(bwd) == front + BACKWARD[ALL]
    ff1 = bwd[len(front) - 1]["args"]
    assert ff1["epilogue"] == NAT.EPI_BIAS and ff1["aux"] is None
    assert ff1["out"] == {"shape": [M, F4], "stride": [F4, 1], "dtype": "bfloat16"}


def test_refusals_need_no_device():
    from videopainter_amd import autograd as AG
    x, temb, rope, _, _ = _inputs()
    blk = _block()
    blk.ff.net[0].proj.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="trains no parameter"):
        AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope)
    blk.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="time-embedding"):
        AG.block_apply(blk, x.clone().requires_grad_(), T, temb.clone().requires_grad_(), rope)
    blk.attn1.fp8_qk_exp = (0, 0)
    with pytest.raises(NotImplementedError, match="fp8 modes"):
        AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope)
