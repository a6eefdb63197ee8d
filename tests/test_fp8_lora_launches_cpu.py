"""The launch sequence of one CogVideoXBlock on the MX-FP8 GEMMs that carries unfused LoRA adapters on to_q / to_k /
to_v / to_out.0 — inference, the training forward, the backward's recompute and the backward — on the CPU, for the
standard processor and both backward forms of the resample processor, in both orders of enabling fp8 and attaching
the adapter.

The recorder of tests/test_fp8_training_launches_cpu.py (the MX entries and the device-free MXTensor), extended INSIDE
THIS TEST ONLY with the dual modulate entry.  Pinned: the sequence is the frozen fp8 block's plus exactly the side-path
launches — the dual modulate in place of the MX one, T = x A_cat^T and one low-rank GEMM per adapted projection added
in place onto the base qkv (EPI_BIAS_ADDROWS with addrows = C), T and the gated low-rank GEMM onto the residual before
to_out's MX GEMM, and in the backward `_aug_dgrad`'s bf16 launches after each base dgrad; without adapters the
sequence is the frozen fp8 block's own.  The whole traces (every scalar argument, shape / strides / dtype of every
tensor argument) are recorded in tests/golden/fp8_lora_launches.json; to record it:
    python -c "from tests.test_fp8_lora_launches_cpu import write_fixture; write_fixture()"
"""
import contextlib
import inspect
import json
import os

import pytest
import torch

from tests.test_block_launches_cpu import MODES
from tests.test_fp8_training_launches_cpu import (BACKWARD, INFERENCE, _MX, _describe_x, _names, _plain, _rows,
                                                  recording_mx)
from tests.test_fp8_training_launches_cpu import _block as _frozen_block
from tests.test_fp8_training_launches_cpu import _inference as _frozen_inference

GOLD = os.path.join(os.path.dirname(__file__), "golden", "fp8_lora_launches.json")
B, T, GRID, D, H, F4 = 2, 6, (2, 12, 12), 256, 4, 1024
NV = GRID[0] * GRID[1] * GRID[2]
N = T + NV
M = B * N  # 588: a multiple of neither 128 nor 256
ALL = ("ff2", "ff1", "out", "qkv")
RP = 64    # a projection's rank block, zero-padded to one 64-wide K-tile


@contextlib.contextmanager
def recording_side():
    """`recording_mx()` plus the dual modulate's recorder."""
    from videopainter_amd import kernels as K
    real = K.adaln_modulate_dual
    sig = inspect.signature(real)
    with recording_mx() as log:
        def rec(*args, **kw):
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            a = ba.arguments
            log.append({"entry": "adaln_modulate_dual", "args": {k: _describe_x(v) for k, v in a.items()}})
            out = a["out"] if a["out"] is not None else torch.empty_like(a["x"])
            return out, (a["out_mx"] if a["out_mx"] is not None else _MX(_rows(a["x"]), a["x"].shape[-1]))
        K.adaln_modulate_dual = rec
        try:
            yield log
        finally:
            K.adaln_modulate_dual = real


def _block(order="attach_first", resample=False, closed=False, rank=16, trainable=True, ffn=True, qkv=True, out=True,
           targets=("to_q", "to_k", "to_v", "to_out.0")):
    """A D = 256 block with adapters of `rank` on `targets` and the chosen MX-FP8 GEMMs; order: which came first
    (trainable q / k / v factors go on before the fp8 QKV projection: `test_both_orders...`).
    trainable: PEFT's add_adapter (B = 0), else a loaded adapter (attach_lora_, non-zero factors)."""
    from videopainter_amd.lora import add_trainable_adapter_, attach_lora_
    from videopainter_amd.transformer import CogVideoXBlock
    torch.manual_seed(3)
    blk = CogVideoXBlock(dim=D, num_attention_heads=H, attention_head_dim=64, time_embed_dim=32, attention_bias=True,
                         id_pool_resample_learnable=resample)
    blk.requires_grad_(False)

    def attach():
        if rank == 0:
            return
        if trainable:
            add_trainable_adapter_(blk, rank, float(rank), tuple(targets))
            return
        g = torch.Generator().manual_seed(9)
        sd = {}
        for t in targets:
            sd[f"attn1.{t}.lora_A.weight"] = torch.randn(rank, D, generator=g)
            sd[f"attn1.{t}.lora_B.weight"] = torch.randn(D, rank, generator=g)
        attach_lora_(blk, sd)

    def enable():
        with recording_side() as log:
            if ffn:
                blk.enable_fp8_ffn()
            if qkv:
                blk.enable_fp8_qkv()
            if out:
                blk.enable_fp8_out()
        assert _names(log) == ["mx_quantize"] * (2 * ffn + 3 * qkv + out)  # (the adapters add nothing here)
    for step in ((enable, attach) if order == "enable_first" else (attach, enable)):
        step()
    if closed:
        blk.enable_closed_form_resample_backward()
    return blk


def _inputs(resample=False):
    from oracle.cogvideox_oracle import prepare_rotary_positional_embeddings
    from videopainter_amd.attention_processor import _rope_dev
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, N, D, generator=g).to(torch.bfloat16)
    temb = torch.randn(B, 32, generator=g).to(torch.bfloat16)
    cos, sin = prepare_rotary_positional_embeddings(GRID[1] * 16, GRID[2] * 16, GRID[0], 64)
    rope = _rope_dev((cos.float(), sin.float()), x.device, GRID)
    rmask = None
    if resample:
        rmask = torch.zeros(B, N, dtype=torch.uint8)
        rmask[:, T:] = (torch.rand(B, NV, generator=g) < 0.5).to(torch.uint8)
    return x, temb, rope, rmask


def _inference(blk, resample=False):
    from videopainter_amd import attention_processor as AP
    x, temb, rope, rmask = _inputs(resample)
    AP._MASK_PLANS.clear()
    with torch.no_grad(), recording_side() as log:
        blk.forward_joint(x, T, temb, rope, resample_mask=rmask)
    AP._MASK_PLANS.clear()
    return _plain(log)


def _step(blk, mode, resample=False, dgrad=ALL):
    """(forward trace, backward trace) of the second block_apply + backward on the block at a keep mode (the
    transposed-weight caches filled by the first)."""
    from videopainter_amd import attention_processor as AP
    from videopainter_amd import autograd as AG
    x, temb, rope, rmask = _inputs(resample)
    saved = AG._room_for, AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION, AG.FP8_DGRAD
    AG._room_for = lambda *a, **k: True
    AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION = MODES[mode]
    AG.FP8_DGRAD = set(dgrad)
    try:
        for _ in range(2):
            AP._MASK_PLANS.clear()
            with recording_side() as log, torch.enable_grad():
                y = AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope, resample_mask=rmask)
                n_fwd = len(log)
                y.backward(torch.ones_like(y))
    finally:
        AG._room_for, AG.SAVE_ACTIVATIONS, AG.SAVE_ATTENTION, AG.FP8_DGRAD = saved
        AP._MASK_PLANS.clear()
    return _plain(log[:n_fwd]), _plain(log[n_fwd:])


# the side path's launches, by where they sit
QKV_SIDE = ["gemm"] * 4  # T = x A_cat^T, then q, k, v: rnd(rnd(T_i (s B_i)^T) + qkv) in place
OUT_SIDE = ["gemm"] * 2  # T = o A^T, then R' = rnd(x + rnd(gate rnd(T (s B)^T)))
FORWARD = ["adaln_modulate_dual", "gemm_mx", *QKV_SIDE, "head_norm_rope", "head_norm_rope", "attention", *OUT_SIDE,
           "mx_quantize", "gemm_mx", "adaln_modulate_mx", "gemm_mx", "gemm_mx"]
ATTN = ["attention_bwd", "head_norm_rope_bwd", "head_norm_rope_bwd"]
# `_aug_dgrad` with train: dT, dT A_cat, the add onto the base dgrad, then dB_i = s dy_i^T T_i per projection, dA = dT^T x
AUG_OUT = ["gemm", "gemm", "axpy", "wgrad", "wgrad"]
AUG_QKV = ["gemm", "gemm", "axpy", "wgrad", "wgrad", "wgrad", "wgrad"]
# (a block that trains q / k / v factors keeps the to_out dgrad on the bf16 GEMM: autograd.FP8_DGRAD_LORA_OFF)
BACKWARD_LORA = ["rowscale_mx", "gemm_mx", "gemm_mx", "adaln_bwd",                       # the FeedForward: as frozen
                 "rowscale", "gemm", "gemm", *AUG_OUT,                                    # to_out: T, base dgrad, adapter
                 *ATTN, "mx_quantize", "gemm_mx", *AUG_QKV, "adaln_bwd"]                  # QKV: base dgrad, adapter
# with the to_out dgrad in fp8 (FP8_DGRAD_LORA_OFF emptied, or adapters that do not train): the bf16 row-scale is the
# adapter's dy and the MX operand is quantised from it
OUT_MX = ["rowscale", "mx_quantize", "gemm_mx", "gemm", *AUG_OUT]


def _without_side(names):
    """The trace's names with the forward side path taken out: what a frozen fp8 block without adapters launches."""
    out = list(names)
    i = out.index("adaln_modulate_dual")
    assert out[i + 1:i + 6] == ["gemm_mx", *QKV_SIDE]
    out[i:i + 6] = ["adaln_modulate_mx", "gemm_mx"]
    j = len(out) - 1 - out[::-1].index("mx_quantize")  # (to_out's operand: the last quantisation of the forward)
    assert out[j - 2:j] == OUT_SIDE
    del out[j - 2:j]
    return out


@pytest.mark.parametrize("rank", [16, 64])
@pytest.mark.parametrize("trainable", [True, False], ids=["trainable", "loaded"])
def test_inference_is_the_fp8_forward_plus_the_side_path(rank, trainable):
    from videopainter_amd import _native as NAT
    log = _inference(_block(rank=rank, trainable=trainable))
    assert _names(log) == FORWARD and _without_side(_names(log)) == INFERENCE
    bf = lambda shape, stride: {"shape": shape, "stride": stride, "dtype": "bfloat16"}  # noqa: E731
    # the dual modulate: bf16 rows into the K-augmented operand [M, D + 3 x 64] (rank 16 zero-padded to 64 columns)
    assert log[0]["args"]["out"] == bf([B, N, D], [N * (D + 3 * RP), D + 3 * RP, 1])
    assert log[1]["args"]["a"] == {"mx": [M, D]} and log[1]["args"]["out"] == bf([M, 3 * D], [3 * D, 1])
    t = log[2]["args"]  # T into the operand's tail columns
    assert t["a"] == bf([M, D], [D + 3 * RP, 1]) and t["weights"] == [bf([3 * RP, D], [D, 1])]
    assert t["out"] == bf([M, 3 * RP], [D + 3 * RP, 1]) and t["epilogue"] == NAT.EPI_BIAS
    for l in log[3:6]:  # one launch per projection, in place on its columns of the base qkv
        a = l["args"]
        assert a["epilogue"] == NAT.EPI_BIAS_ADDROWS and a["biases"] == [None]
        assert a["a"] == bf([M, RP], [D + 3 * RP, 1]) and a["weights"] == [bf([D, RP], [RP, 1])]
        assert a["out"] == a["addrows"] == bf([M, D], [3 * D, 1])
        assert (a["rows_per_group"], a["group_stride"], a["row_offset"], a["addrows_offset"]) == (None, 0, 0, 0)
    to, gd, q8, mx = (l["args"] for l in log[9:13])
    assert to["a"] == bf([M, D], [D + RP, 1]) and to["out"] == bf([M, RP], [D + RP, 1])
    assert gd["epilogue"] == NAT.EPI_GATED and gd["biases"] == [None] and gd["a"] == bf([M, RP], [D + RP, 1])
    assert gd["resid"] == bf([M, D], [D, 1]) and gd["out"] == bf([M, D], [D, 1])
    assert (gd["gate_chunk"], gd["gate_text_chunk"], gd["tokens_per_batch"], gd["text_len"]) == (2, 5, N, T)
    assert q8["x"] == bf([M, D], [D + RP, 1])  # o, the operand's first columns
    assert mx["epilogue"] == NAT.EPI_GATED and mx["resid"] == bf([M, D], [D, 1]) and mx["biases"] != [None]


def test_without_adapters_the_trace_is_the_frozen_fp8_block_s():
    """No adapter attached, or a loaded one folded by fuse_lora: the frozen fp8 block's own launches (the traces of
    tests/test_fp8_training_launches_cpu.py, which this file leaves as they are, pin them at that test's shapes)."""
    from videopainter_amd.lora import fuse_lora_
    assert _names(_frozen_inference(_frozen_block())) == INFERENCE
    want = _inference(_block(rank=0))
    assert _names(want) == INFERENCE
    blk = _block(trainable=False)
    with recording_side() as log:  # (a model's fold re-quantises its blocks' fp8 weights; a bare block is no model)
        fuse_lora_(blk)
        blk.enable_fp8_qkv()
        blk.enable_fp8_out()
    assert _names(log) == ["mx_quantize"] * 4
    assert _inference(blk) == want


@pytest.mark.parametrize("form", ["standard", "explicit", "closed"])
def test_both_orders_give_the_same_launches(form):
    """A loaded adapter (load_lora_weights) attached before or after enable_fp8_*: the same launches, inference and
    training step.  A TRAINABLE adapter on q / k / v goes on first: add_adapter after enable_fp8_qkv still raises, before
    anything is attached (tests/test_lora_cpu.py pins that), while to_out's may come in either order."""
    from videopainter_amd.lora import add_trainable_adapter_
    resample, closed = form != "standard", form == "closed"
    a = _block("enable_first", resample, closed, trainable=False)
    b = _block("attach_first", resample, closed, trainable=False)
    assert _inference(a, resample) == _inference(b, resample)
    assert _step(a, "recompute", resample) == _step(b, "recompute", resample)
    blk = _block(rank=0, resample=resample)
    with pytest.raises(NotImplementedError, match="fp8 QKV"):
        add_trainable_adapter_(blk, 16, 16.0)
    assert not any(hasattr(m, "lora_A") for m in blk.modules())
    add_trainable_adapter_(blk, 16, 16.0, ("to_out.0",))
    assert hasattr(blk.attn1.to_out[0], "lora_A")


@pytest.mark.parametrize("mode", MODES)
def test_training_forward_and_backward_standard(mode):
    from videopainter_amd import _native as NAT
    blk = _block()
    fwd, bwd = _step(blk, mode)
    assert _names(fwd) == FORWARD
    front = []
    if mode != "all":  # the recompute: the forward's stages, FF1 storing z alone, the attention where it was not kept
        front = ["adaln_modulate_dual", "gemm_mx", *QKV_SIDE, "head_norm_rope", "head_norm_rope",
                 *(["attention"] if mode == "recompute" else []), *OUT_SIDE, "mx_quantize", "gemm_mx",
                 "adaln_modulate_mx", "gemm_mx"]
    assert _names(bwd) == front + BACKWARD_LORA
    # the same backward without the adapters' launches is the frozen block's
    frozen = [n for n in BACKWARD[ALL] if n != "mask_scale_rows"]  # (that test injects a branch sample)
    assert frozen == ["rowscale_mx", "gemm_mx", "gemm_mx", "adaln_bwd", "rowscale_mx", "gemm_mx", *ATTN, "mx_quantize",
                      "gemm_mx", "adaln_bwd"]
    b = bwd[len(front):]
    assert [l["args"]["epilogue"] for l in b if l["entry"] == "gemm_mx"] == [NAT.EPI_GELU_BWD_MXFP8, NAT.EPI_BIAS,
                                                                              NAT.EPI_BIAS]
    assert all(l["args"]["epilogue"] == NAT.EPI_BIAS for l in b if l["entry"] == "gemm")  # the low-rank backward: bf16
    wg = [l["args"] for l in b if l["entry"] == "wgrad"]
    shapes = [(a["dy"]["shape"], a["x"]["shape"]) for a in wg]
    assert shapes == [([M, D], [M, RP]), ([M, RP], [M, D]),                                  # to_out: dB, dA
                      ([M, D], [M, RP]), ([M, 3 * RP], [M, D]), ([M, D], [M, RP]), ([M, D], [M, RP])]  # q dB, dA, k, v


@pytest.mark.parametrize("off", ALL)
def test_one_dgrad_in_bf16_keeps_the_low_rank_backward(off):
    """A name out of FP8_DGRAD moves that base dgrad to the bf16 GEMM; the adapters' launches stay.  ("out" is on the
    bf16 GEMM already under trainable q / k / v factors.)"""
    _, bwd = _step(_block(), "all", dgrad=[n for n in ALL if n != off])
    n = _names(bwd)
    assert n.count("wgrad") == 6 and n.count("axpy") == 2
    moved = 0 if off == "out" else 1
    assert n.count("gemm_mx") == 3 - moved and n.count("gemm") == BACKWARD_LORA.count("gemm") + moved


def test_to_out_dgrad_in_fp8_where_no_qkv_factor_trains(monkeypatch):
    """The to_out dgrad runs on the fp8 GEMM under adapters when FP8_DGRAD_LORA_OFF is emptied (the A/B arm), and
    by default for adapters that do not train (a loaded adapter: `_aug_dgrad` adds dT A_cat alone)."""
    from videopainter_amd import autograd as AG
    i = BACKWARD_LORA.index("rowscale")
    monkeypatch.setattr(AG, "FP8_DGRAD_LORA_OFF", set())
    _, bwd = _step(_block(), "all")
    assert _names(bwd) == BACKWARD_LORA[:i] + OUT_MX + BACKWARD_LORA[i + 3 + len(AUG_OUT):]
    monkeypatch.undo()
    _, bwd = _step(_block(trainable=False), "all")
    dx_only = ["gemm", "gemm", "axpy"]
    assert _names(bwd) == ["rowscale_mx", "gemm_mx", "gemm_mx", "adaln_bwd", "rowscale", "mx_quantize", "gemm_mx",
                           *dx_only, *ATTN, "mx_quantize", "gemm_mx", *dx_only, "adaln_bwd"]


@pytest.mark.parametrize("form,mode", [("explicit", "recompute"), ("closed", "attention")])
def test_resample_forms(form, mode):
    """The resample processor on the fp8 QKV / output projections with adapters (refused before): the forward hands
    the pre-norm qkv over, the backward's recompute reads its columns as "qpre" / "kpre" and runs the form's norm
    launches from them — no bf16 QKV GEMM anywhere."""
    closed = form == "closed"
    blk = _block(resample=True, closed=closed)
    fwd, bwd = _step(blk, mode, resample=True)
    n = _names(fwd)
    assert n[:6] == ["adaln_modulate_dual", "gemm_mx", *QKV_SIDE] and n.count("attention") == 1
    assert n[-7:] == [*OUT_SIDE, "mx_quantize", "gemm_mx", "adaln_modulate_mx", "gemm_mx", "gemm_mx"]
    assert _inference(blk, True) == [dict(l, args=dict(l["args"], lse=None)) if l["entry"] == "attention" else l
                                     for l in fwd]
    nb = _names(bwd)
    assert nb[:6] == ["adaln_modulate_dual", "gemm_mx", *QKV_SIDE]
    assert nb.count("attention") == (0 if closed else 1) and nb.count("attention_bwd") == 1
    assert nb.count("null_key_mass_bwd") == (1 if closed else 0)
    assert nb.count("wgrad") == 6 and nb.count("gemm_mx") == 3 + 3  # recompute: QKV, to_out, FF1; three base dgrads
    # every bf16 GEMM of the step but the to_out dgrad is low-rank: K or N is a rank block
    full = [l["args"] for l in fwd + bwd if l["entry"] == "gemm"
            and not set(l["args"]["weights"][0]["shape"]) & {RP, 3 * RP}]
    assert len(full) == 1 and full[0]["weights"] == [{"shape": [D, D], "stride": [D, 1], "dtype": "bfloat16"}]


def test_ffn_alone_in_fp8_under_bf16_adapters():
    """enable_fp8_ffn alone on a block whose attention projections carry trainable adapters (refused before: the
    guard looked at the whole block): the bf16 K-augmented projections, the fp8 FeedForward and both its dgrads."""
    blk = _block(qkv=False, out=False)
    fwd, bwd = _step(blk, "all")
    assert _names(fwd) == ["adaln_modulate", "gemm", "gemm", "attention", "gemm", "gemm", "adaln_modulate_mx",
                           "gemm_mx", "gemm_mx"]
    n = _names(bwd)
    assert n[:4] == ["rowscale_mx", "gemm_mx", "gemm_mx", "adaln_bwd"] and n.count("gemm_mx") == 2
    assert n.count("wgrad") == 6


def test_refusals_still_raised():
    from videopainter_amd import autograd as AG
    x, temb, rope, _ = _inputs()
    for p in ("attn1.to_q.weight", "attn1.to_out.0.bias", "norm1.norm.weight", "attn1.norm_q.weight",
              "norm2.linear.weight", "ff.net.2.bias"):
        blk = _block()
        dict(blk.named_parameters())[p].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="trains no parameter"):
            AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope)
    blk = _block(rank=0, resample=True)
    x, temb, rope, rmask = _inputs(True)
    with pytest.raises(NotImplementedError, match="resample"):  # (lifted for blocks that carry adapters only)
        AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope, resample_mask=rmask)
    blk = _block()
    with pytest.raises(NotImplementedError, match="time-embedding"):
        AG.block_apply(blk, x.clone().requires_grad_(), T, temb.clone().requires_grad_(), rope)
    blk.attn1.fp8_qk_exp = (0, 0)
    with pytest.raises(NotImplementedError, match="fp8 modes"):
        AG.block_apply(blk, x.clone().requires_grad_(), T, temb, rope)


# ------------------------------------------------------------------------------------------------------------------
# the recorded traces
# ------------------------------------------------------------------------------------------------------------------

CASES = {
    "inference_standard_r16": lambda: _inference(_block()),
    "inference_standard_r64_loaded": lambda: _inference(_block(rank=64, trainable=False)),
    "inference_resample": lambda: _inference(_block(resample=True), True),
    **{f"step_standard_{m}": (lambda m=m: sum(_step(_block(), m), [])) for m in MODES},
    "step_explicit": lambda: sum(_step(_block(resample=True), "recompute", True), []),
    "step_closed_form": lambda: sum(_step(_block(resample=True, closed=True), "attention", True), []),
    "step_ffn_alone": lambda: sum(_step(_block(qkv=False, out=False), "all"), []),
}


def write_fixture(path: str = GOLD) -> None:
    """{"launches": [every distinct launch, one per line], "cases": {case: [indices into launches]}}."""
    index, cases = {}, {}
    for name, run in CASES.items():
        cases[name] = [index.setdefault(json.dumps(l, sort_keys=True, separators=(",", ":")), len(index))
                       for l in run()]
    with open(path, "w") as f:
        f.write('{"launches": [\n' + ",\n".join(index) + '\n],\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(n)}: {json.dumps(ix, separators=(',', ':'))}" for n, ix in cases.items()))
        f.write("\n}}\n")


@pytest.mark.parametrize("case", CASES)
def test_trace_equals_the_recorded_one(case):
    with open(GOLD) as f:
        gold = json.load(f)
    want = [gold["launches"][i] for i in gold["cases"][case]]
    got = CASES[case]()
    assert _names(got) == _names(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: launch {i} ({g['entry']}) differs"
