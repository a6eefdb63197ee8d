"""The launch sequence of one ID-resample block with the fp8 two-segment attention, on the CPU: the rehearsal of the
host logic of `CogVideoXAttnProcessor2_0_resample.attend_heads` on a machine without a GPU.

The recorder of tests/test_block_launches_cpu.py, extended INSIDE THIS TEST ONLY with recorders for the fp8
entries the path calls.  The rope carries the video grid and is CogVideoX's separable 3D table
(rebuilt from random per-axis factors), so the processor's plan sums the null keys in closed form — the one form the
fp8 path takes.  With the switch off the block must issue today's launches (golden case e_resample_k2_full for a
rope without a grid, and for the grid rope the same trace as a block that never heard of the switch)."""
import contextlib
import inspect
import json
import os

import pytest
import torch

from tests.test_block_launches_cpu import B, D, H, N, NV, T, _block, _describe, _empty, recording

GOLD = os.path.join(os.path.dirname(__file__), "golden", "block_launches.json")
GRID = (2, 12, 12)  # F * Hh * Ww = NV video rows
assert GRID[0] * GRID[1] * GRID[2] == NV


class _VPacked:  # what v_pack_fp8 returns, without a device
    def __init__(self, v, heads):
        Bv, n, _ = v.shape
        self.n, self.npad = n, (n + 63) // 64 * 64
        self.vt = _empty(Bv * heads * 64 * self.npad, like=v, dtype=torch.uint8)
        self.vs = _empty(Bv * heads * (self.npad // 64) * 128, like=v, dtype=torch.uint8)


def _describe_x(v):
    if isinstance(v, _VPacked):
        return {"vpacked": {"n": v.n, "npad": v.npad, "vt": _describe(v.vt), "vs": _describe(v.vs)}}
    return _describe(v)


_RETURNS_X = {
    "head_norm_rope_fp8": lambda a: a["out"] if a["out"] is not None else _empty(
        a["x_in"].shape[0], a["x_in"].shape[1], a["heads"] * 64, like=a["x_in"], dtype=torch.uint8),
    "v_pack_fp8": lambda a: _VPacked(a["v"], a["heads"]),
    "attention_fp8": lambda a: a["out"],
}  # (the closed-form null-key entries are the shared recorder's, tests/launch_recorder.py)


@contextlib.contextmanager
def recording_fp8():
    """`recording()` plus recorders for the fp8 / null-key entries; the tensors themselves are kept beside the log
    (`raw`) so a test can check which tensor went where."""
    from videopainter_amd import kernels as K
    from videopainter_amd import attention_processor as AP
    from tests.test_block_launches_cpu import _RETURNS
    saved = {}
    AP._MASK_PLANS.clear()
    sigs = {n: inspect.signature(getattr(K, n)) for n in _RETURNS}
    with recording() as log:
        raw = []

        def keep_raw(name, rec):  # around a recorder of `recording()`: the same log entry, plus the tensors
            def f(*args, **kw):
                ba = sigs[name].bind(*args, **kw)
                ba.apply_defaults()
                ret = rec(*args, **kw)
                raw.append((len(log) - 1, name, dict(ba.arguments), ret))
                return ret
            return f
        for n in _RETURNS:  # (restored by `recording()` itself on exit)
            setattr(K, n, keep_raw(n, getattr(K, n)))

        def recorder(name, real):
            sig = inspect.signature(real)

            def rec(*args, **kw):
                ba = sig.bind(*args, **kw)
                ba.apply_defaults()
                ret = _RETURNS_X[name](ba.arguments)
                log.append({"entry": name, "args": {k: _describe_x(v) for k, v in ba.arguments.items()}})
                raw.append((len(log) - 1, name, dict(ba.arguments), ret))
                return ret
            return rec
        try:
            for n in _RETURNS_X:
                saved[n] = getattr(K, n)
                setattr(K, n, recorder(n, saved[n]))
            yield log, raw
        finally:
            for n, f in saved.items():
                setattr(K, n, f)
            AP._MASK_PLANS.clear()


def _grid_rope(seed=7):
    """CogVideoX's separable 3D table [F*Hh*Ww, 64]: dims 0-15 by frame, 16-39 by row, 40-63 by column."""
    from videopainter_amd.attention_processor import RopeTables
    g = torch.Generator().manual_seed(seed)
    F_, Hh, Ww = GRID
    tabs = []
    for _ in range(2):
        t_, y_, x_ = (torch.randn(n, w, generator=g) for n, w in ((F_, 16), (Hh, 24), (Ww, 24)))
        tabs.append(torch.cat([t_[:, None, None, :].expand(F_, Hh, Ww, 16), y_[None, :, None, :].expand(F_, Hh, Ww, 24),
                               x_[None, None, :, :].expand(F_, Hh, Ww, 24)], dim=-1).reshape(NV, 64).contiguous())
    rope = RopeTables(tabs)
    rope.grid = GRID
    return rope


def _inputs():
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    x = torch.randn(B, N, D, generator=g).to(bf)
    temb = torch.randn(B, 32, generator=g).to(bf)
    rmask = torch.zeros(B, N, dtype=torch.uint8)
    rmask[:, T:] = (torch.rand(B, NV, generator=g) < 0.5).to(torch.uint8)
    prev = torch.randn(B, N, D, generator=g).to(bf)
    return x, temb, rmask, prev


def _run(blk, rope, prev=None, w=None):
    x, temb, rmask, prev_x = _inputs()
    kw = {}
    if prev:
        kw = dict(prev_joint=prev_x, prev_clip_weight=w, prev_resample_mask=rmask)
    with torch.no_grad(), recording_fp8() as (log, raw):
        blk.forward_joint(x, T, temb, rope, resample_mask=rmask, **kw)
    return json.loads(json.dumps(log)), raw


def test_switch_signatures():
    """The opt-in reaches every level; on the parent commit `resample=` is a TypeError."""
    from videopainter_amd import CogVideoXTransformer3DModel
    blk = _block(resample=True)
    blk.enable_fp8_attention(True, resample=True)
    assert blk.attn1.fp8_resample is True and blk.attn1.fp8_qk_exp is not None
    blk.enable_fp8_attention()  # the default stays off
    assert blk.attn1.fp8_resample is False and blk.attn1.fp8_qk_exp is not None
    blk.enable_fp8_attention(True, resample=True)
    blk.enable_fp8_attention(False)  # clears both
    assert blk.attn1.fp8_resample is False and blk.attn1.fp8_qk_exp is None
    for fn in (CogVideoXTransformer3DModel.enable_fp8_attention, type(blk).enable_fp8_attention):
        assert inspect.signature(fn).parameters["resample"].default is False
    assert inspect.signature(CogVideoXTransformer3DModel.enable_fp8).parameters["resample_attention"].default is False


@pytest.mark.parametrize("window", ["w0", "later"])
def test_switch_on_launch_sequence(window):
    """The five steps of the fp8 path, in order, with the plan's cnt as lens / k2_len and the documented tensors."""
    blk = _block(resample=True)
    blk.enable_fp8_attention(True, resample=True)
    q_exp, k_exp = blk.attn1.fp8_qk_exp
    rope = _grid_rope()
    later = window == "later"
    log, raw = _run(blk, rope, prev=later, w=0.3)
    names = [l["entry"] for l in log]
    steps = ["head_norm_rope_fp8", "head_norm_rope_fp8", "v_pack_fp8",        # 1: q8, k8, vp
             "head_norm_rope_fp8",                                            # 2: k2_8 (masked, permuted)
             "mask_scale_rows", "v_pack_fp8",                                 # 3: v2, vp2 (lens = cnt)
             "head_norm_rope", "null_key_mass",                               # 4: q in place, l_extra
             "attention_fp8"]                                                 # 5
    a0 = names.index("head_norm_rope_fp8")
    assert names[a0:a0 + len(steps)] == steps, names
    assert "attention" not in names and names.count("attention_fp8") == 1
    # before them: the mask plan (once) and the projections (QKV, and the previous window's K / V)
    assert names[:a0].count("partition_rows_index") == 1 and names[:a0].count("mask_null_segments") == 1
    assert names[:a0].count("gemm") == (2 if later else 1) and names[a0 - 1] == "gemm"
    by = {i: (n, a, r) for i, n, a, r in raw}
    cnt = by[names.index("partition_rows_index")][2][1]  # the plan's count: partition_rows_index -> (dst, counts)
    q8c, k8c, vpc, k2c, msc, vp2c, hnc, nkc, atc = (by[a0 + j] for j in range(9))
    scale = blk.attn1.scale
    from videopainter_amd import kernels as K
    # 1: the pre-norm q / k views of the fused projection, Q's factor carrying scale * log2 e
    assert q8c[1]["out_mul"] == scale * K.LOG2E * 2.0 ** q_exp and k8c[1]["out_mul"] == 2.0 ** k_exp
    for c in (q8c, k8c):
        assert tuple(c[1]["x_in"].shape) == (B, N, D) and c[1]["x_in"].stride(1) == 3 * D
        assert c[1]["tok_mask"] is None and c[1]["dst_rows"] is None and c[1]["out"] is None
    assert tuple(vpc[1]["v"].shape) == (B, N, D) and vpc[1]["lens"] is None
    # 2: the masked rows through the permuted fp8 norm into a [B, N, D] uint8 buffer, K's factor
    assert k2c[1]["out"].dtype == torch.uint8 and tuple(k2c[1]["out"].shape) == (B, N, D)
    assert k2c[1]["out_mul"] == 2.0 ** k_exp and k2c[1]["tok_mask"] is not None and k2c[1]["dst_rows"] is not None
    assert k2c[1]["pre_scale"] == (0.3 if later else 1.0)
    assert tuple(k2c[1]["dst_rows"].shape) == (B, N) and k2c[1]["dst_rows"].dtype == torch.int32
    if later:  # the previous window's K projection, not this window's k
        assert k2c[1]["x_in"].stride(1) == 2 * D and msc[1]["x_in"].stride(1) == 2 * D
    else:
        assert k2c[1]["x_in"].data_ptr() == k8c[1]["x_in"].data_ptr()
    # 3: v2 in bf16 for N rows, packed with the device-side count as lens
    assert msc[1]["out"].dtype == torch.bfloat16 and tuple(msc[1]["out"].shape) == (B, N, D)
    assert msc[1]["scale"] == (0.3 if later else 1.0) and msc[1]["dst_rows"] is k2c[1]["dst_rows"]
    assert vp2c[1]["v"] is msc[1]["out"] and vp2c[1]["lens"] is cnt
    # 4: q normed in place after q8 read it, then the null-key mass from it
    assert hnc[1]["x_in"].data_ptr() == q8c[1]["x_in"].data_ptr()
    assert hnc[1]["x_out"].data_ptr() == hnc[1]["x_in"].data_ptr()
    assert nkc[1]["q"].data_ptr() == hnc[1]["x_out"].data_ptr() and tuple(nkc[1]["grid"]) == GRID
    # 5: one call with both segments, the count and the mass
    a = atc[1]
    assert a["q8"] is q8c[2] and a["k8"] is k8c[2] and a["vp"] is vpc[2]
    assert a["k2"] is k2c[1]["out"] and a["vp2"] is vp2c[2] and a["k2_len"] is cnt and a["l_extra"] is nkc[2]
    assert a["k2_len"].dtype == torch.int32 and tuple(a["k2_len"].shape) == (B,)
    assert a["l_extra"].dtype == torch.float32 and tuple(a["l_extra"].shape) == (B, H, N)
    assert (a["q_exp"], a["k_exp"], a["out_scale"], a["accumulate"]) == (q_exp, k_exp, 1.0, False)
    assert tuple(a["out"].shape) == (B, N, D) and a["out"].dtype == torch.bfloat16


def test_switch_off_is_todays_trace():
    """Off (never set, set without `resample`, or cleared) the block issues today's launches: for a rope without a
    grid the recorded golden case e_resample_k2_full, for the grid rope the trace of an untouched block."""
    from tests.test_block_launches_cpu import _inputs as base_inputs
    with open(GOLD) as f:
        want = json.load(f)["e_resample_k2_full"]
    x, temb, rope = base_inputs()
    g = torch.Generator().manual_seed(6)
    rmask = torch.zeros(B, N, dtype=torch.uint8)
    rmask[:, T:] = (torch.rand(B, NV, generator=g) < 0.5).to(torch.uint8)

    def trace(blk):
        with torch.no_grad(), recording_fp8() as (log, _):
            blk.forward_joint(x, T, temb, rope, resample_mask=rmask)
        return json.loads(json.dumps(log))

    # a rope without a grid: bf16 whatever the switch says (no closed-form plan)
    blk = _block(resample=True)
    assert trace(blk) == want
    blk.enable_fp8_attention(True, resample=True)
    blk.enable_fp8_attention(False)
    assert trace(blk) == want
    # the grid rope: opted in and cleared again equals never opted in
    grope = _grid_rope()
    plain, _ = _run(_block(resample=True), grope)
    assert "attention" in [l["entry"] for l in plain] and "attention_fp8" not in [l["entry"] for l in plain]
    blk.enable_fp8_attention(True, resample=True)
    blk.enable_fp8_attention(False)
    assert _run(blk, grope)[0] == plain
