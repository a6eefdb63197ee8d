"""Training through frozen blocks on the MX-FP8 GEMMs (enable_fp8_ffn / _qkv / _out), forward and dgrad — GPU tests.

The blocks: a small one (D = 256: 4 heads x 64, FF 1024, time_embed 32; counter weights from the generators of
tests/golden/cases.py; B = 2, T = 8, 288 video tokens) for the structural properties, and the full-width block of
`full_block_case()` (config-1 shape, B = 1, T = 226, 1 152 video tokens).

The band of an input gradient is the rule of `fp8_block_gate` (tests/test_model_gpu.py), restated here:
r8 <= 5 * r16, with r8 = rel(HIP fp8, oracle fp32) and r16 = rel(oracle bf16 autograd, oracle fp32) of the same
gradient — one block is one rounding deep, and e4m3's 3-bit mantissa has 16x bf16's rounding step (per-element noise
~16x, ~4x after the block's averaging sums).  The rule was established on the forward; the tests print r8, r16, their
ratio and, as a yardstick, the same ratio for the fp8 block's forward output.

Measured on an MI355X (profiles/fp8_training_gpu_tests.log), dx r8 / r16 = ratio | the forward's ratio:
  full-width block, all four dgrads in fp8        1.229e-2 / 2.672e-3 = 4.60 | 4.31   (gated: <= 5)
  full-width block, FP8_DGRAD emptied              6.579e-3 / 2.672e-3 = 2.46 | 4.31   (gated)
  full-width, one dgrad in bf16: ff2 3.70, ff1 3.70, out 4.59, qkv 4.59               (gated)
  full-width resample block, fp8 FFN alone         1.214e-2 / 2.669e-3 = 4.55 | 4.16   (gated)
  small block (D = 256), all four dgrads in fp8    1.745e-2 / 2.996e-3 = 5.82 | 5.59   (printed: its forward, existing
                                                    code, is itself outside the band)
  small block, FP8_DGRAD emptied                   9.665e-3 / 2.996e-3 = 3.23 | 5.59   (printed)
  small resample block, fp8 FFN alone              1.666e-2 / 2.964e-3 = 5.62 | 5.17   (printed)
  model step: every used branch gradient 0.49 - 1.28 x the oracle's bf16 drift (gated: <= 5 x + 1e-3)
"""
import functools

import pytest
import torch

from tests.golden.cases import TINY_BRANCH_CFG, TINY_CFG, full_block_case, tiny_inputs

pytestmark = pytest.mark.gpu
dev = "cuda"
FP8_BLOCK_MUL = 5.0  # fp8_block_gate (tests/test_model_gpu.py): 5x the oracle's own bf16 drift of one block
MODEL_ADD = 1e-3     # the training tests' additive term (tests/test_training_gpu.py GATE_ADD)
SMALL_CFG = dict(TINY_CFG, num_attention_heads=4)

def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------
# the two blocks, their inputs and the oracle's gradients (computed once per session, never modified)
# ------------------------------------------------------------------------------------------------------------------

def _block_weights(dim, temb, seed=0):
    from videopainter_amd.config import block_shapes
    from videopainter_amd.weights import synth_state_dict
    s2 = {}
    for k, v in block_shapes(dim, temb).items():
        if k == "attn1.to_q.weight":
            for n in ("norm_q", "norm_k"):
                s2[f"attn1.{n}.weight"] = (64,)
                s2[f"attn1.{n}.bias"] = (64,)
        s2[k] = v
    w = synth_state_dict({"SB." + k: v for k, v in s2.items()}, seed)
    return {k[3:]: v for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _case(kind):
    """dict(weights, x [B, N, D], temb, dout, rope, T, heads, temb_dim) in bf16-rounded CPU tensors."""
    if kind == "full":
        c = full_block_case()
        T, heads, x = 226, 48, torch.cat([c["e"], c["h"]], 1)
        weights, temb, rope = c["weights"], c["temb"], c["rope"]
    else:
        i = tiny_inputs()
        T, heads = 8, 4
        g = torch.Generator().manual_seed(41)
        x = torch.randn(2, T + 288, 256, generator=g)
        temb = torch.randn(2, 32, generator=g)
        weights, rope = _block_weights(256, 32), i["rope"]
    g = torch.Generator().manual_seed(43)
    dout = torch.randn(x.shape, generator=g)
    return dict(weights=weights, x=x.bfloat16(), temb=temb.bfloat16(), dout=dout.bfloat16(), rope=rope, T=T,
                heads=heads, temb_dim=temb.shape[1])


@functools.lru_cache(maxsize=None)
def _oracle(kind, resample=False):
    """(out32, dx32, out16, dx16): the oracle's block forward + autograd in fp32 and in bf16 on the bf16 weights."""
    from oracle import cogvideox_oracle as O
    c = _case(kind)
    T = c["T"]
    cfg = dict(num_attention_heads=c["heads"], norm_eps=1e-5)
    kw = {}
    if resample:
        cfg["id_pool_resample_learnable"] = True
        kw = dict(resample=True)
    res = []
    for dtype in (torch.float32, torch.bfloat16):
        sd = {"b." + k: torch.from_numpy(v).to(torch.bfloat16).to(dtype) for k, v in c["weights"].items()}
        x = c["x"].to(dtype).clone().requires_grad_()  # (a copy: the cached case stays as it is)
        if resample:
            kw["resample_mask"] = _resample_mask(c).to(dtype)
        h, e = O.block_forward(sd, "b", cfg, x[:, T:], x[:, :T], c["temb"].to(dtype), c["rope"], **kw)
        out = torch.cat([e, h], 1)
        out.backward(c["dout"].to(dtype))
        res += [out.detach(), x.grad]
    return tuple(res)


def _resample_mask(c):
    g = torch.Generator().manual_seed(47)
    B, N = c["x"].shape[:2]
    m = torch.zeros(B, N, dtype=torch.bool)
    m[:, c["T"]:] = torch.rand(B, N - c["T"], generator=g) < 0.4
    return m


def _block(kind, ffn=True, qkv=True, out=True, resample=False):
    """A frozen block on the device with the chosen MX-FP8 GEMMs."""
    from videopainter_amd import device_scope
    from videopainter_amd.transformer import CogVideoXBlock
    c = _case(kind)
    with device_scope(dev):
        blk = CogVideoXBlock(dim=c["x"].shape[-1], num_attention_heads=c["heads"], attention_head_dim=64,
                             time_embed_dim=c["temb_dim"], attention_bias=True, id_pool_resample_learnable=resample)
    with torch.no_grad():
        for k, p in blk.state_dict().items():
            p.copy_(torch.from_numpy(c["weights"][k]))
    blk.requires_grad_(False)
    if ffn:
        blk.enable_fp8_ffn()
    if qkv:
        blk.enable_fp8_qkv()
    if out:
        blk.enable_fp8_out()
    return blk


@functools.lru_cache(maxsize=None)
def _shared_block(kind):
    """The block with all three fp8 GEMMs, for the tests that only run it."""
    return _block(kind)


def _rope(c):
    return (c["rope"][0].to(dev), c["rope"][1].to(dev))


def _step(blk, c, inject=None, inject_mask=None, resample_mask=None):
    """block_apply + backward of the case's cotangent: (out, dx, dinject)."""
    from videopainter_amd.autograd import block_apply
    xd = c["x"].to(dev).requires_grad_()
    injd = inject.to(dev).requires_grad_() if inject is not None else None
    out = block_apply(blk, xd, c["T"], c["temb"].to(dev), _rope(c), injd, inject_mask, resample_mask)
    out.backward(c["dout"].to(dev))
    return out.detach(), xd.grad, injd.grad if injd is not None else None


def _report(name, out, dx, oracle):
    """Prints r8, r16 and their ratio for the gradient, and the forward's as the yardstick; returns the four."""
    o32, g32, o16, g16 = oracle
    r8, r16 = rel(dx.float(), g32), rel(g16.float(), g32)
    f8, f16 = rel(out.float(), o32), rel(o16.float(), o32)
    print(f"{name}: dx r8 {r8:.3e} r16 {r16:.3e} ratio {r8 / r16:.2f} | forward r8 {f8:.3e} r16 {f16:.3e} "
          f"ratio {f8 / f16:.2f}")
    return r8, r16, f8, f16


# ------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------

def test_frozen_fp8_block_trains_with_the_inference_forward_bits():
    """A frozen block with enable_fp8_ffn / _qkv / _out: block_apply then .backward() runs (it raised
    NotImplementedError before the fp8 dgrad existed), and block_apply's output is torch.equal to the same block's
    forward_joint under no_grad."""
    c = _case("small")
    blk = _block("small")
    out, dx, _ = _step(blk, c)
    assert float(dx.float().abs().max()) > 0 and bool(torch.isfinite(dx.float()).all())
    with torch.no_grad():
        ref = blk.forward_joint(c["x"].to(dev), c["T"], c["temb"].to(dev), _rope(c))
    assert torch.equal(out, ref)


@pytest.mark.parametrize("inject", [False, True], ids=["plain", "inject"])
def test_keep_levels_give_the_same_bits(monkeypatch, inject):
    """SAVE_ACTIVATIONS / SAVE_ATTENTION at (True, True), (False, True), (False, False): the same output, dx and
    dinject bits, with and without a branch sample injected under a mask."""
    from videopainter_amd import autograd as AG
    c = _case("small")
    blk = _block("small")
    g = torch.Generator().manual_seed(5)
    inj = torch.randn(2, 288, 256, generator=g).bfloat16() if inject else None
    inj_mask = (torch.rand(2, 288, generator=g) < 0.5).to(torch.uint8).to(dev) if inject else None
    res = []
    for acts, attn in ((True, True), (False, True), (False, False)):
        monkeypatch.setattr(AG, "SAVE_ACTIVATIONS", acts)
        monkeypatch.setattr(AG, "SAVE_ATTENTION", attn)
        res.append(_step(blk, c, inj, inj_mask))
    o0, gx0, gi0 = res[-1]
    assert float(gx0.float().abs().max()) > 0
    assert not inject or float(gi0.float().abs().max()) > 0
    for o1, gx1, gi1 in res[:-1]:
        assert torch.equal(o1, o0) and torch.equal(gx1, gx0)
        assert not inject or torch.equal(gi1, gi0)


@pytest.mark.parametrize("kind", ["small", "full"])
def test_input_gradient_against_the_oracle(kind):
    """dx of the fp8 block against the oracle's fp32 autograd: r8 <= 5 * r16 (module docstring), gated on the
    full-width block.  The small block's FORWARD — the fp8 inference forward, code older than the fp8 dgrad — is itself
    outside the 5x band (measured 5.59x; D = 256 averages over 12x fewer terms than D = 3072), so there the figures
    are printed only (gradient 5.82x) and the small block serves the structural tests."""
    c = _case(kind)
    blk = _shared_block(kind)
    out, dx, _ = _step(blk, c)
    with torch.no_grad():
        assert torch.equal(out, blk.forward_joint(c["x"].to(dev), c["T"], c["temb"].to(dev), _rope(c)))
    r8, r16, f8, f16 = _report(f"fp8 block ({kind})", out, dx, _oracle(kind))
    if kind == "full":
        assert r8 <= FP8_BLOCK_MUL * r16, (r8, r16)


@pytest.mark.parametrize("kind", ["small", "full"])
def test_bf16_dgrad_switch_launches_no_fp8_gemm(monkeypatch, kind):
    """FP8_DGRAD emptied: the forward stays fp8, the backward launches no gemm_mx (counted with
    kernels.timed_launches, the forward having kept everything: SAVE_ACTIVATIONS), and dx still passes the gate."""
    from videopainter_amd import autograd as AG
    from videopainter_amd import kernels as K
    from videopainter_amd.autograd import block_apply
    monkeypatch.setattr(AG, "SAVE_ACTIVATIONS", True)
    monkeypatch.setattr(AG, "_room_for", lambda *a, **k: True)
    c = _case(kind)
    blk = _shared_block(kind)
    counts = {}
    dxs = {}
    for name, names in (("fp8", {"ff2", "ff1", "out", "qkv"}), ("bf16", set())):
        monkeypatch.setattr(AG, "FP8_DGRAD", names)
        xd = c["x"].to(dev).requires_grad_()
        with K.timed_launches("gemm_mx") as fw:
            out = block_apply(blk, xd, c["T"], c["temb"].to(dev), _rope(c))
        with K.timed_launches("gemm_mx", "gemm") as bw:
            out.backward(c["dout"].to(dev))
        counts[name] = (fw.count("gemm_mx"), bw.count("gemm_mx"), bw.count("gemm"))
        dxs[name] = (out.detach(), xd.grad)
    print(f"{kind}: (forward gemm_mx, backward gemm_mx, backward gemm) {counts}")
    assert counts["fp8"] == (4, 4, 0)
    assert counts["bf16"] == (4, 0, 4)
    assert torch.equal(dxs["fp8"][0], dxs["bf16"][0])  # the forward does not depend on the switch
    r8, r16, _, _ = _report(f"fp8 forward, bf16 dgrad ({kind})", *dxs["bf16"], _oracle(kind))
    if kind == "full":  # (the small block's forward is outside the band: test_input_gradient_against_the_oracle)
        assert r8 <= FP8_BLOCK_MUL * r16, (r8, r16)


@pytest.mark.parametrize("off", ["ff2", "ff1", "out", "qkv"])
def test_each_dgrad_switch_alone(monkeypatch, off):
    """One name out of FP8_DGRAD: that dgrad alone moves to the bf16 GEMM (3 fp8 + 1 bf16 GEMM in the backward), and
    the full-width block's gradient stays within the band."""
    from videopainter_amd import autograd as AG
    from videopainter_amd import kernels as K
    from videopainter_amd.autograd import block_apply
    monkeypatch.setattr(AG, "SAVE_ACTIVATIONS", True)
    monkeypatch.setattr(AG, "_room_for", lambda *a, **k: True)
    monkeypatch.setattr(AG, "FP8_DGRAD", {"ff2", "ff1", "out", "qkv"} - {off})
    c = _case("full")
    blk = _shared_block("full")
    xd = c["x"].to(dev).requires_grad_()
    out = block_apply(blk, xd, c["T"], c["temb"].to(dev), _rope(c))
    with K.timed_launches("gemm_mx", "gemm") as bw:
        out.backward(c["dout"].to(dev))
    assert (bw.count("gemm_mx"), bw.count("gemm")) == (3, 1)
    r8, r16, _, _ = _report(f"fp8 block, {off} dgrad in bf16", out.detach(), xd.grad, _oracle("full"))
    assert r8 <= FP8_BLOCK_MUL * r16, (r8, r16)


def test_model_step_branch_gradients():
    """The reference's branch training step on a 4-layer transformer + 2-layer branch at D = 256: the transformer
    frozen with enable_fp8(attention=False), the branch trainable in bf16.  Every branch parameter gradient the
    oracle uses, against the oracle's fp32 autograd: r <= 5 * r16 + 1e-3 (depth 4 is nearer one block than 42, so the
    block rule applies; the additive term is the training tests').  No transformer parameter receives a gradient."""
    from oracle import cogvideox_oracle as O
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd.config import full_config, state_dict_shapes
    from videopainter_amd.weights import synth_state_dict
    bcfg = dict(SMALL_CFG, num_layers=TINY_BRANCH_CFG["num_layers"])
    tsd = synth_state_dict(state_dict_shapes(full_config(SMALL_CFG)), 0)
    bsd = synth_state_dict({("B." + k): v for k, v in state_dict_shapes(full_config(bcfg, True), True).items()}, 0)
    bsd = {k[2:]: v for k, v in bsd.items()}
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**SMALL_CFG)
        br = CogvideoXBranchModel(**bcfg)
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    br.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()})
    tr.requires_grad_(False)
    br.requires_grad_(True)
    tr.enable_fp8(attention=False)
    assert all(b.ff_mx is not None and b.qkv_mx is not None and b.out_mx is not None for b in tr.transformer_blocks)
    i = tiny_inputs()
    g = torch.Generator().manual_seed(6)
    R = torch.randn(i["video"].shape, generator=g).bfloat16()
    samples = br(hidden_states=i["video"].to(dev).bfloat16(), encoder_hidden_states=i["enc"].to(dev).bfloat16(),
                 branch_cond=i["branch_cond"].to(dev).bfloat16(), timestep=i["timestep"].to(dev),
                 image_rotary_emb=i["rope"], return_dict=False)[0]
    out = tr(hidden_states=i["hidden"].to(dev).bfloat16(), encoder_hidden_states=i["enc"].to(dev).bfloat16(),
             timestep=i["timestep"].to(dev), image_rotary_emb=i["rope"], branch_block_samples=samples,
             branch_block_masks=i["mask"].to(dev), return_dict=False)[0]
    assert out.requires_grad
    out.backward(R.to(dev))
    assert all(p.grad is None for p in tr.parameters())
    trainable = [n for n, _ in br.named_parameters()]
    ours = {n: p.grad for n, p in br.named_parameters()}

    def oracle(dtype):
        tp = {k: torch.from_numpy(v).to(dtype) for k, v in tsd.items()}
        bp = {k: torch.from_numpy(v).to(dtype).requires_grad_(k in trainable) for k, v in bsd.items()}
        s = O.branch_forward(bp, full_config(bcfg, True), i["video"].to(dtype), i["enc"].to(dtype),
                             i["branch_cond"].to(dtype), i["timestep"], i["rope"])
        o = O.transformer_forward(tp, full_config(SMALL_CFG), i["hidden"].to(dtype), i["enc"].to(dtype),
                                  i["timestep"], i["rope"], branch_block_samples=s,
                                  branch_block_masks=i["mask"].to(dtype))[0]
        o.backward(R.to(dtype))
        return o.detach(), {k: bp[k].grad for k in trainable}

    o32, gp32 = oracle(torch.float32)
    o16, gp16 = oracle(torch.bfloat16)
    print(f"model output: fp8 {rel(out.detach().float(), o32):.3e}  oracle-bf16 {rel(o16.float(), o32):.3e}")
    used = [n for n in trainable if gp32[n] is not None]
    assert used and sorted(n for n in trainable if ours[n] is None) == sorted(n for n in trainable
                                                                             if gp32[n] is None)
    worst = []
    for n in used:
        r, r16 = rel(ours[n].float(), gp32[n]), rel(gp16[n].float(), gp32[n])
        print(f"{n:56s} fp8 {r:.3e}  oracle-bf16 {r16:.3e}  ratio {r / max(r16, 1e-30):.2f}")
        if not r <= FP8_BLOCK_MUL * r16 + MODEL_ADD:
            worst.append((n, r, r16))
    assert not worst, worst


def test_refusals():
    """NotImplementedError for: the fp8 attention; an fp8 block with a trainable parameter; a temb that requires
    grad; qkv_mx on a resample-processor block."""
    from videopainter_amd.autograd import block_apply
    c = _case("small")
    x, temb, rope = c["x"].to(dev).requires_grad_(), c["temb"].to(dev), _rope(c)
    blk = _block("small")
    blk.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="fp8 modes"):
        block_apply(blk, x, c["T"], temb, rope)
    blk.enable_fp8_attention(False)
    blk.ff.net[2].bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="trains no parameter"):
        block_apply(blk, x, c["T"], temb, rope)
    blk.ff.net[2].bias.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="time-embedding"):
        block_apply(blk, x, c["T"], temb.clone().requires_grad_(), rope)
    block_apply(blk, x, c["T"], temb, rope)  # (and the frozen block with a constant temb goes through)
    rm = _resample_mask(c).to(dev).to(torch.uint8)
    for kw in (dict(ffn=False, qkv=True, out=False), dict(ffn=False, qkv=False, out=True)):
        rblk = _block("small", resample=True, **kw)
        with pytest.raises(NotImplementedError, match="resample"):
            block_apply(rblk, x, c["T"], temb, rope, resample_mask=rm)


@pytest.mark.parametrize("kind", ["small", "full"])
def test_fp8_ffn_alone_on_a_resample_block(kind):
    """ff_mx alone on a resample-processor block (the explicit 2N-key form): runs, with the inference forward's bits,
    and the full-width block's dx passes the block gate against the oracle's resample autograd (the small block's
    figures are printed)."""
    c = _case(kind)
    blk = _block(kind, ffn=True, qkv=False, out=False, resample=True)
    rm = _resample_mask(c).to(dev).to(torch.uint8)
    out, dx, _ = _step(blk, c, resample_mask=rm)
    with torch.no_grad():
        assert torch.equal(out, blk.forward_joint(c["x"].to(dev), c["T"], c["temb"].to(dev), _rope(c),
                                                  resample_mask=rm))
    r8, r16, _, _ = _report(f"fp8 FFN on a resample block ({kind})", out, dx, _oracle(kind, True))
    if kind == "full":
        assert r8 <= FP8_BLOCK_MUL * r16, (r8, r16)
