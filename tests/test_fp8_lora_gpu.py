"""MX-FP8 projections under unfused LoRA — GPU tests: the dual modulate kernel, the side path's bits, gradients
across the keep levels, and the accuracy of a block and of a tiny VideoPainterID training step against the oracle's
PEFT-unmerged twin (oracle/cogvideox_oracle.py `linear`: base(x) + lora_B(lora_A(x)) * scaling) and its autograd.

Blocks: D = 256 (4 heads x 64, FF 1024; 6 text rows + a 3 x 8 x 12 video grid: M = 294 at B = 1, 588 at B = 2, a
multiple of neither 128 nor 256) for the structural properties; the full-width config-1 block of
tests/test_fp8_training_gpu.py (D = 3072, T = 226, 1 152 video tokens) for accuracy.  Ranks 64 and 16 (16 is
zero-padded to one 64-column rank block).

Exact operands (test (c)): norm1 with w = 1, b = 0, eps = 0.75 on rows of +-0.5 in equal numbers gives xn = +-0.5
exactly (tests/gemm_refs.py, ADALN_EXACT); sparse integer weights and factors keep every accumulator an exactly
representable multiple of 1/2, e4m3 holds the integers -3 .. 3 exactly under any block scale, so the MX GEMM, T and
the low-rank GEMMs are exact and every rnd() of DESIGN §4's chain rounds an exactly known value once.

The accuracy band is the project's: r8 <= 5 x r16 for one block (fp8_block_gate, tests/test_model_gpu.py), r8 =
rel(HIP fp8, oracle fp32) and r16 = rel(oracle bf16, oracle fp32) of the same quantity; 1.5 x r16 for a model's forward
(fp8_model_gate); gradients of the 4-layer model 5 x r16 + 1e-3 as tests/test_fp8_training_gpu.py's model step.
A block that trains q / k / v factors keeps its to_out dgrad on the bf16 GEMM (autograd.FP8_DGRAD_LORA_OFF): with it
in e4m3 the full-width block's q / k factor gradients measured 5.5x and v's 6.2-6.4x, outside the band.

Measured on an MI355X (profiles/fp8_lora_gpu_tests.log), r8 / r16 per quantity, full-width block, rank 64:
  standard   output 4.36  dx 4.57  dA / dB: q 4.88 / 4.90  k 4.89 / 4.92  v 2.62 / 2.85  out 4.75 / 4.44
  explicit   output 4.32  dx 4.57           q 4.79 / 4.81  k 4.91 / 4.93  v 2.61 / 2.81  out 4.66 / 4.47
  closed     output 4.32  dx 4.57           q 4.80 / 4.81  k 4.91 / 4.93  v 2.55 / 2.80  out 4.66 / 4.48
  D = 256 block, rank 16 (printed): output 5.21, dx 5.39, factors 3.5 - 6.5
  tiny ID step: forward 1.22 (gate 1.5), the 32 factor gradients 3.1 - 4.8 (gate 5 x + 1e-3), either backward form
"""
import functools

import pytest
import torch

from tests.backward_refs import rnd_bf16
from tests.golden.cases import TINY_BRANCH_CFG, tiny_inputs
from tests.test_fp8_training_gpu import FP8_BLOCK_MUL, MODEL_ADD, SMALL_CFG, _block_weights, _case, rel

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
F64 = torch.float64
TARGETS = ("to_q", "to_k", "to_v", "to_out.0")
GRIDS = {"small": (3, 8, 12), "full": (3, 16, 24)}
LORA_SCALE = 2.0   # lora_alpha / r
FP8_MODEL_MUL = 1.5  # fp8_model_gate (tests/test_model_gpu.py)
KEEPS = {"all": (True, True), "attention": (False, True), "recompute": (False, False)}


# ------------------------------------------------------------------------------------------------------------------
# cases, blocks, oracles (computed once per session, never modified)
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _small(B):
    g = torch.Generator().manual_seed(40 + B)
    T, nv = 6, 288
    x = torch.randn(B, T + nv, 256, generator=g)
    temb = torch.randn(B, 32, generator=g)
    dout = torch.randn(x.shape, generator=g)
    return dict(weights=_block_weights(256, 32), x=x.bfloat16(), temb=temb.bfloat16(), dout=dout.bfloat16(),
                rope=tiny_inputs()["rope"], T=T, heads=4, temb_dim=32, grid=GRIDS["small"])


def _get(kind, B=2):
    return _small(B) if kind == "small" else dict(_case("full"), grid=GRIDS["full"])


@functools.lru_cache(maxsize=None)
def _factors(D, rank, zero_B=False, seed=11):
    """{(target, "A" | "B"): bf16 values as fp32}: trained-looking factors (PEFT starts B at 0, where dA = 0)."""
    g = torch.Generator().manual_seed(seed + rank)
    out = {}
    for t in TARGETS:
        out[t, "A"] = (torch.randn(rank, D, generator=g) * 0.03).bfloat16().float()
        b = torch.randn(D, rank, generator=g) * 0.03
        out[t, "B"] = (torch.zeros_like(b) if zero_B else b).bfloat16().float()
    return out


def _mask(c, seed=47):
    g = torch.Generator().manual_seed(seed)
    B, N = c["x"].shape[:2]
    m = torch.zeros(B, N, dtype=torch.bool)
    m[:, c["T"]:] = torch.rand(B, N - c["T"], generator=g) < 0.4
    return m


def _block(c, rank=None, resample=False, closed=False, order="attach_first", zero_B=False, fp8=True, loaded=False):
    """loaded: the adapter as load_lora_weights attaches it (frozen factors; either order), else add_adapter's
    trainable one (before the fp8 QKV projection is enabled)."""
    from videopainter_amd import device_scope
    from videopainter_amd.lora import add_trainable_adapter_, attach_lora_
    from videopainter_amd.transformer import CogVideoXBlock
    D = c["x"].shape[-1]
    with device_scope(dev):
        blk = CogVideoXBlock(dim=D, num_attention_heads=c["heads"], attention_head_dim=64,
                             time_embed_dim=c["temb_dim"], attention_bias=True, id_pool_resample_learnable=resample)
    with torch.no_grad():
        for k, p in blk.state_dict().items():
            p.copy_(torch.from_numpy(c["weights"][k]))
    blk.requires_grad_(False)

    def enable():
        if fp8:
            blk.enable_fp8_ffn()
            blk.enable_fp8_qkv()
            blk.enable_fp8_out()

    def attach():
        if rank is None:
            return
        f = _factors(D, rank, zero_B)
        if loaded:
            attach_lora_(blk, {f"attn1.{t}.lora_{ab}.weight": v for (t, ab), v in f.items()}, LORA_SCALE)
            return
        add_trainable_adapter_(blk, rank, LORA_SCALE * rank, TARGETS)
        with torch.no_grad():
            for t in TARGETS:
                lin = blk.attn1.to_out[0] if t == "to_out.0" else getattr(blk.attn1, t)
                lin.lora_A.weight.copy_(f[t, "A"])
                lin.lora_B.weight.copy_(f[t, "B"])
    for step in ((enable, attach) if order == "enable_first" else (attach, enable)):
        step()
    if closed:
        blk.enable_closed_form_resample_backward()
    return blk


def _rope(c):
    from videopainter_amd.attention_processor import _rope_dev
    return _rope_dev(c["rope"], torch.device(dev), c["grid"])


def _factor_params(blk):
    out = {}
    for t in TARGETS:
        lin = blk.attn1.to_out[0] if t == "to_out.0" else getattr(blk.attn1, t)
        out[t, "A"], out[t, "B"] = lin.lora_A.weight, lin.lora_B.weight
    return out


def _step(blk, c, rm=None):
    """block_apply + backward of the case's cotangent: (out, dx, {factor: grad})."""
    from videopainter_amd.autograd import block_apply
    for p in blk.parameters():
        p.grad = None
    xd = c["x"].to(dev).requires_grad_()
    out = block_apply(blk, xd, c["T"], c["temb"].to(dev), _rope(c), resample_mask=rm)
    out.backward(c["dout"].to(dev))
    grads = {k: p.grad for k, p in _factor_params(blk).items()} if hasattr(blk.attn1.to_q, "lora_A") else {}
    return out.detach(), xd.grad, grads


@functools.lru_cache(maxsize=None)
def _oracle(kind, rank, resample=False):
    """[(out, dx, {factor: grad})] in fp32 and in bf16: the oracle's block with PEFT's unmerged LoRA Linears on the
    bf16 weights and factors, and its autograd."""
    from oracle import cogvideox_oracle as O
    c = _get(kind)
    T, D = c["T"], c["x"].shape[-1]
    cfg = dict(num_attention_heads=c["heads"], norm_eps=1e-5)
    kw = {}
    if resample:
        cfg["id_pool_resample_learnable"] = True
        kw = dict(resample=True)
    res = []
    for dtype in (torch.float32, torch.bfloat16):
        sd = {"b." + k: torch.from_numpy(v).to(BF).to(dtype) for k, v in c["weights"].items()}
        leaves = {}
        for (t, ab), v in _factors(D, rank).items():
            leaves[t, ab] = sd[f"b.attn1.{t}.lora_{ab}.weight"] = v.to(dtype).clone().requires_grad_()
            sd[f"b.attn1.{t}.lora_scaling"] = torch.tensor(LORA_SCALE)
        x = c["x"].to(dtype).clone().requires_grad_()
        if resample:
            kw["resample_mask"] = _mask(c).to(dtype)
        h, e = O.block_forward(sd, "b", cfg, x[:, T:], x[:, :T], c["temb"].to(dtype), c["rope"], **kw)
        out = torch.cat([e, h], 1)
        out.backward(c["dout"].to(dtype))
        res.append((out.detach(), x.grad, {k: l.grad for k, l in leaves.items()}))
    return res


def _gate(name, got, o32, o16, mul=FP8_BLOCK_MUL, add=0.0):
    """Prints r8, r16 and their ratio; returns the failure (or None)."""
    r8, r16 = rel(got.float(), o32), rel(o16.float(), o32)
    print(f"{name:28s} r8 {r8:.3e}  r16 {r16:.3e}  ratio {r8 / max(r16, 1e-30):.2f}")
    return None if r8 <= mul * r16 + add else (name, r8, r16)


# ------------------------------------------------------------------------------------------------------------------
# (a) the dual modulate kernel against the two existing kernels
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [256, 3072])
def test_dual_modulate_equals_both_kernels(D):
    """Both outputs bit for bit, with the text / video boundary inside each batch row, text_len 0 and text_len Ntok;
    74 rows (18 whole blocks of 4 rows and a partial one), and the bf16 rows also at the row stride of a K-augmented
    operand."""
    from videopainter_amd import kernels as K
    B, Ntok = 2, 37
    g = torch.Generator().manual_seed(70 + D)
    x = (torch.randn(B, Ntok, D, generator=g) * 1.5 + 0.3).bfloat16().to(dev)
    lw = (1 + 0.2 * torch.randn(D, generator=g)).bfloat16().to(dev)
    lb = (0.1 * torch.randn(D, generator=g)).bfloat16().to(dev)
    mod = (0.5 * torch.randn(B, 6 * D, generator=g)).bfloat16().to(dev)
    for T in (0, 7, Ntok):
        for pad in (0, 192):
            y16 = K.adaln_modulate(x, lw, lb, mod, T, 1e-5)
            q = K.adaln_modulate_mx(x, lw, lb, mod, T, 1e-5, out=K.MXTensor(B * Ntok, D, x.device))
            buf = torch.full((B * Ntok, D + pad), 7.0, device=dev, dtype=BF)
            y, m = K.adaln_modulate_dual(x, lw, lb, mod, T, 1e-5, out=buf[:, :D].view(B, Ntok, D),
                                         out_mx=K.MXTensor(B * Ntok, D, x.device))
            assert torch.equal(y, y16), (T, pad)
            assert torch.equal(m.q, q.q) and torch.equal(m.scales, q.scales), (T, pad)
            assert bool((buf[:, D:] == 7.0).all())  # nothing written past the rows' D columns
    if D == 256:  # the text rows use the enc_* chunks: T matters
        assert not torch.equal(K.adaln_modulate(x, lw, lb, mod, 0, 1e-5), K.adaln_modulate(x, lw, lb, mod, 7, 1e-5))


# ------------------------------------------------------------------------------------------------------------------
# (b) lora_B = 0: the fp8 block with adapters equals the fp8 block without
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("resample", [False, True], ids=["standard", "resample"])
def test_zero_B_is_the_block_without_adapters(monkeypatch, B, resample):
    """PEFT's init (every lora_B = 0): inference and the training forward at each keep level are torch.equal to the
    fp8 block without adapters (the side path adds rnd(0) onto the base and the residual): a trainable adapter, and
    a loaded one for both orders of enabling fp8 and attaching, rank 16."""
    from videopainter_amd import autograd as AG
    from videopainter_amd.autograd import block_apply
    c = _small(B)
    rm = _mask(c).to(dev).to(torch.uint8) if resample else None
    args = (c["x"].to(dev), c["T"], c["temb"].to(dev), _rope(c))
    with torch.no_grad():
        want = _block(c, resample=resample).forward_joint(*args, resample_mask=rm)
    monkeypatch.setattr(AG, "_room_for", lambda *a, **k: True)
    # a trainable adapter (attached before fp8 is enabled), and a loaded one in both orders
    for order, loaded in (("attach_first", False), ("attach_first", True), ("enable_first", True)):
        for closed in ((False, True) if resample else (False,)):
            blk = _block(c, 16, resample, closed, order, zero_B=True, loaded=loaded)
            with torch.no_grad():
                assert torch.equal(blk.forward_joint(*args, resample_mask=rm), want), (order, closed)
            for level, (acts, attn) in KEEPS.items():
                monkeypatch.setattr(AG, "SAVE_ACTIVATIONS", acts)
                monkeypatch.setattr(AG, "SAVE_ATTENTION", attn)
                out = block_apply(blk, args[0].clone().requires_grad_(), *args[1:], resample_mask=rm)
                assert out.requires_grad and torch.equal(out.detach(), want), (order, closed, level)


# ------------------------------------------------------------------------------------------------------------------
# (c) exact operands: the side path's rounding chain per element
# ------------------------------------------------------------------------------------------------------------------

def _sparse_int(g, rows, cols, per_row, lo, hi):
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:per_row]
        w[r, idx] = torch.randint(lo, hi + 1, (per_row,), generator=g).float()
    return w


def exact_case(rank, B=2, seed=90):
    """Operands of the exact test (CPU, fp32 holding bf16-exact values): x rows of +-0.5 in equal numbers, the
    attention output o in {-1.5 .. 1.5} steps of 1/2, integer weights / biases / factors (s = 1), gates from a few
    dyadic values; `exact_refs` asserts what the construction promises."""
    g = torch.Generator().manual_seed(seed + rank)
    D, T, N = 256, 6, 6 + 288
    half = torch.cat([torch.full((D // 2,), 0.5), torch.full((D // 2,), -0.5)])
    x = torch.stack([torch.stack([half[torch.randperm(D, generator=g)] for _ in range(N)]) for _ in range(B)])
    o = torch.randint(-3, 4, (B, N, D), generator=g).float() * 0.5
    gates = torch.tensor([-1.0, -0.5, 0.25, 0.5, 1.0, 1.5])
    mod = torch.zeros(B, 6 * D)
    for chunk in (2, 5):
        mod[:, chunk * D:(chunk + 1) * D] = gates[torch.randint(0, len(gates), (B, D), generator=g)]
    w = {t: _sparse_int(g, D, D, 12, -3, 3) for t in TARGETS}
    bias = {t: torch.randint(-4, 5, (D,), generator=g).float() for t in TARGETS}
    A = {t: _sparse_int(g, rank, D, 6, -3, 3) for t in TARGETS}
    Bf = {t: _sparse_int(g, D, rank, 3, -2, 2) for t in TARGETS}
    return dict(x=x, o=o, mod=mod, w=w, bias=bias, A=A, B=Bf, T=T, rank=rank)


def exact_refs(e):
    """(qkv_base, delta, x_mid) in float64: the base projection rnd(xn W^T + b), the adapters' T (s B)^T, and
    DESIGN §4's chain for x_mid — every accumulator exact, every rnd() a single rounding of an exactly known value."""
    def exact(t):  # a value the construction promises to be a bf16 number
        assert torch.equal(rnd_bf16(t), t)
        return t
    xn, o, mod = e["x"].double(), e["o"].double(), e["mod"].double()
    Bn, N, D = xn.shape
    qkv_base, delta = [], []
    for t in TARGETS[:3]:
        qkv_base.append(exact(xn @ e["w"][t].double().T + e["bias"][t].double()))
        Tt = exact(xn @ e["A"][t].double().T)
        delta.append(exact(Tt @ e["B"][t].double().T))
    qkv_base, delta = torch.cat(qkv_base, -1), torch.cat(delta, -1)
    exact(qkv_base + delta)
    t = "to_out.0"
    text = (torch.arange(N) < e["T"])[None, :, None]
    gate = torch.where(text, mod[:, None, 5 * D:6 * D], mod[:, None, 2 * D:3 * D])
    To = exact(o @ e["A"][t].double().T)
    r1 = rnd_bf16(xn + rnd_bf16(gate * rnd_bf16(To @ e["B"][t].double().T)))      # R' (the residual is x itself)
    y = rnd_bf16(o @ e["w"][t].double().T + e["bias"][t].double())
    return qkv_base, delta, rnd_bf16(r1 + rnd_bf16(gate * y))


def _exact_block(e, adapters):
    from videopainter_amd import device_scope
    from videopainter_amd.lora import add_trainable_adapter_
    from videopainter_amd.transformer import CogVideoXBlock
    with device_scope(dev):
        blk = CogVideoXBlock(dim=256, num_attention_heads=4, attention_head_dim=64, time_embed_dim=32,
                             attention_bias=True, norm_eps=0.75)
    blk.requires_grad_(False)
    a = blk.attn1
    with torch.no_grad():
        blk.norm1.norm.weight.fill_(1.0)
        blk.norm1.norm.bias.zero_()
        for t in TARGETS:
            lin = a.to_out[0] if t == "to_out.0" else getattr(a, t)
            lin.weight.copy_(e["w"][t])
            lin.bias.copy_(e["bias"][t])
    if adapters:
        add_trainable_adapter_(blk, e["rank"], float(e["rank"]), TARGETS)  # alpha = r: s = 1
        with torch.no_grad():
            for t in TARGETS:
                lin = a.to_out[0] if t == "to_out.0" else getattr(a, t)
                lin.lora_A.weight.copy_(e["A"][t])
                lin.lora_B.weight.copy_(e["B"][t])
    blk.enable_fp8_qkv()
    blk.enable_fp8_out()
    return blk


@pytest.mark.parametrize("rank", [16, 64])
def test_side_path_on_exact_operands(rank):
    """The attention-input and attention-output stages of an fp8 block on exactly representable operands:
    qkv_with - qkv_without == T (s B)^T in float64, exactly (and qkv_without is the exact base projection); x_mid_with
    equals the chain R' = rnd(R + rnd(gate rnd(acc_lora))), x_mid = rnd(R' + rnd(gate rnd(acc_base + bias))) per
    element, and without adapters the same chain with R' = R.  The delta is added in place on the base qkv."""
    e = exact_case(rank)
    qkv_base, delta, x_mid = exact_refs(e)
    assert float(delta.abs().max()) > 0 and float((delta != 0).double().mean()) > 0.2
    x, o, mod = (e[k].bfloat16().to(dev) for k in ("x", "o", "mod"))
    with torch.no_grad():
        res = {}
        for adapters in (False, True):
            blk = _exact_block(e, adapters)
            xn, qkv, _ = blk._attn_input(x, e["T"], mod)
            assert (xn is not None) == adapters
            if adapters:
                assert torch.equal(xn.double().cpu(), e["x"].double())
            res[adapters] = (qkv.double().cpu(), blk._attn_output(x, o, mod, e["T"]).double().cpu())
    assert torch.equal(res[False][0], qkv_base)
    assert torch.equal(res[True][0] - res[False][0], delta)
    assert torch.equal(res[True][1], x_mid)
    assert not torch.equal(res[False][1], x_mid)


# ------------------------------------------------------------------------------------------------------------------
# (d) gradients across the keep levels
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,rank", [(2, 16), (1, 64)])
def test_keep_levels_give_the_same_gradients(monkeypatch, B, rank):
    """SAVE_ACTIVATIONS / SAVE_ATTENTION at (True, True), (False, True), (False, False): the same output, dx and LoRA
    factor gradient bits (non-zero B), and every factor receives a non-zero gradient while no base parameter gets
    one."""
    from videopainter_amd import autograd as AG
    monkeypatch.setattr(AG, "_room_for", lambda *a, **k: True)
    c = _small(B)
    blk = _block(c, rank)
    res = []
    for acts, attn in KEEPS.values():
        monkeypatch.setattr(AG, "SAVE_ACTIVATIONS", acts)
        monkeypatch.setattr(AG, "SAVE_ATTENTION", attn)
        res.append(_step(blk, c))
    o0, dx0, g0 = res[-1]
    assert len(g0) == 8 and all(g is not None and float(g.float().abs().max()) > 0 for g in g0.values())
    lora = {id(p) for p in _factor_params(blk).values()}
    assert all(p.grad is None for p in blk.parameters() if id(p) not in lora)
    for o1, dx1, g1 in res[:-1]:
        assert torch.equal(o1, o0) and torch.equal(dx1, dx0)
        for k in g0:
            assert torch.equal(g1[k], g0[k]), k


def test_refusals_still_raised():
    """NotImplementedError for a trainable base weight, bias or norm on an fp8 block with adapters, a wanted temb
    gradient, and the fp8 attention in training."""
    from videopainter_amd.autograd import block_apply
    c = _small(2)
    x, temb, rope = c["x"].to(dev).requires_grad_(), c["temb"].to(dev), _rope(c)
    blk = _block(c, 16)
    for name in ("attn1.to_k.weight", "attn1.to_out.0.bias", "norm1.norm.weight", "attn1.norm_k.weight"):
        p = dict(blk.named_parameters())[name]
        p.requires_grad_(True)
        with pytest.raises(NotImplementedError, match="trains no parameter"):
            block_apply(blk, x, c["T"], temb, rope)
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="time-embedding"):
        block_apply(blk, x, c["T"], temb.clone().requires_grad_(), rope)
    blk.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="fp8 modes"):
        block_apply(blk, x, c["T"], temb, rope)


# ------------------------------------------------------------------------------------------------------------------
# accuracy against the oracle's PEFT-unmerged twin
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["standard", "explicit", "closed"])
def test_full_width_block_against_the_oracle(form):
    """The full-width block with rank-64 adapters on all four projections (non-zero B) on the fp8 GEMMs: the block
    output, dx and every LoRA factor gradient within 5 x the oracle's own bf16 drift of the same quantity, for the
    standard processor and the resample processor in both backward forms."""
    resample = form != "standard"
    c = _get("full")
    blk = _block(c, 64, resample, form == "closed")
    rm = _mask(c).to(dev).to(torch.uint8) if resample else None
    out, dx, grads = _step(blk, c, rm)
    (o32, dx32, g32), (o16, dx16, g16) = _oracle("full", 64, resample)
    bad = [_gate(f"{form} output", out, o32, o16), _gate(f"{form} dx", dx, dx32, dx16)]
    for (t, ab), g in grads.items():
        bad.append(_gate(f"{form} d{ab} {t}", g, g32[t, ab], g16[t, ab]))
    assert not [b for b in bad if b], [b for b in bad if b]


def test_small_block_figures_rank_16():
    """The D = 256 block (rank 16, B = 2), whose own fp8 forward without adapters is outside the band: the
    figures are printed, and the gradients must be finite and non-zero."""
    c = _small(2)
    out, dx, grads = _step(_block(c, 16), c)
    (o32, dx32, g32), (o16, dx16, g16) = _oracle("small", 16)
    _gate("small output", out, o32, o16)
    _gate("small dx", dx, dx32, dx16)
    for (t, ab), g in grads.items():
        _gate(f"small d{ab} {t}", g, g32[t, ab], g16[t, ab])
        assert bool(torch.isfinite(g.float()).all()) and float(g.float().abs().max()) > 0


@pytest.mark.parametrize("closed", [False, True], ids=["explicit", "closed"])
def test_tiny_id_training_step(closed):
    """VideoPainterID's training step on a 4-layer resample transformer at D = 256 with enable_fp8(attention=False)
    and rank-16 adapters on every block: the forward within 1.5 x the oracle's bf16 drift (the whole-model fp8 gate),
    every LoRA factor gradient within 5 x + 1e-3 of it, against the oracle with PEFT's unmerged Linears."""
    from oracle import cogvideox_oracle as O
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd.config import full_config, state_dict_shapes
    from videopainter_amd.weights import synth_state_dict
    cfg = dict(SMALL_CFG, id_pool_resample_learnable=True)
    bcfg = dict(SMALL_CFG, num_layers=TINY_BRANCH_CFG["num_layers"])
    tsd = synth_state_dict(state_dict_shapes(full_config(SMALL_CFG)), 0)
    bsd = synth_state_dict({("B." + k): v for k, v in state_dict_shapes(full_config(bcfg, True), True).items()}, 0)
    bsd = {k[2:]: v for k, v in bsd.items()}
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**cfg)
        br = CogvideoXBranchModel(**bcfg)
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    br.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()})
    br.requires_grad_(False)
    tr.add_adapter({"r": 16, "lora_alpha": 32, "target_modules": list(TARGETS)})
    tr.enable_fp8(attention=False)
    if closed:
        tr.enable_closed_form_resample_backward()
    assert all(b.ff_mx is not None and b.qkv_mx is not None and b.out_mx is not None for b in tr.transformer_blocks)
    g = torch.Generator().manual_seed(7)
    facs = {}
    with torch.no_grad():
        for n, p in tr.named_parameters():
            if p.requires_grad:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
                facs[n] = p.detach().float().cpu()
    assert len(facs) == 8 * SMALL_CFG["num_layers"]
    i = tiny_inputs()
    R = torch.randn(i["video"].shape, generator=g).bfloat16()
    with torch.no_grad():
        samples = br(hidden_states=i["video"].to(dev).bfloat16(), encoder_hidden_states=i["enc"].to(dev).bfloat16(),
                     branch_cond=i["branch_cond"].to(dev).bfloat16(), timestep=i["timestep"].to(dev),
                     image_rotary_emb=i["rope"], return_dict=False)[0]
    out = tr(hidden_states=i["hidden"].to(dev).bfloat16(), encoder_hidden_states=i["enc"].to(dev).bfloat16(),
             timestep=i["timestep"].to(dev), image_rotary_emb=i["rope"], branch_block_samples=samples,
             branch_block_masks=i["mask"].to(dev), id_pool_resample_learnable=True, return_dict=False)[0]
    out.backward(R.to(dev))
    ours = {n: p.grad for n, p in tr.named_parameters() if n in facs}
    assert all(p.grad is None for n, p in tr.named_parameters() if n not in facs)

    def oracle(dtype):
        tp = {k: torch.from_numpy(v).to(dtype) for k, v in tsd.items()}
        leaves = {n: v.to(dtype).clone().requires_grad_() for n, v in facs.items()}
        for n, l in leaves.items():
            tp[n] = l
            tp[n.rsplit(".lora_", 1)[0] + ".lora_scaling"] = torch.tensor(2.0)
        bp = {k: torch.from_numpy(v).to(dtype) for k, v in bsd.items()}
        with torch.no_grad():
            s = O.branch_forward(bp, full_config(bcfg, True), i["video"].to(dtype), i["enc"].to(dtype),
                                 i["branch_cond"].to(dtype), i["timestep"], i["rope"])
        o = O.transformer_forward(tp, dict(full_config(SMALL_CFG), id_pool_resample_learnable=True),
                                  i["hidden"].to(dtype), i["enc"].to(dtype), i["timestep"], i["rope"],
                                  branch_block_samples=s, branch_block_masks=i["mask"].to(dtype),
                                  id_pool_resample_learnable=True)[0]
        o.backward(R.to(dtype))
        return o.detach(), {n: l.grad for n, l in leaves.items()}

    o32, g32 = oracle(torch.float32)
    o16, g16 = oracle(torch.bfloat16)
    bad = [_gate("model output", out.detach(), o32, o16, FP8_MODEL_MUL)]
    for n in facs:
        assert ours[n] is not None, n
        bad.append(_gate(n.replace("transformer_blocks.", "").replace(".weight", ""), ours[n], g32[n], g16[n],
                         FP8_BLOCK_MUL, MODEL_ADD))
    assert not [b for b in bad if b], [b for b in bad if b]
