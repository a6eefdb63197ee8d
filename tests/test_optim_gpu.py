"""Training tail on the GPU (videopainter_amd/optim.py, training.py, csrc/optim.hip): gradient norm, clip, AdamW with
fp32 master weights, the fused v-prediction loss, and the whole step on the tiny model.

Parameter set: bf16 tensors of shapes [1], [7], [3072], [CHUNK+1], [64, 3072], [3, 5, 7] (scalar head / tail, the
exact-chunk boundary, several chunks) plus one parameter whose .grad is None; a second set of 300 tensors of 33
elements.  Weights N(0, 0.02^2), gradients N(0, 1e-3^2) in bf16, the training script's hyper-parameters
(train/VideoPainter.sh), 5 steps with a different lr each."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16
HYP = dict(betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)
LRS = [1e-5, 8e-6, 1.2e-5, 5e-6, 9e-6]
STEPS = 5


def _shapes(kind):
    from videopainter_amd.optim import CHUNK
    if kind == "many":
        return [(33,)] * 300
    return [(1,), (7,), (3072,), (CHUNK + 1,), (64, 3072), (3, 5, 7)]


_DATA = {}


def data(kind):
    """(weights, grads[step][i]) on the CPU in bf16, generated once per parameter set and never modified."""
    if kind not in _DATA:
        g = torch.Generator().manual_seed(20 if kind == "main" else 21)
        shapes = _shapes(kind)
        w = [(torch.randn(s, generator=g) * 0.02).to(BF16) for s in shapes]
        gr = [[(torch.randn(s, generator=g) * 1e-3).to(BF16) for s in shapes] for _ in range(STEPS)]
        _DATA[kind] = (w, gr)
    return _DATA[kind]


def make_params(kind):
    """The set's parameters on the device, plus (at index 2) one parameter that never gets a gradient."""
    w, _ = data(kind)
    ps = [torch.nn.Parameter(t.to(dev)) for t in w]
    idle = torch.nn.Parameter(torch.full((5,), 0.25, device=dev, dtype=BF16))
    return ps, idle, ps[:2] + [idle] + ps[2:]


def set_grads(ps, kind, step, persistent=True):
    _, gr = data(kind)
    for p, g in zip(ps, gr[step]):
        if persistent and p.grad is not None:
            p.grad.copy_(g)
        else:
            p.grad = g.to(dev).clone()


def run_fused(kind, steps=range(STEPS), groups=None, lr_scale=(1.0,), opt=None, ps=None, after_step=None, **kw):
    """Run FusedAdamW over `steps` of the set's gradients; returns (opt, ps, idle)."""
    from videopainter_amd import FusedAdamW
    idle = None
    if opt is None:
        ps, idle, allp = make_params(kind)
        if groups is None:
            pg = [dict(params=allp)]
        else:  # two groups: the first `groups` parameters, and the rest
            pg = [dict(params=allp[:groups]), dict(params=allp[groups:])]
        opt = FusedAdamW(pg, lr=LRS[0], **HYP, **kw)
    for s in steps:
        for grp, sc in zip(opt.param_groups, lr_scale):
            grp["lr"] = LRS[s] * sc
        set_grads(ps, kind, s)
        opt.step()
        if after_step is not None:
            after_step(opt, ps, idle, s)
    return opt, ps, idle


def torch_ref(kind, dtype, max_norm, weight_decay=HYP["weight_decay"], groups=None, lr_scale=(1.0,)):
    """torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ on `dtype` copies (CPU); returns master - initial."""
    w, gr = data(kind)
    ps = [torch.nn.Parameter(t.to(dtype)) for t in w]
    if groups is None:
        pg = [dict(params=ps)]
    else:  # (the idle parameter sits at index 2 of the fused run's list)
        k = groups - 1 if groups > 2 else groups
        pg = [dict(params=ps[:k]), dict(params=ps[k:])]
    opt = torch.optim.AdamW(pg, lr=LRS[0], betas=HYP["betas"], eps=HYP["eps"], weight_decay=weight_decay)
    for s in range(STEPS):
        for grp, sc in zip(opt.param_groups, lr_scale):
            grp["lr"] = LRS[s] * sc
        for p, g in zip(ps, gr[s]):
            p.grad = g.to(dtype)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    return torch.cat([(p.detach().double() - t.double()).reshape(-1) for p, t in zip(ps, w)])


def fused_delta(opt, ps, kind):
    w, _ = data(kind)
    return torch.cat([(opt.state[p]["master"].double().cpu() - t.double()).reshape(-1) for p, t in zip(ps, w)])


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def snapshot(opt, ps):
    return [t.clone() for p in ps for t in (p.detach(), opt.state[p]["master"], opt.state[p]["exp_avg"],
                                            opt.state[p]["exp_avg_sq"])]


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------
# 1, 2: norm and clip
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["main", "many"])
def test_gradient_norm(kind):
    """rel. error against the float64 norm of the same bf16 grads <= 1e-5 (n non-negative fp32 terms in a fixed-order
    tree: <= log2(n) 2^-24 ~ 2e-6 for n <= 1e9); two calls agree bit for bit."""
    from videopainter_amd import get_gradient_norm
    _, idle, allp = make_params(kind)
    set_grads([p for p in allp if p is not idle], kind, 0)
    want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in data(kind)[1][0]))
    a = get_gradient_norm(allp)
    b = get_gradient_norm(allp)
    assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 0
    err = abs(float(a) - want) / want
    print(f"norm[{kind}] {float(a):.9g} vs float64 {want:.9g}: rel {err:.2e}")
    assert err <= 1e-5
    assert torch.equal(a, b)
    assert idle.grad is None


@pytest.mark.parametrize("kind", ["main", "many"])
def test_clip_grad_norm(kind):
    from videopainter_amd import clip_grad_norm_
    _, idle, allp = make_params(kind)
    ps = [p for p in allp if p is not idle]
    set_grads(ps, kind, 1)
    before = [p.grad.clone() for p in ps]
    want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in before))
    # max_norm above the norm: the gradients are untouched
    ptrs = [p.grad.data_ptr() for p in ps]
    n_hi = clip_grad_norm_(allp, 10.0 * want)
    assert abs(float(n_hi) - want) / want <= 1e-5
    assert all(torch.equal(p.grad, b) for p, b in zip(ps, before))
    # below: g <- bf16(g * coef), coef in fp32 from the kernel's own norm
    max_norm = 0.25 * want
    n_lo = clip_grad_norm_(allp, max_norm)
    assert torch.equal(n_lo, n_hi)
    coef = torch.clamp(max_norm / (n_lo + 1e-6), max=1.0)
    assert coef.dtype == torch.float32 and 0.24 < float(coef) < 0.26
    for p, b in zip(ps, before):
        assert torch.equal(p.grad, (b.float() * coef).to(BF16))
    assert [p.grad.data_ptr() for p in ps] == ptrs and idle.grad is None


# ------------------------------------------------------------------------------------------------------------------
# 3: update parity with torch.optim.AdamW in float64 / float32
# ------------------------------------------------------------------------------------------------------------------

PARITY = {
    "script": dict(kind="main", max_norm=1.0),
    "no_clip": dict(kind="main", max_norm=None),
    "clip_active": dict(kind="main", max_norm=0.1),  # the gradient norm is ~0.47: the coefficient is ~0.21
    "no_decay": dict(kind="main", max_norm=1.0, weight_decay=0.0),
    "two_groups": dict(kind="main", max_norm=1.0, groups=4, lr_scale=(1.0, 0.3)),
    "many_tensors": dict(kind="many", max_norm=1.0),
}


@pytest.mark.parametrize("case", list(PARITY))
def test_update_parity(case):
    """D = master after 5 steps - initial.  Gate: rel-L2(D_fused, D_fp64) <= 2 x rel-L2(D_torch_fp32, D_fp64) over
    all tensors: the fp32 drift is the rounding of each master add, which any correct fp32 implementation shares; 2x
    is room for operation order and fused multiply-adds.  (DESIGN.md §5 records the figures.)"""
    c = dict(PARITY[case])
    kind, max_norm = c.pop("kind"), c.pop("max_norm")
    wd = c.pop("weight_decay", HYP["weight_decay"])
    d64 = torch_ref(kind, torch.float64, max_norm, wd, **c)
    d32 = torch_ref(kind, torch.float32, max_norm, wd, **c)
    hyp = dict(HYP, weight_decay=wd)
    from videopainter_amd import FusedAdamW
    ps, idle, allp = make_params(kind)
    g = c.get("groups")
    pg = [dict(params=allp)] if g is None else [dict(params=allp[:g]), dict(params=allp[g:])]
    opt = FusedAdamW(pg, lr=LRS[0], **hyp, max_grad_norm=max_norm)
    opt, ps, _ = run_fused(kind, opt=opt, ps=ps, lr_scale=c.get("lr_scale", (1.0,)))
    df = fused_delta(opt, ps, kind)
    r_fused, r_torch = rel(df, d64), rel(d32, d64)
    print(f"parity[{case}] fused {r_fused:.3e}  torch-fp32 {r_torch:.3e}")
    assert torch.isfinite(df).all() and float(d64.norm()) > 0
    assert r_fused <= 2.0 * r_torch
    if max_norm is not None:  # the pre-clip norm and the coefficient of the last step, on the device
        gn = math.sqrt(sum(float(x.double().pow(2).sum()) for x in data(kind)[1][STEPS - 1]))
        assert abs(float(opt.grad_norm) - gn) / gn <= 1e-5
        assert abs(float(opt.clip_coef) - min(1.0, max_norm / (gn + 1e-6))) <= 1e-5
    assert int(opt.step_count) == STEPS and int(opt.last_step_skipped) == 0


# ------------------------------------------------------------------------------------------------------------------
# 4: the bf16 write-back, the untouched parameter, zero_grads
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["main", "many"])
def test_bf16_write_back_and_idle_parameter(kind):
    seen = []

    def check(opt, ps, idle, s):
        for p in ps:
            assert torch.equal(p.detach(), opt.state[p]["master"].to(BF16)), (s, tuple(p.shape))
        seen.append(s)

    opt, ps, idle = run_fused(kind, max_grad_norm=1.0, after_step=check)
    assert seen == list(range(STEPS))
    w, _ = data(kind)
    assert any(not torch.equal(p.detach().cpu(), t) for p, t in zip(ps, w))  # (bf16 values did move)
    st = opt.state[idle]
    assert idle.grad is None and torch.equal(idle.detach(), torch.full((5,), 0.25, device=dev, dtype=BF16))
    assert torch.equal(st["master"], torch.full((5,), 0.25, device=dev))
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    for p in ps:  # the gradients are left as they were (the clip is folded into the update)
        assert p.grad is not None
    _, gr = data(kind)
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(ps, gr[STEPS - 1]))


def test_zero_grads_in_the_update_pass():
    ptrs = {}

    def check(opt, ps, idle, s):
        for p in ps:
            assert not p.grad.any(), (s, tuple(p.shape))
            assert ptrs.setdefault(p, p.grad.data_ptr()) == p.grad.data_ptr()

    opt, ps, _ = run_fused("main", max_grad_norm=1.0, zero_grads=True, after_step=check)
    ref, rps, _ = run_fused("main", max_grad_norm=1.0)
    assert same(snapshot(opt, ps), snapshot(ref, rps))


def test_unaligned_views_take_the_scalar_paths():
    """Parameters / gradients that are slices at odd element offsets (no common 16-byte phase, or a shared non-zero
    one) run the scalar head / whole-chunk scalar path: the same per-element arithmetic, bit-identical results.
    Offsets (4, 4) share a phase the fp32 state can follow (a head of 4 elements, then the vector body, then a tail);
    3 elements give the norm and the clip a head of 5; sizes below 8, 9 and CHUNK + 1 give pieces of fewer elements
    than one vector, a vector with a one-element tail, and a second chunk of one element."""
    from videopainter_amd import FusedAdamW, clip_grad_norm_, get_gradient_norm
    from videopainter_amd.optim import CHUNK
    g = torch.Generator().manual_seed(5)
    for n in (CHUNK + 37, CHUNK + 1, 9, 7, 1):
        w = (torch.randn(n, generator=g) * 0.02).to(BF16).to(dev)
        gr = (torch.randn(n, generator=g) * 1e-3).to(BF16).to(dev)
        res = []
        for po, go in ((0, 0), (3, 3), (3, 5), (1, 0), (4, 4)):
            pbuf = torch.zeros(n + 16, device=dev, dtype=BF16)
            gbuf = torch.zeros(n + 16, device=dev, dtype=BF16)
            p = torch.nn.Parameter(pbuf[po:po + n])
            p.data.copy_(w)
            p.grad = gbuf[go:go + n]
            p.grad.copy_(gr)
            opt = FusedAdamW([p], lr=1e-5, **HYP)
            opt.step()
            nrm = get_gradient_norm([p])
            clip_grad_norm_([p], 0.01)
            coef = torch.clamp(0.01 / (nrm + 1e-6), max=1.0)
            assert torch.equal(p.grad, (gr.float() * coef).to(BF16))
            want = float(gr.double().norm())
            assert abs(float(nrm) - want) / want <= 1e-5
            # nothing outside the views was written
            assert not pbuf[:po].any() and not pbuf[po + n:].any() and not gbuf[:go].any() and not gbuf[go + n:].any()
            res.append([p.detach().clone(), opt.state[p]["master"].clone(), opt.state[p]["exp_avg"].clone(),
                        opt.state[p]["exp_avg_sq"].clone()])
        assert all(same(r, res[0]) for r in res[1:]), n
        assert not torch.equal(res[0][1], w.float())


# ------------------------------------------------------------------------------------------------------------------
# 5, 6, 7: what a training loop does to an optimizer
# ------------------------------------------------------------------------------------------------------------------

def test_reallocated_gradients():
    """Step 1 with persistent .grad tensors, step 2 after p.grad = None and fresh tensors (other addresses: the old
    ones are kept alive): bit-identical to a run that kept the tensors."""
    kept, kps, _ = run_fused("main", steps=range(2), max_grad_norm=1.0)
    opt, ps, _ = run_fused("main", steps=range(1), max_grad_norm=1.0)
    old = [p.grad for p in ps]
    for p in ps:
        p.grad = None
    for grp in opt.param_groups:
        grp["lr"] = LRS[1]
    set_grads(ps, "main", 1, persistent=False)
    assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(ps, old))
    opt.step()
    assert same(snapshot(opt, ps), snapshot(kept, kps))
    # and a step where another subset has gradients (the tables are rebuilt)
    ps[0].grad = None
    before = snapshot(opt, ps[:1])
    opt.step()
    assert same(snapshot(opt, ps[:1]), before)
    assert not same(snapshot(opt, ps[1:]), snapshot(kept, kps[1:]))


def test_skip_on_nonfinite_gradient():
    """A value check only: one +inf among the gradients, skip_nonfinite=True."""
    ref, rps, _ = run_fused("main", steps=range(3), max_grad_norm=1.0, skip_nonfinite=True)
    opt, ps, idle = run_fused("main", steps=range(2), max_grad_norm=1.0, skip_nonfinite=True)
    before = snapshot(opt, ps + [idle])
    assert int(opt.step_count) == 2 and int(opt.last_step_skipped) == 0
    set_grads(ps, "main", 4)
    ps[4].grad.view(-1)[12345] = float("inf")
    opt.step()
    assert same(snapshot(opt, ps + [idle]), before)
    assert int(opt.step_count) == 2 and int(opt.last_step_skipped) == 1 and int(opt.nonfinite) == 1
    run_fused("main", steps=[2], opt=opt, ps=ps)
    assert int(opt.step_count) == 3 and int(opt.last_step_skipped) == 0 and int(opt.nonfinite) == 0
    assert same(snapshot(opt, ps), snapshot(ref, rps))
    # without skip_nonfinite the step is taken (torch's behaviour): the counter moves
    plain, pps, _ = run_fused("main", steps=range(1))
    set_grads(pps, "main", 1)
    pps[0].grad.fill_(float("nan"))
    plain.step()
    assert int(plain.step_count) == 2 and int(plain.nonfinite) == 1 and int(plain.last_step_skipped) == 0


def test_determinism_and_resume():
    from videopainter_amd import FusedAdamW
    a, aps, _ = run_fused("main", max_grad_norm=1.0)
    b, bps, _ = run_fused("main", max_grad_norm=1.0)
    assert same(snapshot(a, aps), snapshot(b, bps))
    c, cps, cidle = run_fused("main", steps=range(3), max_grad_norm=1.0)
    sd = c.state_dict()
    assert sd["step"] == 3
    clones = [torch.nn.Parameter(p.detach().clone()) for p in cps]
    idle2 = torch.nn.Parameter(cidle.detach().clone())
    d = FusedAdamW(clones[:2] + [idle2] + clones[2:], lr=0.5, betas=(0.5, 0.5), max_grad_norm=1.0)
    d.load_state_dict(sd)
    assert d.param_groups[0]["betas"] == HYP["betas"] and d.param_groups[0]["eps"] == HYP["eps"]
    assert int(d.step_count) == 3
    sd["state"][0]["master"].zero_()  # the state dict holds clones: changing it changes neither optimizer
    run_fused("main", steps=[3, 4], opt=d, ps=clones)
    assert same(snapshot(d, clones), snapshot(a, aps))
    e = FusedAdamW([torch.nn.Parameter(torch.zeros(3, device=dev, dtype=BF16))])
    with pytest.raises(ValueError):
        e.load_state_dict(sd)


def test_lr_scheduler_drives_the_kernel_lr():
    from videopainter_amd import FusedAdamW
    ps, _, allp = make_params("main")
    opt = FusedAdamW(allp, lr=1.0, **HYP, max_grad_norm=1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: LRS[min(s, STEPS - 1)])
    for s in range(STEPS):
        set_grads(ps, "main", s)
        opt.step()
        sched.step()
    ref, rps, _ = run_fused("main", max_grad_norm=1.0)
    assert same(snapshot(opt, ps), snapshot(ref, rps))


def test_no_host_synchronisation():
    """step() (with persistent and with freshly allocated gradients: the table upload), the functional norm / clip
    and the loss forward + backward run with torch's synchronisation check set to raise on any synchronising call."""
    from videopainter_amd import clip_grad_norm_, get_gradient_norm, inpainting_v_loss
    opt, ps, idle = run_fused("main", steps=range(1), max_grad_norm=1.0, skip_nonfinite=True, zero_grads=True)
    fresh = [p.grad.clone() for p in ps]
    shape = (2, 3, 16, 6, 10)
    out, noisy, target = (torch.randn(shape, device=dev).to(BF16) for _ in range(3))
    out.requires_grad_()
    mask = torch.ones(2, 3, 1, 6, 10, device=dev, dtype=BF16)
    ts, ac = torch.tensor([3, 996], device=dev), _alphas().to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        for p, g in zip(ps, fresh):
            p.grad = g
        opt.step()
        norm = get_gradient_norm(ps + [idle])
        total = clip_grad_norm_(ps + [idle], 1e-3)
        inpainting_v_loss(out, noisy, target, ts, ac, mask, 1.0).backward()
        states = (opt.grad_norm, opt.clip_coef, opt.last_step_skipped, opt.step_count)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in states + (norm, total)) and int(opt.step_count) == 3
    assert out.grad is not None and torch.isfinite(out.grad.float()).all()


# ------------------------------------------------------------------------------------------------------------------
# 8: the loss
# ------------------------------------------------------------------------------------------------------------------

GATE_MUL = 1.25  # the project's gate() form (tests/test_model_gpu.py)


def _alphas():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, 0).float()


def script_loss(model_output, noisy, target, timesteps, ac, masks, lam, table_dtype):
    """train_cogvideox_inpainting_i2v_video.py:1879-1891 with scheduler.get_velocity (alphas cast to the sample
    dtype, then the square roots); `ac` is the script's fp32 table (:1731), cast to table_dtype for the weights."""
    B = model_output.shape[0]
    a = ac.to(model_output.dtype)[timesteps]
    sa, sb = a ** 0.5, (1 - a) ** 0.5
    while sa.dim() < model_output.dim():
        sa, sb = sa.unsqueeze(-1), sb.unsqueeze(-1)
    model_pred = sa * noisy - sb * model_output
    weights = 1 / (1 - ac.to(table_dtype)[timesteps])
    while weights.dim() < model_pred.dim():
        weights = weights.unsqueeze(-1)
    loss = torch.mean((weights * (model_pred - target) ** 2).reshape(B, -1), dim=1).mean()
    if masks is not None:
        inp = torch.mean((weights * (model_pred * masks - target * masks) ** 2).reshape(B, -1), dim=1).mean()
        loss = loss + lam * inp
    return loss


@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("mask", ["bf16", "fp32", None])
@pytest.mark.parametrize("shape,ts", [((2, 3, 16, 6, 10), (3, 996)), ((1, 2, 3, 5, 7), (500,))],
                         ids=["2x3x16x6x10", "1x2x3x5x7"])
def test_loss_and_gradient(shape, ts, mask, lam):
    from videopainter_amd import inpainting_v_loss
    B, F, Cc, H, W = shape
    g = torch.Generator().manual_seed(31)
    out, noisy, target = (torch.randn(shape, generator=g).to(BF16) for _ in range(3))
    m = (torch.rand(B, F, 1, H, W, generator=g) > 0.4).float()
    m[:, 0] = 0.5  # a value whose square differs from itself
    ac = _alphas()
    t = torch.tensor(ts, dtype=torch.int64)

    def ref(dtype, table_dtype):
        o = out.to(dtype).clone().requires_grad_()
        mm = None if mask is None else m.to(dtype)
        loss = script_loss(o, noisy.to(dtype), target.to(dtype), t, ac, mm, lam, table_dtype)
        loss.backward()
        return loss.detach(), o.grad

    l64, g64 = ref(torch.float64, torch.float64)
    l16, g16 = ref(BF16, torch.float32)
    md = None if mask is None else m.to(dev, BF16 if mask == "bf16" else torch.float32)
    od = out.to(dev).requires_grad_()
    args = (noisy.to(dev), target.to(dev), t.to(dev), ac.to(dev), md, lam)
    loss = inpainting_v_loss(od, *args)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    loss.backward()
    assert od.grad.dtype == BF16
    e_l, e16_l = abs(float(loss.detach()) - float(l64)) / float(l64), abs(float(l16) - float(l64)) / float(l64)
    e_g, e16_g = rel(od.grad.cpu(), g64), rel(g16, g64)
    print(f"loss {float(loss.detach()):.8g} truth {float(l64):.8g}: rel {e_l:.2e} (bf16 expression {e16_l:.2e}); "
          f"grad rel-L2 {e_g:.2e} (bf16 expression {e16_g:.2e})")
    assert e_l <= GATE_MUL * e16_l + 1e-6
    assert e_g <= GATE_MUL * e16_g + 1e-3
    od2 = out.to(dev).requires_grad_()
    loss2 = inpainting_v_loss(od2, *args)
    (loss2 * 2.0).backward()  # the incoming scalar multiplies the saved gradient
    assert torch.equal(loss, loss2)
    assert torch.equal(od2.grad, (od.grad.float() * 2.0).to(BF16))


# ------------------------------------------------------------------------------------------------------------------
# 9: end to end on the tiny config
# ------------------------------------------------------------------------------------------------------------------

def test_training_step_end_to_end():
    """branch -> transformer -> inpainting_v_loss -> .backward() -> FusedAdamW.step() on the tiny models: the
    gradient that enters the head's backward is the loss kernel's, the parameter gradients equal those of
    out.backward(that gradient), every trained master moves and stays finite."""
    from tests.golden.cases import TINY_CFG, TINY_BRANCH_CFG, tiny_inputs, tiny_weights
    from videopainter_amd import (CogVideoXTransformer3DModel, CogvideoXBranchModel, FusedAdamW, device_scope,
                                  inpainting_v_loss, kernels as K)
    tsd, bsd = tiny_weights()
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**TINY_CFG)
        br = CogvideoXBranchModel(**TINY_BRANCH_CFG)
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    br.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()})
    br.requires_grad_(True)
    i = tiny_inputs()
    b16 = lambda x: x.to(dev, BF16)  # noqa: E731
    g = torch.Generator().manual_seed(8)
    target = b16(torch.randn(i["video"].shape, generator=g))
    ac, ts, mask = _alphas().to(dev), i["timestep"].to(dev), b16(i["mask"])

    def forward():
        samples = br(hidden_states=b16(i["video"]), encoder_hidden_states=b16(i["enc"]),
                     branch_cond=b16(i["branch_cond"]), timestep=ts, image_rotary_emb=i["rope"],
                     return_dict=False)[0]
        return tr(hidden_states=b16(i["hidden"]), encoder_hidden_states=b16(i["enc"]), timestep=ts,
                  image_rotary_emb=i["rope"], branch_block_samples=samples, branch_block_masks=mask,
                  return_dict=False)[0]

    out = forward()
    entered = []
    out.register_hook(lambda gr: entered.append(gr.clone()))
    loss = inpainting_v_loss(out, b16(i["video"]), target, ts, ac, mask, 1.0)
    loss.backward()
    _, d = K.v_loss(out.detach(), b16(i["video"]), target, ts, ac, mask, 1.0)
    assert len(entered) == 1 and torch.equal(entered[0], d)
    named = [(n, p) for n, p in br.named_parameters()]
    got = {n: p.grad.clone() for n, p in named if p.grad is not None}
    assert got and all(torch.isfinite(v.float()).all() for v in got.values())
    for _, p in named:
        p.grad = None
    forward().backward(d)
    for n, p in named:
        assert (p.grad is not None) == (n in got), n
        if p.grad is None:
            continue
        if ".norm_q." in n or ".norm_k." in n:
            # these affine gradients are summed with fp32 atomics across workgroups (tests/test_training_gpu.py):
            # run-to-run noise in the backward itself, so the same band as there instead of bit equality
            assert rel(p.grad.float(), got[n].float()) < 1e-5, n
        else:
            assert torch.equal(p.grad, got[n]), n
    trained = [p for n, p in named if n in got]
    opt = FusedAdamW([p for _, p in named], lr=1e-5, **HYP, max_grad_norm=1.0)
    start = [opt.state[p]["master"].clone() for p in trained]
    opt.step()
    assert torch.isfinite(loss) and torch.isfinite(opt.grad_norm) and int(opt.nonfinite) == 0
    for p, s0 in zip(trained, start):
        m = opt.state[p]["master"]
        assert torch.isfinite(m).all() and not torch.equal(m, s0)
        assert torch.equal(p.detach(), m.to(BF16))
