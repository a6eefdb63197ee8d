"""FusedProdigy and FusedAdam on the GPU (videopainter_amd/optim.py, csrc/prodigy.hip, csrc/optim.hip).

prodigyopt is not a dependency, so parity is pinned to a restatement of prodigyopt 1.0's step() (slice_p = 1, no FSDP)
in torch ops on CPU copies, once in float64 (the truth) and once in float32 (what a correct fp32 implementation loses).

Parameter sets: test_optim_gpu.py's — bf16 tensors of shapes [1], [7], [3072], [CHUNK+1], [64, 3072], [3, 5, 7] plus
one parameter whose .grad is None, and 300 tensors of 33 elements.  Weights N(0, 0.02^2).  Gradients are correlated
across the 12 steps, grad[t] = bf16((base + 0.5 noise_t) 1e-3): with independent gradients <g, p0 - p> stays near zero,
d never leaves d0 and nothing of the d update would be tested."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16
STEPS = 12
D0 = 1e-6
HYP = dict(betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)
SCHEDULE = [1.0, 0.8, 1.2, 0.5, 0.9]
PRODIGY_KEYS = ("master", "exp_avg", "exp_avg_sq", "s", "p0")


def _shapes(kind):
    from videopainter_amd.optim import CHUNK
    if kind == "many":
        return [(33,)] * 300
    return [(1,), (7,), (3072,), (CHUNK + 1,), (64, 3072), (3, 5, 7)]


_DATA = {}


def data(kind):
    """(weights, grads[step][i]) on the CPU in bf16, generated once per parameter set and never modified."""
    if kind not in _DATA:
        g = torch.Generator().manual_seed(40 if kind == "main" else 41)
        shapes = _shapes(kind)
        w = [(torch.randn(s, generator=g) * 0.02).to(BF16) for s in shapes]
        base = [torch.randn(s, generator=g) for s in shapes]
        gr = [[((b + 0.5 * torch.randn(s, generator=g)) * 1e-3).to(BF16) for b, s in zip(base, shapes)]
              for _ in range(STEPS)]
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


def restatement(kind, dtype, steps=STEPS, lrs=(1.0,), betas=HYP["betas"], beta3=None, eps=HYP["eps"],
                weight_decay=HYP["weight_decay"], decouple=True, use_bias_correction=False, safeguard_warmup=False,
                d0=D0, d_coef=1.0, growth_rate=float("inf"), max_norm=None, group_decay=None):
    """The spec of FusedProdigy.step() in torch ops on `dtype` CPU copies, in the spec's order; d and its companions in
    Python floats as in prodigyopt.  group_decay: (index of the first tensor of the second group, its weight decay).
    Returns (master - initial over all tensors, d)."""
    w, gr = data(kind)
    p = [t.to(dtype) for t in w]
    p0 = [t.clone() for t in p]
    m, v, s = ([torch.zeros_like(t) for t in p] for _ in range(3))
    wds = [weight_decay if group_decay is None or i < group_decay[0] else group_decay[1] for i in range(len(p))]
    beta1, beta2 = betas
    beta3 = math.sqrt(beta2) if beta3 is None else beta3
    d = d_max = d0
    num, k = 0.0, 0
    for t in range(steps):
        lr = lrs[t % len(lrs)]
        grads = [x.to(dtype) for x in gr[t]]
        clip = 1.0
        if max_norm is not None:
            norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(x) for x in grads])))
            clip = min(1.0, max_norm / (norm + 1e-6))
        bc = math.sqrt(1 - beta2 ** (k + 1)) / (1 - beta1 ** (k + 1)) if use_bias_correction else 1.0
        dlr = d * lr * bc
        num *= beta3
        den = dot = 0.0
        for i, x in enumerate(grads):
            g = x * clip
            if wds[i] != 0 and not decouple:
                g = g.add(p[i], alpha=wds[i])
            dot += torch.dot(g.flatten(), (p0[i] - p[i]).flatten()).item()
            m[i].mul_(beta1).add_(g, alpha=d * (1 - beta1))
            v[i].mul_(beta2).addcmul_(g, g, value=d * d * (1 - beta2))
            s[i].mul_(beta3).add_(g, alpha=(d / d0) * (d if safeguard_warmup else dlr))
            den += s[i].abs().sum().item()
        num += (d / d0) * dlr * dot
        if den == 0:
            continue
        if lr > 0:
            d_hat = d_coef * num / den
            if d == d0:
                d = max(d, d_hat)
            d_max = max(d_max, d_hat)
            d = min(d_max, d * growth_rate)
        for i in range(len(p)):
            denom = v[i].sqrt().add_(d * eps)
            if wds[i] != 0 and decouple:
                p[i].add_(p[i], alpha=-wds[i] * dlr)
            p[i].addcdiv_(m[i], denom, value=-dlr)
        k += 1
    return torch.cat([(a.double() - b.double()).reshape(-1) for a, b in zip(p, w)]), d


_REF = {}


def reference(case):
    """(delta64, d64, delta32, d32) of a parity case, computed once."""
    if case not in _REF:
        c = dict(CASES[case])
        kind = c.pop("kind")
        _REF[case] = restatement(kind, torch.float64, **c) + restatement(kind, torch.float32, **c)
    return _REF[case]


def run_fused(kind, steps=range(STEPS), lrs=(1.0,), group_decay=None, opt=None, ps=None, after_step=None,
              persistent=True, **kw):
    """Run FusedProdigy over `steps` of the set's gradients; returns (opt, ps, idle)."""
    from videopainter_amd import FusedProdigy
    idle = None
    if opt is None:
        ps, idle, allp = make_params(kind)
        if group_decay is None:
            pg = [dict(params=allp)]
        else:  # (the idle parameter sits at index 2 of the list)
            k = group_decay[0] + 1 if group_decay[0] >= 2 else group_decay[0]
            pg = [dict(params=allp[:k]), dict(params=allp[k:], weight_decay=group_decay[1])]
        opt = FusedProdigy(pg, **dict(dict(HYP, lr=lrs[0], d0=D0), **kw))
    for s in steps:
        for grp in opt.param_groups:
            grp["lr"] = lrs[s % len(lrs)]
        set_grads(ps, kind, s, persistent)
        opt.step()
        if after_step is not None:
            after_step(opt, ps, idle, s)
    return opt, ps, idle


def fused_delta(opt, ps, kind):
    w, _ = data(kind)
    return torch.cat([(opt.state[p]["master"].double().cpu() - t.double()).reshape(-1) for p, t in zip(ps, w)])


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def snapshot(opt, ps):
    return [t.clone() for p in ps for t in (p.detach(), *(opt.state[p][k] for k in PRODIGY_KEYS))] + [
        opt.d_block.clone(), opt.step_count.clone()]


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------
# parity with the float64 restatement
# ------------------------------------------------------------------------------------------------------------------

CASES = {
    "default": dict(kind="main"),
    "clip_active": dict(kind="main", max_norm=0.1),  # the gradient norm is ~0.5: the coefficient is ~0.2
    "coupled_decay": dict(kind="main", decouple=False),
    "bias_correction": dict(kind="main", use_bias_correction=True),
    "safeguard": dict(kind="main", safeguard_warmup=True, use_bias_correction=True),
    "growth_rate": dict(kind="main", growth_rate=1.5),
    "two_groups": dict(kind="main", group_decay=(3, 1e-2)),
    "lr_schedule": dict(kind="main", lrs=SCHEDULE),
    "many": dict(kind="many"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_prodigy_parity(case):
    """D = master after 12 steps - initial.  Gates, in test_optim_gpu.py::test_update_parity's form:
    rel-L2(D_fused, D_fp64) <= 2 x rel-L2(D_fp32, D_fp64), and |d_fused - d_fp64| / d_fp64 <= 2 x the same of the fp32
    restatement: the fp32 loss is the rounding of each master add and of p0 - p, which any correct fp32 implementation
    shares; 2x is room for operation order and the order of the two sums.  (DESIGN.md §5 records the figures.)"""
    c = dict(CASES[case])
    kind, max_norm = c.pop("kind"), c.pop("max_norm", None)
    d64, dd64, d32, dd32 = reference(case)
    assert dd64 >= 5 * D0, "the case's own inputs must move d, or the d update is not tested"
    opt, ps, _ = run_fused(kind, max_grad_norm=max_norm, **c)
    df, d = fused_delta(opt, ps, kind), float(opt.d)
    r_fused, r_ref = rel(df, d64), rel(d32, d64)
    e_fused, e_ref = abs(d - dd64) / dd64, abs(dd32 - dd64) / dd64
    print(f"prodigy[{case}] delta: fused {r_fused:.3e} fp32 {r_ref:.3e}   d: {d:.6e} (fp64 {dd64:.6e}) "
          f"fused {e_fused:.3e} fp32 {e_ref:.3e}")
    assert torch.isfinite(df).all() and float(d64.norm()) > 0
    assert r_fused <= 2.0 * r_ref
    assert e_fused <= 2.0 * e_ref
    assert int(opt.step_count) == STEPS and int(opt.last_step_skipped) == 0 and int(opt.no_progress) == 0
    assert float(opt.d_max) >= d and float(opt.d_denom) > 0
    if case == "growth_rate":  # the clamp acts: another d than the default case's
        assert reference("default")[1] != dd64


def test_growth_rate_limits_d_once_it_left_d0():
    """The step that leaves d0 takes d_hat whole (d = max(d, d_hat) while d == d0, as in prodigyopt); every later step
    may at most multiply d by growth_rate, and with these inputs at least one does exactly that."""
    seen = []
    run_fused("main", growth_rate=1.5, after_step=lambda opt, ps, idle, s: seen.append(opt.d.clone()))
    ds = [float(x) for x in seen]
    assert ds[0] == D0 and ds[-1] > 5 * D0
    later = [(a, b) for a, b in zip(ds, ds[1:]) if a > D0]
    assert later and all(b <= a * 1.5 for a, b in later)
    assert any(b == a * 1.5 for a, b in later)


# (max_norm, weight_decay): test_optim_gpu.py's PARITY["script"] and ["clip_active"], and one with a decay large
# enough that the L2 term is a visible part of the gradient
ADAM_CASES = {"script": (1.0, 1e-4), "clip_active": (0.1, 1e-4), "strong_decay": (1.0, 0.1)}


@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_adam_parity(case):
    """FusedAdam against torch.optim.Adam (the decay as an L2 term) in float64 and float32 on test_optim_gpu.py's
    data and settings, 5 steps: rel-L2(D_fused, D_fp64) <= 2 x rel-L2(D_torch_fp32, D_fp64).  At the script's decay
    of 1e-4 the L2 term is 2e-6 beside gradients of 1e-3; the third case has a decay of 0.1, where the same gate also
    tells Adam from AdamW (FusedAdamW on the same inputs must miss it)."""
    from tests import test_optim_gpu as T
    from videopainter_amd import FusedAdam, FusedAdamW
    max_norm, wd = ADAM_CASES[case]
    w, gr = T.data("main")

    def torch_adam(dtype):
        ps = [torch.nn.Parameter(t.to(dtype)) for t in w]
        opt = torch.optim.Adam(ps, lr=T.LRS[0], betas=T.HYP["betas"], eps=T.HYP["eps"], weight_decay=wd)
        for s in range(T.STEPS):
            opt.param_groups[0]["lr"] = T.LRS[s]
            for p, g in zip(ps, gr[s]):
                p.grad = g.to(dtype)
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
        return torch.cat([(p.detach().double() - t.double()).reshape(-1) for p, t in zip(ps, w)])

    def fused(cls):
        ps, idle, allp = T.make_params("main")
        opt = cls(allp, lr=T.LRS[0], betas=T.HYP["betas"], eps=T.HYP["eps"], weight_decay=wd, max_grad_norm=max_norm)
        for s in range(T.STEPS):
            opt.param_groups[0]["lr"] = T.LRS[s]
            T.set_grads(ps, "main", s)
            opt.step()
        for p in ps:
            assert torch.equal(p.detach(), opt.state[p]["master"].to(BF16))
        assert int(opt.step_count) == T.STEPS and torch.equal(idle.detach(), torch.full_like(idle, 0.25))
        return T.fused_delta(opt, ps, "main")

    d64, d32 = torch_adam(torch.float64), torch_adam(torch.float32)
    df, dw = fused(FusedAdam), fused(FusedAdamW)
    r_fused, r_torch, r_adamw = T.rel(df, d64), T.rel(d32, d64), T.rel(dw, d64)
    print(f"adam[{case}] fused {r_fused:.3e}  torch-fp32 {r_torch:.3e}  (FusedAdamW against Adam: {r_adamw:.3e})")
    assert torch.isfinite(df).all() and float(d64.norm()) > 0
    assert r_fused <= 2.0 * r_torch
    if case == "strong_decay":  # the decoupled decay is another update: the gate tells the two apart
        assert r_adamw > 2.0 * r_torch


# ------------------------------------------------------------------------------------------------------------------
# behaviour (bit-exact)
# ------------------------------------------------------------------------------------------------------------------

def test_bf16_write_back_and_idle_parameter():
    seen = []

    def check(opt, ps, idle, s):
        for p in ps:
            assert torch.equal(p.detach(), opt.state[p]["master"].to(BF16)), (s, tuple(p.shape))
        seen.append(s)

    opt, ps, idle = run_fused("main", max_grad_norm=1.0, after_step=check)
    assert seen == list(range(STEPS))
    w, gr = data("main")
    assert any(not torch.equal(p.detach().cpu(), t) for p, t in zip(ps, w))  # (bf16 values did move)
    st = opt.state[idle]
    assert idle.grad is None and torch.equal(idle.detach(), torch.full((5,), 0.25, device=dev, dtype=BF16))
    assert torch.equal(st["master"], torch.full((5,), 0.25, device=dev)) and torch.equal(st["p0"], st["master"])
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and not st["s"].any()
    for p, t in zip(ps, w):  # p0 is the initial master, never written
        assert torch.equal(opt.state[p]["p0"].cpu(), t.float())
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(ps, gr[STEPS - 1]))  # gradients are left unscaled


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
    """Parameters / gradients that are slices at odd element offsets run the scalar head / whole-chunk scalar path of
    both passes: the same per-element arithmetic, bit-identical parameters and state after two steps (with
    zero_grads: the zero fill has a phase of its own), and nothing outside the views written.  The two sums take
    their elements in another order on another path, so d_numerator and d_denom may differ in their last bits; the
    two steps stay at d == d0 (asserted), where neither reaches a parameter."""
    from videopainter_amd import FusedProdigy
    from videopainter_amd.optim import CHUNK
    g = torch.Generator().manual_seed(6)
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
            opt = FusedProdigy([p], **HYP, d0=D0, zero_grads=True)
            for _ in range(2):
                p.grad.copy_(gr)
                opt.step()
                assert not p.grad.any()
            assert float(opt.d) == D0 and int(opt.step_count) == 2
            # nothing outside the views was written
            assert not pbuf[:po].any() and not pbuf[po + n:].any() and not gbuf.any()
            res.append([p.detach().clone()] + [opt.state[p][k].clone() for k in PRODIGY_KEYS])
        assert all(same(r, res[0]) for r in res[1:]), n
        assert not torch.equal(res[0][1], w.float()) and res[0][4].any()


def test_reallocated_gradients():
    kept, kps, _ = run_fused("main", steps=range(8), max_grad_norm=1.0)
    opt, ps, _ = run_fused("main", steps=range(4), max_grad_norm=1.0)
    old = [p.grad for p in ps]
    for s in range(4, 8):
        for p in ps:
            p.grad = None
        set_grads(ps, "main", s, persistent=False)
        assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(ps, old))
        old += [p.grad for p in ps]
        opt.step()
    assert float(opt.d) > D0 and same(snapshot(opt, ps), snapshot(kept, kps))
    # and a step where another subset has gradients (the tables are rebuilt)
    ps[0].grad = None
    before = snapshot(opt, ps[:1])[:-2]
    opt.step()
    assert same(snapshot(opt, ps[:1])[:-2], before)


def test_skip_on_nonfinite_gradient():
    ref, rps, _ = run_fused("main", steps=range(8), max_grad_norm=1.0, skip_nonfinite=True)
    opt, ps, idle = run_fused("main", steps=range(6), max_grad_norm=1.0, skip_nonfinite=True)
    assert float(opt.d) > D0  # (the skipped step meets a d block that has moved)
    before = snapshot(opt, ps + [idle])
    set_grads(ps, "main", 9)
    ps[4].grad.view(-1)[12345] = float("inf")
    opt.step()
    assert same(snapshot(opt, ps + [idle]), before)  # parameters, the five buffers, the d block, the counter
    assert int(opt.step_count) == 6 and int(opt.last_step_skipped) == 1 and int(opt.nonfinite) == 1
    run_fused("main", steps=[6, 7], opt=opt, ps=ps)
    assert int(opt.step_count) == 8 and int(opt.last_step_skipped) == 0 and int(opt.nonfinite) == 0
    assert same(snapshot(opt, ps), snapshot(ref, rps))


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_all_zero_gradients_make_no_progress(weight_decay):
    from videopainter_amd import FusedProdigy
    ps, idle, allp = make_params("main")
    opt = FusedProdigy(allp, **dict(HYP, weight_decay=weight_decay), d0=D0)
    before = [p.detach().clone() for p in allp] + [opt.state[p]["master"].clone() for p in allp]
    for _ in range(2):
        for p in ps:
            p.grad = torch.zeros_like(p)
        opt.step()
        assert int(opt.no_progress) == 1 and int(opt.step_count) == 0 and int(opt.last_step_skipped) == 0
    assert float(opt.d) == D0 and float(opt.d_max) == D0 and float(opt.d_numerator) == 0.0
    assert same([p.detach() for p in allp] + [opt.state[p]["master"] for p in allp], before)
    run_fused("main", steps=range(1), opt=opt, ps=ps)  # and a real gradient moves it on
    assert int(opt.no_progress) == 0 and int(opt.step_count) == 1
    assert not torch.equal(opt.state[ps[4]]["master"], before[len(allp) + 5])


def test_determinism_and_resume():
    from videopainter_amd import FusedProdigy
    kw = dict(max_grad_norm=1.0, use_bias_correction=True, growth_rate=3.0)
    a, aps, _ = run_fused("main", **kw)
    b, bps, _ = run_fused("main", **kw)
    assert same(snapshot(a, aps), snapshot(b, bps))
    c, cps, cidle = run_fused("main", steps=range(7), **kw)
    sd = c.state_dict()
    assert sd["step"] == 7 and sd["prodigy"]["d"] == float(c.d) > D0 and set(sd["state"][0]) == set(PRODIGY_KEYS)
    clones = [torch.nn.Parameter(p.detach().clone()) for p in cps]
    idle2 = torch.nn.Parameter(cidle.detach().clone())
    d = FusedProdigy(clones[:2] + [idle2] + clones[2:], lr=0.5, betas=(0.5, 0.5), d0=1e-3, max_grad_norm=1.0)
    d.load_state_dict(sd)
    assert d.param_groups[0]["betas"] == HYP["betas"] and d.d0 == D0 and d.use_bias_correction
    assert int(d.step_count) == 7 and torch.equal(d.d_block, c.d_block)
    sd["state"][0]["master"].zero_()  # the state dict holds clones
    assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(clones, cps))  # bf16 parameters are left alone
    run_fused("main", steps=range(7, STEPS), opt=d, ps=clones)
    assert same(snapshot(d, clones), snapshot(a, aps))
    e = FusedProdigy([torch.nn.Parameter(torch.zeros(3, device=dev, dtype=BF16))])
    with pytest.raises(ValueError):
        e.load_state_dict(sd)


def test_lr_scheduler_drives_the_kernel_lr():
    from videopainter_amd import FusedProdigy
    ps, _, allp = make_params("main")
    opt = FusedProdigy(allp, lr=1.0, **HYP, d0=D0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: SCHEDULE[s % len(SCHEDULE)])
    for s in range(STEPS):
        set_grads(ps, "main", s)
        opt.step()
        sched.step()
    ref, rps, _ = run_fused("main", lrs=SCHEDULE)
    assert same(snapshot(opt, ps), snapshot(ref, rps))
    plain, pps, _ = run_fused("main")
    assert not torch.equal(plain.d, opt.d)


def test_group_options_are_checked_every_step():
    opt, ps, _ = run_fused("main", steps=range(1), group_decay=(3, 1e-2))
    opt.param_groups[1]["lr"] = 0.5
    set_grads(ps, "main", 1)
    before = snapshot(opt, ps)
    with pytest.raises(ValueError, match="same in every parameter group"):
        opt.step()
    assert same(snapshot(opt, ps), before)


def test_no_host_synchronisation():
    opt, ps, idle = run_fused("main", steps=range(1), max_grad_norm=1.0, skip_nonfinite=True, zero_grads=True)
    fresh = [g.to(dev) for g in data("main")[1][1]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        for p, g in zip(ps, fresh):
            p.grad = g
        opt.step()
        states = (opt.d, opt.d_max, opt.d_hat, opt.d_numerator, opt.d_denom, opt.dlr, opt.no_progress, opt.d_block,
                  opt.grad_norm, opt.clip_coef, opt.last_step_skipped, opt.step_count)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in states)
    assert all(t.dtype == torch.float64 for t in states[:6]) and states[6].dtype == torch.int32
