"""ShardedFusedProdigy and ShardedFusedAdam on the GPU (videopainter_amd/zero.py, csrc/zero.hip): the ranks are threads
of one process that talk through distributed.LocalComm, each with its own copies of the parameters on the one device.

Parameter sets (tests/test_zero_gpu.py's): "main" — bf16 tensors of shapes [1], [7], [3072], [CHUNK+1], [64, 3072],
[3, 5, 7] plus one parameter whose .grad is None (index 2 of the optimizer's list); "small" — [1], [7] alone, so that
at world 4 two ranks own only padding.  Weights bf16(0.02 randn).  Prodigy needs gradients that are correlated over
the steps, or <g, p0 - p> stays near zero and d never leaves d0: grad[t][r] = bf16((base + 0.5 noise_{t,r}) 1e-3), 12
steps, up to 4 ranks, seed 40, drawn in the order weights, base, then for each step, for each rank, for each shape.

prodigyopt is not a dependency: the reference is tests/test_prodigy_gpu.py's restatement of prodigyopt 1.0's step()
(slice_p = 1, no FSDP) in torch ops on CPU copies, stepped on the mean of the ranks' gradients taken in the
reference's own dtype, once in float64 (the truth) and once in float32 (what a correct fp32 implementation loses).
Every reference and every FusedProdigy / FusedAdam / world-1 run is computed once per configuration and shared."""
import math
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16
STEPS = 12
MAX_WORLD = 4
D0 = 1e-6
HYP = dict(betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)
SCHEDULE = [1.0, 0.8, 1.2, 0.5, 0.9]
ADAM_LR = 1e-5
PRODIGY_KEYS = ("master", "exp_avg", "exp_avg_sq", "s", "p0")
ADAM_KEYS = ("master", "exp_avg", "exp_avg_sq")


def _shapes(kind):
    from videopainter_amd.optim import CHUNK
    if kind == "small":
        return [(1,), (7,)]
    return [(1,), (7,), (3072,), (CHUNK + 1,), (64, 3072), (3, 5, 7)]


_DATA = {}


def data(kind):
    """(weights[i], grads[step][rank][i]) on the CPU in bf16, generated once per set and never modified."""
    if kind not in _DATA:
        g = torch.Generator().manual_seed(40)
        shapes = _shapes(kind)
        w = [(torch.randn(s, generator=g) * 0.02).to(BF16) for s in shapes]
        base = [torch.randn(s, generator=g) for s in shapes]
        gr = [[[((b + 0.5 * torch.randn(s, generator=g)) * 1e-3).to(BF16) for b, s in zip(base, shapes)]
               for _ in range(MAX_WORLD)] for _ in range(STEPS)]
        _DATA[kind] = (w, gr)
    return _DATA[kind]


def mean_grads(kind, step, world, dtype):
    """The mean over the ranks of step `step`'s gradients, taken in `dtype` (world 0: rank 0's gradients alone — what
    every rank holds in a same-gradients run)."""
    _, gr = data(kind)
    if world == 0:
        return [x.to(dtype) for x in gr[step][0]]
    return [sum(gr[step][r][i].to(dtype) for r in range(world)) / world for i in range(len(gr[step][0]))]


def make_params(kind, values=None):
    """One rank's copies of the set on the device (from `values` when given: a resumed run); the main set gets (at
    index 2) a parameter that never has a gradient.  Returns (ps, idle or None, the optimizer's list)."""
    w, _ = data(kind)
    ps = [torch.nn.Parameter(t.to(dev).clone()) for t in (w if values is None else values)]
    if kind == "small":
        return ps, None, list(ps)
    idle = torch.nn.Parameter(torch.full((5,), 0.25, device=dev, dtype=BF16))
    return ps, idle, ps[:2] + [idle] + ps[2:]


def set_grads(ps, kind, step, rank, mode="persistent"):
    """persistent: copy into the .grad tensors there are; fresh: new tensors (the caller set p.grad = None);
    unaligned: new views at odd element offsets of larger buffers (pack's scalar head and whole-chunk scalar paths)."""
    _, gr = data(kind)
    for i, (p, g) in enumerate(zip(ps, gr[step][rank])):
        if mode == "persistent" and p.grad is not None:
            p.grad.copy_(g)
        elif mode == "unaligned":
            off = (3, 5, 1, 4, 7, 2)[i % 6]
            buf = torch.zeros(g.numel() + 16, device=dev, dtype=BF16)
            p.grad = buf[off:off + g.numel()].view(g.shape)
            p.grad.copy_(g)
        else:
            p.grad = g.to(dev).clone()


def _param_groups(allp, split, decay):
    """One group, or two cut at index `split` of the optimizer's list (the second with weight decay `decay`)."""
    if split is None:
        return [dict(params=allp)]
    second = dict(params=allp[split:]) if decay is None else dict(params=allp[split:], weight_decay=decay)
    return [dict(params=allp[:split]), second]


def _cls(name):
    import videopainter_amd
    return getattr(videopainter_amd, name)


class Run:
    """`world` instances of a sharded optimizer (`cls`: its name in the package) over one LocalComm."""

    def __init__(self, cls, kind, world, split=None, decay=None, values=None, **kw):
        from videopainter_amd.distributed import LocalComm
        self.cls, self.kind, self.world, self.comm = cls, kind, world, LocalComm(world)
        self.keys = PRODIGY_KEYS if cls == "ShardedFusedProdigy" else ADAM_KEYS
        self.ps, self.idle, self.opts = [], [], []
        for r in range(world):
            ps, idle, allp = make_params(kind, values)
            self.ps.append(ps)
            self.idle.append(idle)
            self.opts.append(_cls(cls)(_param_groups(allp, split, decay), comm=self.comm, rank=r, **kw))

    def step_all(self):
        self.comm.run(lambda r: self.opts[r].step())

    def run(self, steps=range(STEPS), lrs=None, same_grads=False, after_step=None, mode="persistent"):
        for s in steps:
            for r in range(self.world):
                if lrs is not None:
                    for grp in self.opts[r].param_groups:
                        grp["lr"] = lrs[s % len(lrs)]
                if mode != "persistent":
                    for p in self.ps[r]:
                        p.grad = None
                set_grads(self.ps[r], self.kind, s, 0 if same_grads else r, mode)
            self.step_all()
            if after_step is not None:
                after_step(self, s)
        return self

    def flat(self, name):
        """The state `name` of all ranks assembled in flat order (the padded tail cut off)."""
        return torch.cat([getattr(o, name + "_shard") for o in self.opts])[:self.opts[0].total]

    def snapshot(self):
        """The state buffers in flat order, Prodigy's d block, the step counter, rank 0's bf16 parameters."""
        o = self.opts[0]
        extra = [o.d_block.clone()] if self.cls == "ShardedFusedProdigy" else []
        return [self.flat(k) for k in self.keys] + extra + [o.step_count.clone()] + \
            [p.detach().clone() for p in self.ps[0]]

    def load_all(self, state_dict):
        for o in self.opts:
            o.load_state_dict(state_dict)
        return self

    def full_state_dicts(self):
        return self.comm.run(lambda r: self.opts[r].full_state_dict())


def fused_snapshot(opt, ps, keys):
    """A single-GPU optimizer's state laid out as the sharded optimizer's flat space (every trainable parameter in
    list order, padded with zeros to a multiple of 8 elements), from its public per-parameter state; then as
    Run.snapshot()."""
    allp = [p for g in opt.param_groups for p in g["params"] if p.requires_grad]
    flat = []
    for k in keys:
        parts = []
        for p in allp:
            t = opt.state[p][k].reshape(-1)
            parts += [t, t.new_zeros((-t.numel()) % 8)]
        flat.append(torch.cat(parts))
    extra = [opt.d_block.clone()] if hasattr(opt, "d_block") else []
    return flat + extra + [opt.step_count.clone()] + [p.detach().clone() for p in ps]


def run_fused(cls, kind, steps=range(STEPS), opt=None, ps=None, values=None, after_step=None, **kw):
    """FusedProdigy / FusedAdam on rank 0's gradients (torch-allocated: 16-byte aligned); returns (opt, ps)."""
    if opt is None:
        ps, _, allp = make_params(kind, values)
        opt = _cls(cls)(allp, **kw)
    for s in steps:
        set_grads(ps, kind, s, 0)
        opt.step()
        if after_step is not None:
            after_step(opt, ps, s)
    return opt, ps


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
                                    for x, y in zip(a, b))


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def replicas_agree(run, s=None):
    """bf16 parameters, the whole scalars block and (Prodigy) the whole d block bit-equal on every rank."""
    for r in range(1, run.world):
        assert torch.equal(run.opts[r].scalars, run.opts[0].scalars), (s, r)
        if run.cls == "ShardedFusedProdigy":
            assert torch.equal(run.opts[r].d_block, run.opts[0].d_block), (s, r)
        for p, q in zip(run.ps[r], run.ps[0]):
            assert torch.equal(p.detach(), q.detach()), (s, r, tuple(p.shape))


def sharded_delta(run):
    """master - initial over the set's tensors (padding and the idle parameter left out), assembled from the shards."""
    w, _ = data(run.kind)
    m = run.flat("master").double().cpu()
    off = run.opts[0].flat_offset
    return torch.cat([m[off(p):off(p) + t.numel()] - t.double().reshape(-1) for p, t in zip(run.ps[0], w)])


def bf16_write_back(run):
    """On every rank the parameters are bf16(master), and so is the gathered staging buffer."""
    m16 = run.flat("master").to(BF16)
    for r in range(run.world):
        flat16 = run.opts[r].param_staging[:m16.numel()]
        for p0, p in zip(run.ps[0], run.ps[r]):
            o0 = run.opts[0].flat_offset(p0)
            assert torch.equal(p.detach().reshape(-1), m16[o0:o0 + p.numel()])
            assert torch.equal(flat16[o0:o0 + p.numel()], m16[o0:o0 + p.numel()])


# ------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------

def restatement(kind, world, dtype, steps=STEPS, lrs=(1.0,), betas=HYP["betas"], beta3=None, eps=HYP["eps"],
                weight_decay=HYP["weight_decay"], decouple=True, use_bias_correction=False, safeguard_warmup=False,
                d0=D0, d_coef=1.0, growth_rate=float("inf"), max_norm=None, group_decay=None):
    """tests/test_prodigy_gpu.py's restatement — the spec of FusedProdigy.step() in torch ops on `dtype` CPU copies, in
    the spec's order, d and its companions in Python floats as in prodigyopt — stepped on the mean of the ranks'
    gradients taken in `dtype` (world 0: rank 0's gradients).  group_decay: (index of the first tensor of the second
    group, its weight decay).  Returns (master - initial over all tensors, d, the norm of the last mean gradient)."""
    w, _ = data(kind)
    p = [t.to(dtype) for t in w]
    p0 = [t.clone() for t in p]
    m, v, s = ([torch.zeros_like(t) for t in p] for _ in range(3))
    wds = [weight_decay if group_decay is None or i < group_decay[0] else group_decay[1] for i in range(len(p))]
    beta1, beta2 = betas
    beta3 = math.sqrt(beta2) if beta3 is None else beta3
    d = d_max = d0
    num, k, norm = 0.0, 0, 0.0
    for t in range(steps):
        lr = lrs[t % len(lrs)]
        grads = mean_grads(kind, t, world, dtype)
        norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(x) for x in grads])))
        clip = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
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
    return torch.cat([(a.double() - b.double()).reshape(-1) for a, b in zip(p, w)]), d, norm


CASES = {
    "default": dict(),
    "clip_active": dict(max_norm=0.1),  # the mean gradient's norm is ~0.5: the coefficient is ~0.2
    "coupled_decay": dict(decouple=False),
    "bias_correction": dict(use_bias_correction=True),
    "safeguard": dict(safeguard_warmup=True, use_bias_correction=True),
    "growth_rate": dict(growth_rate=1.5),
    "two_groups": dict(group_decay=(3, 1e-2)),
    "lr_schedule": dict(lrs=SCHEDULE),
}
PARITY = [(2, c) for c in CASES] + [(w, c) for w in (3, 4) for c in ("default", "clip_active")]

_REF = {}


def reference(world, case):
    """(delta64, d64, norm64, delta32, d32, norm32) of a parity case at `world` (0: every rank holds rank 0's
    gradients), computed once."""
    key = ("prodigy", world, case)
    if key not in _REF:
        c = CASES[case]
        _REF[key] = restatement("main", world, torch.float64, **c) + restatement("main", world, torch.float32, **c)
    return _REF[key]


def prodigy_run(world, case, **run_kw):
    """A ShardedFusedProdigy run of a parity case (the reference's options translated to the optimizer's)."""
    c = dict(CASES[case])
    max_norm, lrs, gd = c.pop("max_norm", None), c.pop("lrs", None), c.pop("group_decay", None)
    split, decay = (None, None) if gd is None else (gd[0] + 1, gd[1])  # (the idle parameter sits at list index 2)
    run = Run("ShardedFusedProdigy", "main", world, split=split, decay=decay, lr=1.0, d0=D0, max_grad_norm=max_norm,
              **HYP, **c)
    return run.run(lrs=lrs, **run_kw)


def check_parity(run, world, case):
    """The gates of a parity case on a finished run (the docstring of test_update_parity)."""
    d64, dd64, n64, d32, dd32, _ = reference(world, case)
    assert dd64 >= 5 * D0, "the case's own inputs must move d, or the d update is not tested"
    o = run.opts[0]
    df, d = sharded_delta(run), float(o.d)
    r_sh, r_ref = rel(df, d64), rel(d32, d64)
    e_sh, e_ref = abs(d - dd64) / dd64, abs(dd32 - dd64) / dd64
    e_n = abs(float(o.grad_norm) - n64) / n64
    print(f"parity[world {world}, {case}] delta: sharded {r_sh:.3e} fp32 {r_ref:.3e}   d: {d:.6e} (fp64 {dd64:.6e}, "
          f"{dd64 / D0:.1f} d0) sharded {e_sh:.3e} fp32 {e_ref:.3e}   norm {float(o.grad_norm):.9g} vs fp64 "
          f"{n64:.9g}: rel {e_n:.2e}")
    assert torch.isfinite(df).all() and float(d64.norm()) > 0
    assert r_sh <= 2.0 * r_ref
    assert e_sh <= 2.0 * e_ref
    assert e_n <= 1e-5
    assert int(o.step_count) == STEPS and int(o.last_step_skipped) == 0 and int(o.no_progress) == 0
    assert float(o.d_max) >= d and float(o.d_denom) > 0
    if CASES[case].get("max_norm") is not None:
        assert abs(float(o.clip_coef) - min(1.0, CASES[case]["max_norm"] / (n64 + 1e-6))) <= 1e-5
        assert float(o.clip_coef) < 1.0
    return d


def world1(cls, kind="main"):
    """Snapshot of an uninterrupted world-1 run of a sharded optimizer on rank 0's gradients, no clip (once)."""
    key = ("world1", cls, kind)
    if key not in _REF:
        kw = dict(lr=1.0, d0=D0) if cls == "ShardedFusedProdigy" else dict(lr=ADAM_LR)
        _REF[key] = Run(cls, kind, 1, **kw, **HYP).run(same_grads=True).snapshot()
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------
# 1: world 1 is FusedProdigy / FusedAdam, bit for bit, after every step
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", ["ShardedFusedProdigy", "ShardedFusedAdam"])
def test_world1_is_bit_identical_to_the_single_gpu_optimizer(cls):
    """After each of the 12 steps: the state buffers, the d block, the bf16 parameters and the scalars block.  One
    word of the scalars block cannot be bit-equal: `grad_norm`.  The sharded prologue (the one ShardedFusedAdamW has,
    unchanged) sums squares of the fp32 shard four to a vector, FusedProdigy / FusedAdam sum the bf16 gradients eight
    to a vector — the same terms in another order — so that word gets tests/test_zero_gpu.py's gate for exactly this
    pair of kernels, 1e-5 relative (measured: 1.15e-7 at worst over the 12 steps, both classes), and the other seven
    words (clip_coef, nonfinite, step, both bias corrections, skipped, pad) are compared as bits.  No clip, so the norm
    enters nothing else."""
    fused_cls, keys = ("FusedProdigy", PRODIGY_KEYS) if cls == "ShardedFusedProdigy" else ("FusedAdam", ADAM_KEYS)
    kw = dict(lr=1.0, d0=D0) if cls == "ShardedFusedProdigy" else dict(lr=ADAM_LR)
    seen = []
    run_fused(fused_cls, "main", after_step=lambda o, ps, s: seen.append(
        (fused_snapshot(o, ps, keys), o.scalars.clone())), **kw, **HYP)
    worst = [0.0]

    def check(run, s):
        snap, sc = seen[s]
        o = run.opts[0]
        assert same(run.snapshot(), snap), s
        assert torch.equal(o.scalars[1:], sc[1:]), s
        gn, want = float(o.grad_norm), float(sc.view(torch.float32)[0])
        worst[0] = max(worst[0], abs(gn - want) / want)
        assert abs(gn - want) <= 1e-5 * want, s

    run = Run(cls, "main", 1, **kw, **HYP).run(same_grads=True, after_step=check)
    print(f"world 1 {cls}: grad_norm against {fused_cls}, worst relative difference {worst[0]:.2e}")
    assert len(seen) == STEPS and int(run.opts[0].step_count) == STEPS
    w, _ = data("main")
    assert any(not torch.equal(p.detach().cpu(), t) for p, t in zip(run.ps[0], w))  # (bf16 values did move)
    if cls == "ShardedFusedProdigy":
        assert float(run.opts[0].d) > 5 * D0
    assert same(run.snapshot(), world1(cls))  # run to run


# ------------------------------------------------------------------------------------------------------------------
# 2, 3: update parity with the float64 restatement on the mean gradient; the replicas agree after every step
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,case", PARITY)
def test_update_parity(world, case):
    """D = master after 12 steps - initial, assembled from the shards.  Gates (tests/test_prodigy_gpu.py's and
    tests/test_zero_gpu.py's): rel-L2(D_sharded, D_fp64) <= 2 x rel-L2(D_fp32, D_fp64); |d - d_fp64| / d_fp64 <= 2 x
    the same of the fp32 restatement; the norm of the averaged gradient within 1e-5 of the fp64 one; and the case's
    own fp64 d is at least 5 d0, so the d update is exercised.  After every step the bf16 parameters, the scalars
    block and the d block are bit-equal on all ranks.  (DESIGN.md §5 has the figures.)"""
    run = prodigy_run(world, case, after_step=replicas_agree)
    check_parity(run, world, case)
    bf16_write_back(run)
    if case == "growth_rate":  # the clamp acts: another d than the default case's
        assert reference(world, "default")[1] != reference(world, case)[1]


ADAM_CASES = {"script": (1.0, 1e-4), "clip_active": (0.1, 1e-4), "strong_decay": (1.0, 0.1)}  # (max_norm, decay)


def adam_ref(world, dtype, max_norm, wd):
    """torch.optim.Adam (the decay as an L2 term) + clip_grad_norm_ on `dtype` CPU copies, stepped on the mean of the
    ranks' gradients taken in `dtype`; returns (master - initial, the norm of the last mean gradient)."""
    key = ("adam", world, dtype, max_norm, wd)
    if key not in _REF:
        w, _ = data("main")
        ps = [torch.nn.Parameter(t.to(dtype)) for t in w]
        opt = torch.optim.Adam(ps, lr=ADAM_LR, betas=HYP["betas"], eps=HYP["eps"], weight_decay=wd)
        norm = 0.0
        for s in range(STEPS):
            for p, g in zip(ps, mean_grads("main", s, world, dtype)):
                p.grad = g
            norm = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
        _REF[key] = (torch.cat([(p.detach().double() - t.double()).reshape(-1) for p, t in zip(ps, w)]), norm)
    return _REF[key]


@pytest.mark.parametrize("case", list(ADAM_CASES))
@pytest.mark.parametrize("world", [2, 3, 4])
def test_adam_update_parity(world, case):
    """ShardedFusedAdam against torch.optim.Adam in float64 and float32 on the same data, lr 1e-5: the delta gate and
    the norm gate of test_update_parity.  With a decay of 0.1 the L2 term is a visible part of the gradient, and the
    same gate tells Adam from AdamW (ShardedFusedAdamW on the same inputs must miss it)."""
    max_norm, wd = ADAM_CASES[case]
    d64, n64 = adam_ref(world, torch.float64, max_norm, wd)
    d32, _ = adam_ref(world, torch.float32, max_norm, wd)
    kw = dict(lr=ADAM_LR, betas=HYP["betas"], eps=HYP["eps"], weight_decay=wd, max_grad_norm=max_norm)
    run = Run("ShardedFusedAdam", "main", world, **kw).run(after_step=replicas_agree)
    df, o = sharded_delta(run), run.opts[0]
    r_sh, r_t = rel(df, d64), rel(d32, d64)
    e_n = abs(float(o.grad_norm) - n64) / n64
    print(f"adam[world {world}, {case}] sharded {r_sh:.3e}  torch-fp32 {r_t:.3e}  norm rel {e_n:.2e}")
    assert torch.isfinite(df).all() and float(d64.norm()) > 0
    assert r_sh <= 2.0 * r_t
    assert e_n <= 1e-5
    assert int(o.step_count) == STEPS and (float(o.clip_coef) < 1.0) == (case == "clip_active")
    bf16_write_back(run)
    if case == "strong_decay" and world == 2:  # the decoupled decay is another update: the gate tells the two apart
        dw = sharded_delta(Run("ShardedFusedAdamW", "main", world, **kw).run())
        assert rel(dw, d64) > 2.0 * r_t


def test_replicas_agree_and_idle_parameter_untouched():
    seen = []

    def check(run, s):
        replicas_agree(run, s)
        for r in range(run.world):
            idle, o = run.idle[r], run.opts[r]
            assert idle.grad is None and torch.equal(idle.detach(), torch.full((5,), 0.25, device=dev, dtype=BF16))
            assert len(o.state) == 0  # no per-parameter state grows: the state is the five flat shards
        off = run.opts[0].flat_offset(run.idle[0])
        quarter = torch.tensor([0.25] * 5 + [0.0] * 3, device=dev)
        assert torch.equal(run.flat("master")[off:off + 8], quarter) and torch.equal(run.flat("p0")[off:off + 8], quarter)
        assert not any(run.flat(k)[off:off + 8].any() for k in ("exp_avg", "exp_avg_sq", "s"))
        assert not run.opts[0].grad_staging[off:off + 8].any()  # its gradient region: zeros
        seen.append(s)

    run = Run("ShardedFusedProdigy", "main", 3, lr=1.0, d0=D0, max_grad_norm=1.0, **HYP).run(after_step=check)
    assert seen == list(range(STEPS)) and float(run.opts[0].d) > 5 * D0
    per, total = run.opts[0].per, run.opts[0].total
    for k in PRODIGY_KEYS:  # padding is zero and stays zero
        full = torch.cat([getattr(o, k + "_shard") for o in run.opts])
        assert full.numel() == 3 * per and not full[total:].any()
    w, gr = data("main")
    for p, t in zip(run.ps[0], w):  # p0 is the initial master, never written
        o = run.opts[0].flat_offset(p)
        assert torch.equal(run.flat("p0")[o:o + p.numel()].cpu(), t.float().reshape(-1))
    for r in range(3):  # the gradients are left as they were (the clip is folded into the update)
        assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(run.ps[r], gr[STEPS - 1][r]))


# ------------------------------------------------------------------------------------------------------------------
# 4: sharding invariance with the same gradient on every rank
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 4])
def test_adam_sharding_invariance(world):
    """1 / P and the P-term sum are exact for P = 2, 4 and Adam is element-wise: bit-identical to world 1."""
    run = Run("ShardedFusedAdam", "main", world, lr=ADAM_LR, **HYP).run(same_grads=True, after_step=replicas_agree)
    assert same(run.snapshot(), world1("ShardedFusedAdam"))
    for r in range(world):
        assert same([p.detach() for p in run.ps[r]], world1("ShardedFusedAdam")[len(ADAM_KEYS) + 1:])


@pytest.mark.parametrize("world", [2, 4])
def test_prodigy_sharding_invariance(world):
    """The same gradients on every rank, no clip: every element sees the arithmetic of world 1, but the shard cuts
    re-associate the two sums of the d update, so no bitwise claim is made.  Re-partitioning a sum must cost less than
    doing the whole step in fp32: |d_w - d_1| / d_1 <= the fp32 restatement's own d error on these gradients."""
    _, dd64, _, _, dd32, _ = reference(0, "default")
    e_ref = abs(dd32 - dd64) / dd64
    d1 = float(world1("ShardedFusedProdigy")[len(PRODIGY_KEYS)][0])
    run = Run("ShardedFusedProdigy", "main", world, lr=1.0, d0=D0, **HYP).run(same_grads=True,
                                                                             after_step=replicas_agree)
    dw = float(run.opts[0].d)
    e_w = abs(dw - d1) / d1
    print(f"prodigy sharding invariance, world {world}: d {dw:.9e} against world 1 {d1:.9e}: rel {e_w:.3e}  "
          f"(the fp32 restatement's d error: {e_ref:.3e})")
    assert dd64 >= 5 * D0 and d1 > 5 * D0
    assert e_w <= e_ref


# ------------------------------------------------------------------------------------------------------------------
# 5: ranks that own only padding
# ------------------------------------------------------------------------------------------------------------------

def test_padding_only_ranks():
    """"small" at world 4: per = 8, ranks 0 and 1 own one tensor each, ranks 2 and 3 nothing.  The ranges are world 1's
    and a record is one range's pair, so the d update sums the same two terms in the same slots: equal to world 1 and
    to FusedProdigy bit for bit, d block included."""
    kw = dict(lr=1.0, d0=D0, **HYP)
    run4 = Run("ShardedFusedProdigy", "small", 4, **kw).run(same_grads=True, after_step=replicas_agree)
    assert run4.opts[0].per == 8 and run4.opts[0].total == 16
    assert same(run4.snapshot(), world1("ShardedFusedProdigy", "small"))
    f, fps = run_fused("FusedProdigy", "small", **kw)
    assert same(run4.snapshot(), fused_snapshot(f, fps, PRODIGY_KEYS))
    assert float(run4.opts[0].d) > D0
    for r in (2, 3):
        o = run4.opts[r]
        assert o.n_ranges == 0 and int(o.step_count) == STEPS
        assert not any(getattr(o, k + "_shard").any() for k in PRODIGY_KEYS)
    for o in run4.opts:  # the empty ranks published (0, 0); every rank holds all four records
        recs = o.d_records.view(4, 2)
        assert not recs[2:].any() and recs[:2, 1].gt(0).all() and torch.equal(recs, run4.opts[0].d_records.view(4, 2))
    assert run4.opts[0].n_ranges == 1 and run4.opts[1].n_ranges == 1


# ------------------------------------------------------------------------------------------------------------------
# 6: a non-finite value on one rank
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["other_shard", "own_shard"])
def test_nonfinite_on_one_rank_skips_every_rank(where):
    """One +inf in rank 1's gradient: in tensor [3072] (flat offset 24, rank 0's shard) or in [3, 5, 7] (the end of the
    flat space, rank 1's own shard).  No state, d block, counter or parameter changes on any rank, and the next step
    equals a run that never saw the bad step."""
    kw = dict(lr=1.0, d0=D0, max_grad_norm=1.0, skip_nonfinite=True, zero_grads=True, **HYP)
    run = Run("ShardedFusedProdigy", "main", 2, **kw).run(steps=range(6))
    o0 = run.opts[0]
    assert float(o0.d) > D0  # (the skipped step meets a d block that has moved)
    ti = 2 if where == "other_shard" else 5
    off = o0.flat_offset(run.ps[0][ti])
    assert (off + run.ps[0][ti].numel() <= o0.per) if where == "other_shard" else (off >= o0.per)

    def everything():
        return run.snapshot() + [p.detach().clone() for p in run.ps[1]] + [o.d_block.clone() for o in run.opts] + \
            [o.scalars[3:6].clone() for o in run.opts]

    before = everything()
    for r in range(2):
        set_grads(run.ps[r], "main", 9, r)
    run.ps[1][ti].grad.view(-1)[17] = float("inf")
    run.step_all()
    assert same(everything(), before)
    for r in range(2):
        o = run.opts[r]
        assert int(o.last_step_skipped) == 1 and int(o.nonfinite) == 1 and int(o.step_count) == 6
        assert all(not p.grad.any() for p in run.ps[r])  # zero_grads: zeroed all the same
    replicas_agree(run)
    run.run(steps=[6, 7])  # and the next good steps are taken
    assert all(int(o.step_count) == 8 and int(o.last_step_skipped) == 0 and int(o.nonfinite) == 0 for o in run.opts)
    ref = Run("ShardedFusedProdigy", "main", 2, **kw).run(steps=range(8))
    assert same(run.snapshot(), ref.snapshot())


# ------------------------------------------------------------------------------------------------------------------
# 7: all-zero gradients make no progress, and the unpack is gated on it
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_all_zero_gradients_make_no_progress(weight_decay):
    """tests/test_prodigy_gpu.py::test_all_zero_gradients_make_no_progress on two ranks.  Pass 2 writes nothing in a
    no-progress step, so the gathered staging buffer does not hold the parameters (here: zeros, it was never written):
    an unpack gated on `skipped` alone would overwrite every parameter with it."""
    run = Run("ShardedFusedProdigy", "main", 2, lr=1.0, d0=D0, **dict(HYP, weight_decay=weight_decay))

    def everything():  # master and p0 of the shards (the moments and s are pass 1's), the counter, every parameter byte
        return [run.flat("master"), run.flat("p0"), run.opts[0].step_count.clone()] + \
            [p.detach().clone() for r in range(2) for p in run.ps[r] + [run.idle[r]]]

    before = everything()
    for _ in range(2):
        for r in range(2):
            for p in run.ps[r]:
                p.grad = torch.zeros_like(p)
        run.step_all()
        replicas_agree(run)
        for o in run.opts:
            assert int(o.no_progress) == 1 and int(o.step_count) == 0 and int(o.last_step_skipped) == 0
            assert float(o.d) == D0 and float(o.d_max) == D0 and float(o.d_numerator) == 0.0
            assert float(o.d_denom) == 0.0
    assert not run.opts[0].param_staging.any()
    assert same(everything(), before)
    run.run(steps=range(1))  # and a real gradient moves it on
    replicas_agree(run)
    assert all(int(o.no_progress) == 0 and int(o.step_count) == 1 for o in run.opts)
    assert not torch.equal(run.flat("master"), before[0])
    assert not torch.equal(run.ps[1][4].detach(), before[3 + 4])


# ------------------------------------------------------------------------------------------------------------------
# 8: checkpoints move between world sizes and the single-GPU optimizers
# ------------------------------------------------------------------------------------------------------------------

def test_prodigy_checkpoint_interchange():
    """FusedProdigy -> world 3 -> world 2 -> FusedProdigy through the full format (every rank holds rank 0's
    gradients).  A transfer is exact: right after every load the assembled state, the d block and the counter are the
    source's, bit for bit.  Prodigy's d is not bit-identical across world sizes, so "continued = uninterrupted" is
    claimed per world: a world-3 run stopped at step 6 and reloaded (from the full format, and from the local format
    into the same ranks) ends bit-identical to the world-3 run that was never stopped.  The chain's end passes the
    d gate of the parity test."""
    kw = dict(lr=1.0, d0=D0, use_bias_correction=True, growth_rate=3.0, **HYP)
    f, fps = run_fused("FusedProdigy", "main", steps=range(5), **kw)  # (with these options d leaves d0 in step 4)
    sd = f.state_dict()
    assert sd["step"] == 5 and sd["prodigy"]["d"] > D0
    values = [p.detach().clone() for p in fps]
    # into world 3, with other options in the constructor: the checkpoint's win
    b = Run("ShardedFusedProdigy", "main", 3, values=values, lr=0.5, betas=(0.5, 0.5), d0=1e-3).load_all(sd)
    assert same(b.snapshot(), fused_snapshot(f, fps, PRODIGY_KEYS))
    o = b.opts[1]
    assert o.param_groups[0]["betas"] == HYP["betas"] and o.d0 == D0 and o.use_bias_correction and o.growth_rate == 3.0
    assert all(torch.equal(x.d_block, f.d_block) and int(x.step_count) == 5 for x in b.opts)
    b.run(steps=range(5, 7), same_grads=True, after_step=replicas_agree)
    full = b.full_state_dicts()
    assert sorted(full[0]) == sorted(sd) and full[0]["step"] == 7 and full[0]["prodigy"] == full[2]["prodigy"]
    assert set(full[0]["state"][0]) == set(PRODIGY_KEYS) and sorted(full[0]["state"]) == sorted(sd["state"])
    for k in PRODIGY_KEYS:  # every rank assembles the same full state, in FusedProdigy's shapes
        assert all(torch.equal(full[2]["state"][i][k], full[0]["state"][i][k]) and
                   full[0]["state"][i][k].shape == sd["state"][i][k].shape for i in sd["state"])
    # into world 2
    values = [p.detach().clone() for p in b.ps[0]]
    c = Run("ShardedFusedProdigy", "main", 2, values=values, lr=1.0).load_all(full[0])
    assert same(c.snapshot(), b.snapshot())
    c.run(steps=range(7, 9), same_grads=True, after_step=replicas_agree)
    # and back into FusedProdigy
    full2 = c.full_state_dicts()[1]
    ps, _, allp = make_params("main", [p.detach().clone() for p in c.ps[0]])
    g = _cls("FusedProdigy")(allp, lr=1.0)
    g.load_state_dict(full2)
    assert same(fused_snapshot(g, ps, PRODIGY_KEYS), c.snapshot())
    run_fused("FusedProdigy", "main", steps=range(9, STEPS), opt=g, ps=ps)
    _, dd64, _, _, dd32, _ = restatement("main", 0, torch.float64, use_bias_correction=True, growth_rate=3.0) + \
        restatement("main", 0, torch.float32, use_bias_correction=True, growth_rate=3.0)
    assert int(g.step_count) == STEPS and dd64 >= 5 * D0
    assert abs(float(g.d) - dd64) / dd64 <= 2.0 * abs(dd32 - dd64) / dd64
    # continued = uninterrupted, in the same world: from the full format and from the local format
    never = Run("ShardedFusedProdigy", "main", 3, **kw).run()
    a = Run("ShardedFusedProdigy", "main", 3, **kw).run(steps=range(6))
    full_a, local = a.full_state_dicts()[0], [o.state_dict() for o in a.opts]
    assert local[1]["world"] == 3 and local[1]["rank"] == 1 and local[1]["per"] == a.opts[1].per
    assert set(PRODIGY_KEYS) <= set(local[1]) and local[1]["prodigy"] == full_a["prodigy"]
    values = [p.detach().clone() for p in a.ps[0]]
    d = Run("ShardedFusedProdigy", "main", 3, values=values, lr=1.0).load_all(full_a)
    e = Run("ShardedFusedProdigy", "main", 3, values=values, lr=1.0)
    for o, s in zip(e.opts, local):
        o.load_state_dict(s)
    assert same(d.snapshot(), a.snapshot()) and same(e.snapshot(), a.snapshot())
    local[0]["master"].zero_()  # the state dict holds clones
    assert same(e.snapshot(), a.snapshot())
    assert same(d.run(steps=range(6, STEPS)).snapshot(), never.snapshot())
    assert same(e.run(steps=range(6, STEPS)).snapshot(), never.snapshot())
    # what must be refused
    with pytest.raises(ValueError):
        e.opts[0].load_state_dict(local[1])  # another rank's shard
    with pytest.raises(ValueError):
        c.opts[0].load_state_dict(local[0])  # another world's shard
    no_d = {k: v for k, v in full_a.items() if k != "prodigy"}
    with pytest.raises(ValueError, match="d block"):
        e.opts[0].load_state_dict(no_d)
    with pytest.raises(ValueError, match="d block"):
        e.opts[0].load_state_dict({k: v for k, v in local[0].items() if k != "prodigy"})
    assert same(e.snapshot(), never.snapshot())  # a refused dict changed nothing


def test_adam_checkpoint_interchange():
    """FusedAdam -> world 4 -> world 2 -> FusedAdam with rank 0's gradients on every rank and no clip: Adam is
    element-wise and the mean over 2 or 4 equal gradients is exact, so the chain ends bit-identical to FusedAdam run
    without a stop; the local format reloads into the same rank."""
    kw = dict(lr=ADAM_LR, **HYP)
    never, nps = run_fused("FusedAdam", "main", **kw)
    want = fused_snapshot(never, nps, ADAM_KEYS)
    f, fps = run_fused("FusedAdam", "main", steps=range(3), **kw)
    b = Run("ShardedFusedAdam", "main", 4, values=[p.detach() for p in fps], lr=0.5, betas=(0.5, 0.5))
    b.load_all(f.state_dict()).run(steps=range(3, 6), same_grads=True)
    assert b.opts[0].param_groups[0]["betas"] == HYP["betas"]
    full = b.full_state_dicts()[3]
    assert sorted(full) == ["param_groups", "state", "step"] and full["step"] == 6
    c = Run("ShardedFusedAdam", "main", 2, values=[p.detach() for p in b.ps[0]], lr=0.5).load_all(full)
    c.run(steps=range(6, 8), same_grads=True)
    local = [o.state_dict() for o in c.opts]
    d = Run("ShardedFusedAdam", "main", 2, values=[p.detach() for p in c.ps[0]], lr=0.5)
    for o, s in zip(d.opts, local):
        o.load_state_dict(s)
    assert same(d.snapshot(), c.snapshot())
    with pytest.raises(ValueError):
        d.opts[0].load_state_dict(local[1])
    d.run(steps=range(8, 10), same_grads=True)
    ps, _, allp = make_params("main", [p.detach().clone() for p in d.ps[0]])
    g = _cls("FusedAdam")(allp, lr=0.5)
    g.load_state_dict(d.full_state_dicts()[0])
    run_fused("FusedAdam", "main", steps=range(10, STEPS), opt=g, ps=ps)
    assert same(fused_snapshot(g, ps, ADAM_KEYS), want)


# ------------------------------------------------------------------------------------------------------------------
# 9: unaligned gradient views, gradients reallocated every step
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["unaligned", "fresh"])
def test_unaligned_and_reallocated_gradients_pass_the_parity_gate(mode):
    """p.grad = None before every step, then new gradient tensors: views at odd element offsets of larger buffers
    (pack's scalar head and its whole-chunk scalar path), or plain new tensors at other addresses (the table upload
    every step).  The gates of test_update_parity at world 2; pack is element-wise, so the result is also bit-equal to
    the run with persistent aligned gradients."""
    ptrs = []

    def note(run, s):
        replicas_agree(run, s)
        ptrs.append([p.grad.data_ptr() for p in run.ps[0]])
        if mode == "unaligned":
            assert any(p.grad.data_ptr() % 16 for p in run.ps[0]) and any(p.grad.data_ptr() % 4 for p in run.ps[0])

    run = prodigy_run(2, "default", after_step=note, mode=mode)
    check_parity(run, 2, "default")
    assert same(run.snapshot(), prodigy_run(2, "default").snapshot())
    assert len(ptrs) == STEPS


# ------------------------------------------------------------------------------------------------------------------
# 10: no host synchronisation in step()
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", ["ShardedFusedProdigy", "ShardedFusedAdam"])
def test_no_host_synchronisation(cls):
    """tests/test_prodigy_gpu.py::test_no_host_synchronisation's method: torch's synchronisation check set to raise
    around a step with persistent gradients and a step with reallocated ones (the table upload)."""
    kw = dict(lr=1.0, d0=D0) if cls == "ShardedFusedProdigy" else dict(lr=ADAM_LR)
    run = Run(cls, "main", 1, max_grad_norm=1.0, skip_nonfinite=True, zero_grads=True, **kw, **HYP)
    run.run(steps=range(1))
    opt, ps = run.opts[0], run.ps[0]
    fresh = [g.to(dev) for g in data("main")[1][1][0]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        for p, g in zip(ps, fresh):
            p.grad = g
        opt.step()
        states = [opt.grad_norm, opt.clip_coef, opt.last_step_skipped, opt.step_count, opt.nonfinite]
        if cls == "ShardedFusedProdigy":
            states = [opt.d, opt.d_max, opt.d_hat, opt.d_numerator, opt.d_denom, opt.dlr, opt.no_progress, opt.d_block,
                      opt.master_shard, opt.exp_avg_shard, opt.exp_avg_sq_shard, opt.s_shard, opt.p0_shard] + states
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in states)
    if cls == "ShardedFusedProdigy":
        assert all(t.dtype == torch.float64 for t in states[:6]) and states[6].dtype == torch.int32
    assert int(opt.step_count) == 3  # (the second met all-zero gradients, zero_grads had cleared them: still a step)


# ------------------------------------------------------------------------------------------------------------------
# 11: the whole step through RCCL at world size 1
# ------------------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture
def rccl_world1(monkeypatch):
    import torch.distributed as dist
    from videopainter_amd import distributed as VD
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", str(_free_port())), ("RANK", "0"),
                 ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
        monkeypatch.setenv(k, v)
    d = torch.device("cuda", 0)
    torch.cuda.set_device(d)
    VD.init("nccl", d)
    try:
        assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
        yield d
    finally:
        dist.destroy_process_group()


def test_full_step_on_rccl_world1(rccl_world1):
    """The reduce-scatter and the three all-gathers (the 16-byte record of doubles among them) run in RCCL on the
    device buffers; 12 steps of both optimizers equal the LocalComm world-1 result bit for bit."""
    from videopainter_amd import distributed as VD
    for cls, keys, kw in (("ShardedFusedProdigy", PRODIGY_KEYS, dict(lr=1.0, d0=D0)),
                          ("ShardedFusedAdam", ADAM_KEYS, dict(lr=ADAM_LR))):
        ps, idle, allp = make_params("main")
        opt = _cls(cls)(allp, **kw, **HYP)  # the default process group
        assert isinstance(opt.comm, VD.GroupComm) and (opt.world, opt.rank) == (1, 0)
        assert VD._staged(opt.grad_staging).host is False and VD._staged(opt.param_staging).host is False
        for s in range(STEPS):
            set_grads(ps, "main", s, 0)
            opt.step()
        n = opt.total
        extra = [opt.d_block.clone()] if cls == "ShardedFusedProdigy" else []
        got = [getattr(opt, k + "_shard")[:n] for k in keys] + extra + [opt.step_count.clone()] + \
            [p.detach() for p in ps]
        assert same(got, world1(cls)), cls
        sd = opt.full_state_dict()  # (collective; world 1)
        assert sd["step"] == STEPS and torch.equal(sd["state"][0]["master"].reshape(-1), opt.master_shard[:1])
