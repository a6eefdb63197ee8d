"""fp32 gradient accumulation on the GPU: `accumulate()` / `pending` / `reset_accumulation()` of the six fused
optimizers (videopainter_amd/optim.py, zero.py) and the kernels behind them (vp_mt_accumulate_bf16 and the
fp32-gradient norm and update passes, csrc/optim.hip, csrc/prodigy.hip).

Parameter set: tests/test_zero_gpu.py's main set — bf16 tensors of shapes [1], [7], [3072], [CHUNK+1], [64, 3072],
[3, 5, 7] plus one parameter whose .grad is None (index 2 of the optimizer's list).  With `views`, the [7] and [3072]
parameters and their gradients are slices at storage offsets of 1 and 3 elements (the all-scalar paths) and the
[CHUNK+1] pair at offset 4 (a scalar head of four before the vector body).  Weights N(0, 0.02^2); micro-batch gradients
N(0, 1e-3^2) in bf16, one set per (step, rank, micro-batch), generated once and never modified; for Prodigy they are
correlated across the 12 steps as in tests/test_prodigy_gpu.py.  Hyper-parameters are those files'.  Sharded ranks are
threads over distributed.LocalComm.  torch references are computed once per configuration and shared."""
import functools
import math
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16
HYP = dict(betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)
LRS = [1e-5, 8e-6, 1.2e-5, 5e-6, 9e-6]
STEPS = 5
PSTEPS = 12  # Prodigy
D0 = 1e-6
ADAM_KEYS = ("master", "exp_avg", "exp_avg_sq")
PRODIGY_KEYS = ADAM_KEYS + ("s", "p0")
SINGLE = {"FusedAdamW": "ShardedFusedAdamW", "FusedAdam": "ShardedFusedAdam", "FusedProdigy": "ShardedFusedProdigy"}
VIEW_OFFSETS = {1: 1, 2: 3, 3: 4}  # index in the set -> storage offset in elements


def _shapes():
    from videopainter_amd.optim import CHUNK
    return [(1,), (7,), (3072,), (CHUNK + 1,), (64, 3072), (3, 5, 7)]


@functools.lru_cache(maxsize=None)
def weights():
    g = torch.Generator().manual_seed(40)
    return tuple((torch.randn(s, generator=g) * 0.02).to(BF16) for s in _shapes())


@functools.lru_cache(maxsize=None)
def _base():
    g = torch.Generator().manual_seed(43)
    return tuple(torch.randn(s, generator=g) for s in _shapes())


@functools.lru_cache(maxsize=None)
def micro(step, rank=0, j=0, correlated=False):
    """The bf16 gradients of micro-batch j of `step` on `rank` (CPU)."""
    g = torch.Generator().manual_seed(100000 + 1000 * step + 10 * rank + j + (500000 if correlated else 0))
    if correlated:
        return tuple(((b + 0.5 * torch.randn(b.shape, generator=g)) * 1e-3).to(BF16) for b in _base())
    return tuple((torch.randn(s, generator=g) * 1e-3).to(BF16) for s in _shapes())


def make_params(views=False):
    """(ps, idle, the optimizer's list, the backing buffers of the views)."""
    ps, bufs = [], []
    for i, t in enumerate(weights()):
        if views and i in VIEW_OFFSETS:
            o, n = VIEW_OFFSETS[i], t.numel()
            buf = torch.zeros(n + 16, device=dev, dtype=BF16)
            p = torch.nn.Parameter(buf[o:o + n].view(t.shape))
            p.data.copy_(t)
            bufs.append(buf)
        else:
            p = torch.nn.Parameter(t.to(dev))
        ps.append(p)
    idle = torch.nn.Parameter(torch.full((5,), 0.25, device=dev, dtype=BF16))
    return ps, idle, ps[:2] + [idle] + ps[2:], bufs


def set_grads(ps, grads, views=False, mode="persistent"):
    """mode: "persistent" copies into the existing .grad, "fresh" assigns new tensors, "add" adds into the existing
    .grad as autograd does (bf16)."""
    for i, (p, g) in enumerate(zip(ps, grads)):
        if p.grad is not None and mode != "fresh":
            p.grad.add_(g.to(dev)) if mode == "add" else p.grad.copy_(g)
        elif views and i in VIEW_OFFSETS:
            o, n = VIEW_OFFSETS[i], g.numel()
            p.grad = torch.zeros(n + 16, device=dev, dtype=BF16)[o:o + n].view(g.shape)
            p.grad.copy_(g)
        else:
            p.grad = g.to(dev).clone()


def make_opt(cls, allp, **kw):
    import videopainter_amd as V
    if "Prodigy" in cls:
        return getattr(V, cls)(allp, **dict(dict(HYP, lr=1.0, d0=D0), **kw))
    return getattr(V, cls)(allp, **dict(dict(HYP, lr=LRS[0]), **kw))


def n_steps(cls):
    return PSTEPS if "Prodigy" in cls else STEPS


def set_lr(opt, cls, s):
    if "Prodigy" not in cls:
        for grp in opt.param_groups:
            grp["lr"] = LRS[s]


def keys_of(cls):
    return PRODIGY_KEYS if "Prodigy" in cls else ADAM_KEYS


def snapshot(opt, ps, cls):
    """Everything a step writes but the grad_norm word: bf16 parameters, the state, the scalars block from clip_coef
    on, Prodigy's d block."""
    out = [t.clone() for p in ps for t in (p.detach(), *(opt.state[p][k] for k in keys_of(cls)))]
    out.append(opt.scalars[2:].clone())
    if "Prodigy" in cls:
        out.append(opt.d_block.clone())
    return out


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
                                    for x, y in zip(a, b))


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def run_single(cls, k, grads_of, views=False, steps=None, mode="persistent", opt=None, ps=None, **kw):
    """`cls` over `steps` optimizer steps of k micro-batches each (k = 0: one plain step() per step on grads_of(s, 0));
    returns (opt, ps, bufs)."""
    bufs = None
    if opt is None:
        ps, _, allp, bufs = make_params(views)
        opt = make_opt(cls, allp, **kw)
    for s in (range(n_steps(cls)) if steps is None else steps):
        set_lr(opt, cls, s)
        for j in range(max(k, 1)):
            if mode == "fresh":
                for p in ps:
                    p.grad = None
            set_grads(ps, grads_of(s, j), views, mode)
            if j < k - 1:
                opt.accumulate()
                assert opt.pending == j + 1
            else:
                opt.step()
                assert opt.pending == 0
    return opt, ps, bufs


# ------------------------------------------------------------------------------------------------------------------
# 1: the fold kernel, per element
# ------------------------------------------------------------------------------------------------------------------

def _fold_run():
    """Three folds (the last scaled by fl(1/3) and zeroing the gradients) over a table of its own: every tensor's
    accumulator region sits between 8-element guards, tensor 2 has no gradient, gradients are slices at element
    offsets 0, 1, 3, 4, 0, 2.  Returns what the checks need, on the CPU."""
    from videopainter_amd import kernels as K
    from videopainter_amd.optim import DeviceTables, _align, build_chunk_table, build_tensor_table
    shapes = _shapes()
    numels = [math.prod(s) for s in shapes]
    numels.insert(2, 5)  # the tensor without a gradient
    goffs = [0, 1, None, 3, 4, 0, 2]
    offs, at = [], 8
    for n in numels:
        offs.append(at)
        at += _align(n) + 8
    sentinel = 777.0
    acc = torch.full((at,), sentinel, device=dev, dtype=torch.float32)
    gbufs = [None if o is None else torch.full((n + 16,), 3.0, device=dev, dtype=BF16) for n, o in zip(numels, goffs)]
    gviews = [None if b is None else b[o:o + n] for b, n, o in zip(gbufs, numels, goffs)]
    t = DeviceTables(torch.device(dev))
    tt = build_tensor_table([0 if v is None else v.data_ptr() for v in gviews], [0] * len(numels), offs, numels)
    ct = build_chunk_table(numels)
    t.upload("fold", (tt, ct), int(ct.shape[0]))
    gs = [[g.reshape(-1) for g in micro(0, 0, j)] for j in range(3)]
    after = []
    for j in range(3):
        it = iter(gs[j])
        for v in gviews:
            if v is not None:
                v.copy_(next(it))
        K.mt_accumulate(t.buf, t.table(1), int(ct.shape[0]), acc, first=j == 0, scale=1.0 / 3 if j == 2 else 1.0,
                        zero_grads=j == 2)
        after.append(acc.cpu())
        if j == 0:  # mark the idle tensor's region: later folds must leave it alone
            acc[offs[2]:offs[2] + 5] = 5.0
    torch.cuda.synchronize()
    return dict(numels=numels, offs=offs, goffs=goffs, sentinel=sentinel, after=after, gs=gs,
                gbufs=[None if b is None else b.cpu() for b in gbufs], total=at)


def test_fold_per_element():
    r = _fold_run()
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    covered = torch.zeros(r["total"], dtype=torch.bool)
    it = [iter(g) for g in r["gs"]]
    for i, (n, o, go) in enumerate(zip(r["numels"], r["offs"], r["goffs"])):
        covered[o:o + n] = True
        if go is None:  # zeros after the first fold, untouched (the mark) by the later ones
            assert not r["after"][0][o:o + n].any()
            assert torch.equal(r["after"][2][o:o + n], torch.full((n,), 5.0))
            continue
        g1, g2, g3 = (next(x).float() for x in it)
        assert torch.equal(r["after"][0][o:o + n], g1), i
        assert torch.equal(r["after"][1][o:o + n], g1 + g2), i
        got = r["after"][2][o:o + n]
        assert torch.equal(got, ((g1 + g2) + g3) * third), i  # one rounding per add, one for the product
        exact = (g1.double() + g2.double() + g3.double()) / 3.0
        allow = 2.0 * 2.0 ** -24 * (g1.abs() + g2.abs() + g3.abs()).double()
        err = (got.double() - exact).abs()
        assert bool((err <= allow).all()), (i, float((err / allow.clamp_min(1e-300)).max()))
        buf = r["gbufs"][i]  # zero_grads zeroed exactly the gradient
        assert not buf[go:go + n].any()
        assert bool((buf[:go] == 3.0).all()) and bool((buf[go + n:] == 3.0).all())
    for a in r["after"]:  # guards and padding stay as they were
        assert bool((a[~covered] == r["sentinel"]).all())
    again = _fold_run()
    assert all(torch.equal(a, b) for a, b in zip(r["after"], again["after"]))  # run to run


# ------------------------------------------------------------------------------------------------------------------
# 2: equal micro-gradients: the mean is the gradient itself
# ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plain_ref(cls, max_norm):
    """`cls` stepping once per step on micro-batch 0 (views): (snapshot, masters, grad_norm), computed once."""
    corr = "Prodigy" in cls
    opt, ps, _ = run_single(cls, 0, lambda s, j: micro(s, 0, 0, corr), views=True, max_grad_norm=max_norm)
    return snapshot(opt, ps, cls), torch.cat([opt.state[p]["master"].reshape(-1) for p in ps]), float(opt.grad_norm)


@pytest.mark.parametrize("max_norm", [None, 0.1])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("cls", list(SINGLE))
def test_equal_micro_gradients_match_the_plain_step(cls, k, max_norm):
    """k equal micro-batches: g + g (+ g + g) and the product with 1/2 (1/4) are exact, so the accumulated mean is g.
    Without a clip every buffer, the bf16 parameters, the d block and the scalars block but its grad_norm word are
    bit-identical to the optimizer stepping on g; grad_norm is within 1e-5 (fp32 values are summed four to a vector,
    bf16 values eight: n non-negative terms in a fixed-order tree, <= log2(n) 2^-24 ~ 2e-6).  With the clip active the
    coefficient may differ in its last bits: rel-L2 of the masters < 1e-6 (fp32 masters an ulp or two apart)."""
    corr = "Prodigy" in cls
    ref, ref_master, ref_norm = plain_ref(cls, max_norm)
    opt, ps, _ = run_single(cls, k, lambda s, j: micro(s, 0, 0, corr), views=True, max_grad_norm=max_norm)
    gn = float(opt.grad_norm)
    print(f"{cls} k={k} clip={max_norm}: grad_norm {gn:.9g} (plain {ref_norm:.9g}) coef {float(opt.clip_coef):.9g}")
    assert abs(gn - ref_norm) <= 1e-5 * ref_norm
    assert int(opt.step_count) == n_steps(cls) and opt.grad_accumulator.dtype == torch.float32
    if max_norm is None:
        assert same(snapshot(opt, ps, cls), ref)
    else:
        assert float(opt.clip_coef) < 1.0
        assert rel(torch.cat([opt.state[p]["master"].reshape(-1) for p in ps]), ref_master) < 1e-6


# ------------------------------------------------------------------------------------------------------------------
# 3: distinct micro-gradients against float64 on the float64 mean
# ------------------------------------------------------------------------------------------------------------------

def mean_grads(dtype, s, k, world=1, correlated=False):
    """The mean over ranks and micro-batches of the bf16 gradients of step s, taken in `dtype`."""
    sets = [micro(s, r, j, correlated) for r in range(world) for j in range(k)]
    return [sum(g[i].to(dtype) for g in sets) / (k * world) for i in range(len(sets[0]))]


@functools.lru_cache(maxsize=None)
def torch_ref(cls, dtype, k, world=1):
    """torch.optim.AdamW / Adam on `dtype` CPU copies stepped on mean_grads: master - initial."""
    w = weights()
    ps = [torch.nn.Parameter(t.to(dtype)) for t in w]
    T = torch.optim.AdamW if cls.endswith("AdamW") else torch.optim.Adam
    opt = T(ps, lr=LRS[0], **HYP)
    for s in range(STEPS):
        opt.param_groups[0]["lr"] = LRS[s]
        for p, g in zip(ps, mean_grads(dtype, s, k, world)):
            p.grad = g
        opt.step()
    return torch.cat([(p.detach().double() - t.double()).reshape(-1) for p, t in zip(ps, w)])


@functools.lru_cache(maxsize=None)
def prodigy_ref(dtype, k, world=1, equal=False):
    """tests/test_prodigy_gpu.py's restatement of prodigyopt 1.0's step() (default options, no clip) in torch ops on
    `dtype` CPU copies, stepped on mean_grads (equal: on micro-batch 0 itself): (master - initial, d)."""
    w = weights()
    p = [t.to(dtype) for t in w]
    p0 = [t.clone() for t in p]
    m, v, sq = ([torch.zeros_like(t) for t in p] for _ in range(3))
    beta1, beta2 = HYP["betas"]
    beta3, wd, eps = math.sqrt(beta2), HYP["weight_decay"], HYP["eps"]
    d = d_max = D0
    num = 0.0
    for t in range(PSTEPS):
        grads = [g.to(dtype) for g in micro(t, 0, 0, True)] if equal else mean_grads(dtype, t, k, world, True)
        dlr = d * 1.0
        num *= beta3
        den = dot = 0.0
        for i, g in enumerate(grads):
            dot += torch.dot(g.flatten(), (p0[i] - p[i]).flatten()).item()
            m[i].mul_(beta1).add_(g, alpha=d * (1 - beta1))
            v[i].mul_(beta2).addcmul_(g, g, value=d * d * (1 - beta2))
            sq[i].mul_(beta3).add_(g, alpha=(d / D0) * dlr)
            den += sq[i].abs().sum().item()
        num += (d / D0) * dlr * dot
        if den == 0:
            continue
        d_hat = num / den
        if d == D0:
            d = max(d, d_hat)
        d_max = max(d_max, d_hat)
        d = min(d_max, d * float("inf"))
        for i in range(len(p)):
            denom = v[i].sqrt().add_(d * eps)
            p[i].add_(p[i], alpha=-wd * dlr)
            p[i].addcdiv_(m[i], denom, value=-dlr)
    return torch.cat([(a.double() - b.double()).reshape(-1) for a, b in zip(p, w)]), d


def master_delta(opt, ps):
    return torch.cat([(opt.state[p]["master"].double().cpu() - t.double()).reshape(-1)
                      for p, t in zip(ps, weights())])


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedAdam"])
def test_distinct_micro_gradients_parity(cls, k):
    """D = master after 5 steps - initial.  Gate: rel-L2(D, D_fp64) <= 2 x rel-L2(D_torch_fp32, D_fp64), both torch
    references stepping on the mean of the bf16 micro-gradients taken in their own dtype.  Contrast (FusedAdamW): the
    same optimizer stepping on gradients accumulated in bf16 — each micro-batch's bf16(g / k), as a loss / k gives,
    added into .grad with a bf16 rounding per add, as autograd does — must FAIL the same gate: that is the loss the
    fp32 accumulator exists to avoid."""
    d64, d32 = torch_ref(cls, torch.float64, k), torch_ref(cls, torch.float32, k)
    opt, ps, _ = run_single(cls, k, lambda s, j: micro(s, 0, j))
    r_acc, r_t = rel(master_delta(opt, ps), d64), rel(d32, d64)
    print(f"{cls} k={k}: fp32 accumulation {r_acc:.3e}  torch-fp32 {r_t:.3e}  ratio {r_acc / r_t:.3f}")
    assert float(d64.norm()) > 0 and r_acc <= 2.0 * r_t
    if cls != "FusedAdamW":
        return

    def bf16_sum(s, j):
        acc = None
        for jj in range(k):
            part = [(g.float() / k).to(BF16) for g in micro(s, 0, jj)]
            acc = part if acc is None else [(a + b) for a, b in zip(acc, part)]  # bf16 + bf16 -> bf16
        return acc

    opt, ps, _ = run_single(cls, 0, bf16_sum)
    r_bf = rel(master_delta(opt, ps), d64)
    print(f"{cls} k={k}: bf16 accumulation {r_bf:.3e}  = {r_bf / r_t:.1f} x torch-fp32 (the gate is 2 x)")
    assert r_bf > 2.0 * r_t


@pytest.mark.parametrize("k", [3, 8])
def test_distinct_micro_gradients_parity_prodigy(k):
    """The same gate for FusedProdigy against the float64 restatement on the float64 mean, 12 correlated steps, and
    on d: |d - d_fp64| / d_fp64 <= 2 x the fp32 restatement's."""
    (d64, dd64), (d32, dd32) = prodigy_ref(torch.float64, k), prodigy_ref(torch.float32, k)
    assert dd64 >= 5 * D0, "the inputs must move d, or the d update is not tested"
    opt, ps, _ = run_single("FusedProdigy", k, lambda s, j: micro(s, 0, j, True))
    r_acc, r_t = rel(master_delta(opt, ps), d64), rel(d32, d64)
    d = float(opt.d)
    e_acc, e_t = abs(d - dd64) / dd64, abs(dd32 - dd64) / dd64
    print(f"FusedProdigy k={k}: delta {r_acc:.3e} (fp32 {r_t:.3e})  d {d:.6e} (fp64 {dd64:.6e}) err {e_acc:.3e} "
          f"(fp32 {e_t:.3e})")
    assert r_acc <= 2.0 * r_t and e_acc <= 2.0 * e_t
    assert int(opt.step_count) == PSTEPS and int(opt.no_progress) == 0


# ------------------------------------------------------------------------------------------------------------------
# 4: a non-finite value in one micro-batch
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [0, 1, 2])
@pytest.mark.parametrize("cls", list(SINGLE))
def test_nonfinite_micro_batch_skips_the_step(cls, bad):
    """One +inf in micro-batch `bad` of 3 stays non-finite in the fp32 sum: the whole step is skipped, nothing but the
    scalars block changes, `pending` is 0 again and the next step is an ordinary one."""
    corr = "Prodigy" in cls
    kw = dict(skip_nonfinite=True, zero_grads=True, max_grad_norm=1.0)
    grads = lambda s, j: micro(s, 0, j, corr)  # noqa: E731
    opt, ps, _ = run_single(cls, 3, grads, steps=range(2), mode="add", **kw)
    before = snapshot(opt, ps, cls)
    for j in range(3):
        set_grads(ps, grads(2, j), mode="add")
        if j == bad:
            ps[4].grad.view(-1)[17] = float("inf")
        opt.accumulate() if j < 2 else opt.step()
    assert opt.pending == 0
    assert int(opt.last_step_skipped) == 1 and int(opt.nonfinite) == 1 and int(opt.step_count) == 2
    after = snapshot(opt, ps, cls)
    skip = len(ps) * (1 + len(keys_of(cls)))  # (the scalars block is where the skip is recorded)
    assert same(after[:skip] + after[skip + 1:], before[:skip] + before[skip + 1:])
    assert all(not p.grad.any() for p in ps)  # zero_grads: zeroed all the same
    run_single(cls, 3, grads, steps=[2], mode="add", opt=opt, ps=ps)
    assert int(opt.last_step_skipped) == 0 and int(opt.nonfinite) == 0 and int(opt.step_count) == 3
    ref, rps, _ = run_single(cls, 3, grads, steps=range(3), mode="add", **kw)
    assert same(snapshot(opt, ps, cls), snapshot(ref, rps, cls))


# ------------------------------------------------------------------------------------------------------------------
# 5: where the gradients live
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", list(SINGLE))
def test_reallocated_and_persistent_gradients_agree(cls):
    """p.grad = None and fresh tensors every micro-batch (the tables are rebuilt) against persistent gradients that
    zero_grads zeroes in the fold and the next micro-batch is ADDED into, as autograd adds: bit-identical."""
    corr = "Prodigy" in cls
    grads = lambda s, j: micro(s, 0, j, corr)  # noqa: E731
    a, aps, _ = run_single(cls, 3, grads, steps=range(3), mode="fresh")
    b, bps, _ = run_single(cls, 3, grads, steps=range(3), mode="add", zero_grads=True)
    assert same(snapshot(a, aps, cls), snapshot(b, bps, cls))
    assert torch.equal(a.scalars, b.scalars)
    assert all(not p.grad.any() for p in bps) and all(p.grad.any() for p in aps)


# ------------------------------------------------------------------------------------------------------------------
# 6: errors
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", list(SINGLE))
def test_errors_and_reset(cls):
    corr = "Prodigy" in cls
    grads = lambda s, j: micro(s, 0, j, corr)  # noqa: E731
    opt, ps, _ = run_single(cls, 2, grads, steps=range(1))
    sd = opt.state_dict()
    assert opt.pending == 0 and opt.grad_accumulator is not None
    clean = snapshot(opt, ps, cls)
    set_grads(ps, grads(1, 0))
    opt.accumulate()
    assert opt.pending == 1
    for call in (opt.state_dict, lambda: opt.load_state_dict(sd)):
        with pytest.raises(RuntimeError):
            call()
    kept = ps[0].grad
    ps[0].grad = None  # another active set inside one step
    with pytest.raises(ValueError):
        opt.accumulate()
    with pytest.raises(ValueError):
        opt.step()
    assert opt.pending == 1 and same(snapshot(opt, ps, cls), clean)
    ps[0].grad = kept
    opt.reset_accumulation()
    assert opt.pending == 0
    opt.load_state_dict(sd)  # (allowed again)
    run_single(cls, 2, grads, steps=[1], opt=opt, ps=ps)  # a clean step: the dropped fold left no trace
    ref, rps, _ = run_single(cls, 2, grads, steps=range(2))
    assert same(snapshot(opt, ps, cls), snapshot(ref, rps, cls))


def test_sharded_checkpoint_methods_refuse_pending_folds():
    from videopainter_amd.distributed import LocalComm
    ps, _, allp, _ = make_params()
    opt = make_opt("ShardedFusedProdigy", allp, comm=LocalComm(1), rank=0)
    sd = opt.state_dict()
    set_grads(ps, micro(0))
    opt.accumulate()
    for call in (opt.state_dict, opt.full_state_dict, lambda: opt.load_state_dict(sd)):
        with pytest.raises(RuntimeError):
            call()
    ps[1].grad = None
    with pytest.raises(ValueError):
        opt.step()
    opt.reset_accumulation()
    assert opt.pending == 0 and opt.full_state_dict()["step"] == 0


# ------------------------------------------------------------------------------------------------------------------
# 7: the sharded classes
# ------------------------------------------------------------------------------------------------------------------

def counting_comm(world):
    from videopainter_amd.distributed import LocalComm

    class Counting(LocalComm):
        def __init__(self, P):
            super().__init__(P)
            self.calls = [[] for _ in range(P)]

        def reduce_scatter_sum(self, rank, out, flat):
            self.calls[rank].append("reduce_scatter")
            super().reduce_scatter_sum(rank, out, flat)

        def all_gather(self, rank, out, inp):
            self.calls[rank].append("all_gather")
            super().all_gather(rank, out, inp)

    return Counting(world)


class Run:
    """`world` sharded optimizers of the class behind `cls` over one counting LocalComm."""

    def __init__(self, cls, world, **kw):
        self.cls, self.world, self.comm = cls, world, counting_comm(world)
        self.ps, self.opts = [], []
        for r in range(world):
            ps, _, allp, _ = make_params()
            self.ps.append(ps)
            self.opts.append(make_opt(SINGLE[cls], allp, comm=self.comm, rank=r, **kw))

    def run(self, k, grads_of, steps=None):
        """grads_of(s, r, j); after every optimizer step the replicas must agree bit for bit."""
        collectives = 4 if "Prodigy" in self.cls else 3
        for s in (range(n_steps(self.cls)) if steps is None else steps):
            for j in range(k):
                for r in range(self.world):
                    set_lr(self.opts[r], self.cls, s)
                    set_grads(self.ps[r], grads_of(s, r, j))
                before = [len(c) for c in self.comm.calls]
                if j < k - 1:
                    self.comm.run(lambda r: self.opts[r].accumulate())
                    assert [len(c) for c in self.comm.calls] == before  # no collective
                else:
                    self.comm.run(lambda r: self.opts[r].step())
                    assert [len(c) - b for c, b in zip(self.comm.calls, before)] == [collectives] * self.world
                assert all(o.pending == (j + 1 if j < k - 1 else 0) for o in self.opts)
            for r in range(1, self.world):
                assert torch.equal(self.opts[r].scalars, self.opts[0].scalars), (s, r)
                assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(self.ps[r], self.ps[0])), (s, r)
                if "Prodigy" in self.cls:
                    assert torch.equal(self.opts[r].d_block, self.opts[0].d_block), (s, r)
        return self

    def flat(self, name):
        return torch.cat([getattr(o, name + "_shard") for o in self.opts])[:self.opts[0].total]

    def snapshot(self):
        out = [self.flat(k) for k in keys_of(self.cls)] + [p.detach().clone() for p in self.ps[0]]
        out.append(self.opts[0].scalars[2:].clone())
        if "Prodigy" in self.cls:
            out.append(self.opts[0].d_block.clone())
        return out

    def delta(self):
        m, off = self.flat("master").double().cpu(), self.opts[0].flat_offset
        return torch.cat([m[off(p):off(p) + t.numel()] - t.double().reshape(-1)
                          for p, t in zip(self.ps[0], weights())])


@pytest.mark.parametrize("cls", list(SINGLE))
def test_world1_accumulation_is_bit_identical_to_the_single_gpu_class(cls):
    """Distinct micro-gradients, k = 3: the world-1 sharded optimizer's accumulate() / step() against the single-GPU
    class's, in everything but the grad_norm word (the shard sums its ranges, the single-GPU class its chunks)."""
    corr = "Prodigy" in cls
    opt, ps, _ = run_single(cls, 3, lambda s, j: micro(s, 0, j, corr))
    run = Run(cls, 1).run(3, lambda s, r, j: micro(s, 0, j, corr))
    o = run.opts[0]
    for p, q in zip(ps, run.ps[0]):
        assert torch.equal(p.detach(), q.detach())
        at = o.flat_offset(q)
        for k in keys_of(cls):
            assert torch.equal(opt.state[p][k].reshape(-1), run.flat(k)[at:at + p.numel()]), k
    assert torch.equal(opt.scalars[1:], o.scalars[1:])
    assert abs(float(opt.grad_norm) - float(o.grad_norm)) <= 1e-5 * float(opt.grad_norm)
    if corr:
        assert torch.equal(opt.d_block, o.d_block) and float(o.d) > 5 * D0
    assert o.grad_accumulator.data_ptr() == o.grad_staging.data_ptr()  # no memory of its own


@functools.lru_cache(maxsize=None)
def world1_equal(cls):
    corr = "Prodigy" in cls
    return tuple(Run(cls, 1).run(2, lambda s, r, j: micro(s, 0, 0, corr)).snapshot())


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedAdam"])
def test_sharding_invariance_with_accumulation(cls, world):
    """Every rank and both micro-batches have the same gradients: the sum of two, the scale 1 / (2 P) and the P-term
    reduce-scatter are exact for P = 2, 4, so the result is bit-identical to world 1."""
    run = Run(cls, world).run(2, lambda s, r, j: micro(s, 0, 0))
    assert same(run.snapshot(), list(world1_equal(cls)))
    for r in range(world):
        assert same([p.detach() for p in run.ps[r]], [p.detach() for p in run.ps[0]])


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedAdam"])
def test_world3_distinct_gradients_parity(cls):
    """World 3, k = 2, distinct gradients per rank and micro-batch: the gate of test 3 against the float64 mean over
    ranks and micro-batches."""
    d64, d32 = torch_ref(cls, torch.float64, 2, 3), torch_ref(cls, torch.float32, 2, 3)
    run = Run(cls, 3).run(2, lambda s, r, j: micro(s, r, j))
    r_sh, r_t = rel(run.delta(), d64), rel(d32, d64)
    print(f"{SINGLE[cls]} world 3 k=2: {r_sh:.3e}  torch-fp32 {r_t:.3e}  ratio {r_sh / r_t:.3f}")
    assert float(d64.norm()) > 0 and r_sh <= 2.0 * r_t
    assert int(run.opts[0].step_count) == STEPS


@pytest.mark.parametrize("world", [2, 4])
def test_prodigy_d_across_worlds_with_accumulation(world):
    """Equal gradients, k = 2: the shard cuts re-associate the two double sums of the d update, so d agrees to
    rounding: |d_w - d_1| / d_1 below the fp32 restatement's own d error on these gradients (the gate of
    tests/test_zero_prodigy_gpu.py)."""
    (_, dd64), (_, dd32) = prodigy_ref(torch.float64, 1, equal=True), prodigy_ref(torch.float32, 1, equal=True)
    e_ref = abs(dd32 - dd64) / dd64
    d1 = float(world1_equal("FusedProdigy")[-1][0])
    run = Run("FusedProdigy", world).run(2, lambda s, r, j: micro(s, 0, 0, True))
    dw = float(run.opts[0].d)
    print(f"ShardedFusedProdigy world {world} k=2: d {dw:.9e}  world 1 {d1:.9e}  rel {abs(dw - d1) / d1:.3e} "
          f"(the fp32 restatement's d error: {e_ref:.3e})")
    assert d1 > 5 * D0 and abs(dw - d1) / d1 <= e_ref


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


def test_accumulate_and_step_on_rccl_world1(rccl_world1):
    """accumulate() x 2 + step() with the collectives in RCCL: bit-identical to FusedAdamW's, and accumulate() runs
    with torch's synchronisation check set to raise."""
    from videopainter_amd import ShardedFusedAdamW
    from videopainter_amd import distributed as VD
    ref, rps, _ = run_single("FusedAdamW", 3, lambda s, j: micro(s, 0, j), steps=range(2))
    ps, _, allp, _ = make_params()
    opt = ShardedFusedAdamW(allp, lr=LRS[0], **HYP)  # the default process group
    assert isinstance(opt.comm, VD.GroupComm) and opt.world == 1
    for s in range(2):
        opt.param_groups[0]["lr"] = LRS[s]
        for j in range(3):
            set_grads(ps, micro(s, 0, j))
            if j == 2:
                opt.step()
                continue
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                opt.accumulate()
            finally:
                torch.cuda.set_sync_debug_mode("default")
    for p, q in zip(rps, ps):
        assert torch.equal(p.detach(), q.detach())
        at = opt.flat_offset(q)
        assert torch.equal(ref.state[p]["master"].reshape(-1), opt.master_shard[at:at + p.numel()])
    assert int(opt.step_count) == 2 and opt.pending == 0


# ------------------------------------------------------------------------------------------------------------------
# 8: the tiny model, two micro-batches
# ------------------------------------------------------------------------------------------------------------------

def _alphas():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, 0).float()


def test_tiny_model_two_micro_batches():
    """Two micro-batches (other noise and timesteps) through the tiny branch + frozen transformer, forward, loss and
    backward, with accumulate() after the first and step() after the second, the gradients set to None in between.
    The accumulator holds the fp32 mean of the two recorded bf16 gradient sets, element for element, and the masters
    are bit-identical to a second FusedAdamW that is handed the recorded sets through accumulate() / step()."""
    from tests.golden.cases import TINY_CFG, TINY_BRANCH_CFG, tiny_inputs, tiny_weights
    from videopainter_amd import (CogVideoXTransformer3DModel, CogvideoXBranchModel, FusedAdamW, device_scope,
                                  inpainting_v_loss)
    tsd, bsd = tiny_weights()
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**TINY_CFG)
        br = CogvideoXBranchModel(**TINY_BRANCH_CFG)
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    br.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()})
    br.requires_grad_(True)
    i = tiny_inputs()
    b16 = lambda x: x.to(dev, BF16)  # noqa: E731
    ac, mask = _alphas().to(dev), b16(i["mask"])
    g = torch.Generator().manual_seed(8)
    named = list(br.named_parameters())
    start = [p.detach().clone() for _, p in named]
    opt = FusedAdamW([p for _, p in named], lr=1e-5, **HYP)
    recorded = []
    for j in range(2):
        noisy = b16(i["video"] + 0.1 * torch.randn(i["video"].shape, generator=g))
        target = b16(torch.randn(i["video"].shape, generator=g))
        ts = torch.full_like(i["timestep"], 200 + 500 * j).to(dev)
        samples = br(hidden_states=noisy, encoder_hidden_states=b16(i["enc"]), branch_cond=b16(i["branch_cond"]),
                     timestep=ts, image_rotary_emb=i["rope"], return_dict=False)[0]
        out = tr(hidden_states=b16(i["hidden"]), encoder_hidden_states=b16(i["enc"]), timestep=ts,
                 image_rotary_emb=i["rope"], branch_block_samples=samples, branch_block_masks=mask,
                 return_dict=False)[0]
        inpainting_v_loss(out, noisy, target, ts, ac, mask, 1.0).backward()
        recorded.append([None if p.grad is None else p.grad.detach().clone() for _, p in named])
        if j == 0:
            opt.accumulate()
            for _, p in named:
                p.grad = None
        else:
            opt.step()
    has = [x is not None for x in recorded[0]]
    assert any(has) and has == [x is not None for x in recorded[1]]
    assert any(not torch.equal(a, b) for a, b in zip(*recorded) if a is not None)  # other data per micro-batch
    assert opt.pending == 0 and int(opt.step_count) == 1 and int(opt.nonfinite) == 0
    acc = opt.grad_accumulator
    for (_, p), a, b in zip(named, *recorded):
        if a is not None:
            at = opt.flat_offset(p)
            assert torch.equal(acc[at:at + p.numel()], ((a.float() + b.float()) * 0.5).reshape(-1))
    twins = [torch.nn.Parameter(s.clone()) for s in start]
    ref = FusedAdamW(twins, lr=1e-5, **HYP)
    for j in range(2):
        for q, x in zip(twins, recorded[j]):
            q.grad = x
        ref.accumulate() if j == 0 else ref.step()
    moved = 0
    for (n, p), q, h, s in zip(named, twins, has, start):
        if h:
            assert torch.equal(opt.state[p]["master"], ref.state[q]["master"]), n
            assert torch.equal(p.detach(), q.detach()), n
            moved += int(not torch.equal(opt.state[p]["master"], s.float()))
    assert moved > 0
