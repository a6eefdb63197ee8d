"""ShardedFusedAdamW on the GPU (videopainter_amd/zero.py, csrc/zero.hip): the ranks are threads of one process that
talk through distributed.LocalComm, each with its own copies of the parameters on the one device.

Parameter sets (those of tests/test_optim_gpu.py, restated): "main" — bf16 tensors of shapes [1], [7], [3072],
[CHUNK+1], [64, 3072], [3, 5, 7] plus one parameter whose .grad is None (index 2 of the optimizer's list); "small" —
[1], [7] alone, so that at world 4 two ranks own only padding.  Weights N(0, 0.02^2), gradients N(0, 1e-3^2) in bf16,
different per rank, the training script's hyper-parameters, 5 steps with a different lr each.  The FusedAdamW and
world-1 references are computed once per configuration and shared, never modified."""
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
MAX_WORLD = 4


def _shapes(kind):
    from videopainter_amd.optim import CHUNK
    if kind == "small":
        return [(1,), (7,)]
    return [(1,), (7,), (3072,), (CHUNK + 1,), (64, 3072), (3, 5, 7)]


_DATA = {}


def data(kind):
    """(weights[i], grads[step][rank][i]) on the CPU in bf16, generated once per set and never modified."""
    if kind not in _DATA:
        g = torch.Generator().manual_seed(40 if kind == "main" else 41)
        shapes = _shapes(kind)
        w = [(torch.randn(s, generator=g) * 0.02).to(BF16) for s in shapes]
        gr = [[[(torch.randn(s, generator=g) * 1e-3).to(BF16) for s in shapes] for _ in range(MAX_WORLD)]
              for _ in range(STEPS)]
        _DATA[kind] = (w, gr)
    return _DATA[kind]


def make_params(kind):
    """One rank's copies of the set on the device; the main set gets (at index 2) a parameter that never has a
    gradient.  Returns (ps, idle or None, the optimizer's list)."""
    w, _ = data(kind)
    ps = [torch.nn.Parameter(t.to(dev)) for t in w]
    if kind == "small":
        return ps, None, list(ps)
    idle = torch.nn.Parameter(torch.full((5,), 0.25, device=dev, dtype=BF16))
    return ps, idle, ps[:2] + [idle] + ps[2:]


def set_grads(ps, kind, step, rank, persistent=True):
    _, gr = data(kind)
    for p, g in zip(ps, gr[step][rank]):
        if persistent and p.grad is not None:
            p.grad.copy_(g)
        else:
            p.grad = g.to(dev).clone()


def _groups(allp, groups):
    return [dict(params=allp)] if groups is None else [dict(params=allp[:groups]), dict(params=allp[groups:])]


class Run:
    """`world` ShardedFusedAdamW instances over one LocalComm."""

    def __init__(self, kind, world, groups=None, params=None, **kw):
        from videopainter_amd import ShardedFusedAdamW
        from videopainter_amd.distributed import LocalComm
        self.kind, self.world, self.comm = kind, world, LocalComm(world)
        self.ps, self.idle, self.opts = [], [], []
        for r in range(world):
            ps, idle, allp = make_params(kind)
            if params is not None:  # start from given bf16 values (a resumed run)
                with torch.no_grad():
                    for p, v in zip(ps, params):
                        p.copy_(v)
            self.ps.append(ps)
            self.idle.append(idle)
            self.opts.append(ShardedFusedAdamW(_groups(allp, groups), lr=LRS[0], **HYP, comm=self.comm, rank=r, **kw))

    def step_all(self):
        self.comm.run(lambda r: self.opts[r].step())

    def run(self, steps=range(STEPS), lr_scale=(1.0,), same_grads=False, after_step=None):
        for s in steps:
            for r in range(self.world):
                for grp, sc in zip(self.opts[r].param_groups, lr_scale):
                    grp["lr"] = LRS[s] * sc
                set_grads(self.ps[r], self.kind, s, 0 if same_grads else r)
            self.step_all()
            if after_step is not None:
                after_step(self, s)
        return self

    def flat(self, name):
        """The state `name` of all ranks assembled in flat order (the padded tail cut off)."""
        return torch.cat([getattr(o, name + "_shard") for o in self.opts])[:self.opts[0].total]

    def snapshot(self):
        return [self.flat("master"), self.flat("exp_avg"), self.flat("exp_avg_sq")] + \
            [p.detach().clone() for p in self.ps[0]]


def run_fused(kind, steps=range(STEPS), groups=None, lr_scale=(1.0,), opt=None, ps=None, **kw):
    """FusedAdamW on rank 0's gradients; returns (opt, ps)."""
    from videopainter_amd import FusedAdamW
    if opt is None:
        ps, _, allp = make_params(kind)
        opt = FusedAdamW(_groups(allp, groups), lr=LRS[0], **HYP, **kw)
    for s in steps:
        for grp, sc in zip(opt.param_groups, lr_scale):
            grp["lr"] = LRS[s] * sc
        set_grads(ps, kind, s, 0)
        opt.step()
    return opt, ps


def fused_snapshot(opt, ps):
    """FusedAdamW's state laid out as the sharded optimizer's flat space (every trainable parameter in list order,
    padded with zeros to a multiple of 8 elements), from its public per-parameter state, then the bf16 parameters."""
    allp = [p for g in opt.param_groups for p in g["params"] if p.requires_grad]
    flat = []
    for k in ("master", "exp_avg", "exp_avg_sq"):
        parts = []
        for p in allp:
            t = opt.state[p][k].reshape(-1)
            parts += [t, t.new_zeros((-t.numel()) % 8)]
        flat.append(torch.cat(parts))
    return flat + [p.detach().clone() for p in ps]


_REF = {}


def fused_ref(kind, max_norm=None, steps=STEPS):
    """Snapshot + (grad_norm, clip_coef) of FusedAdamW after `steps` steps of rank 0's gradients (computed once)."""
    key = ("fused", kind, max_norm, steps)
    if key not in _REF:
        opt, ps = run_fused(kind, steps=range(steps), max_grad_norm=max_norm)
        _REF[key] = (fused_snapshot(opt, ps), float(opt.grad_norm), float(opt.clip_coef))
    return _REF[key]


def world1_ref(kind):
    """Snapshot of an uninterrupted world-1 sharded run, same gradients, no clip (computed once)."""
    key = ("world1", kind)
    if key not in _REF:
        _REF[key] = Run(kind, 1).run(same_grads=True).snapshot()
    return _REF[key]


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
                                    for x, y in zip(a, b))


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def replicas_agree(run, s=None):
    """bf16 parameters and the whole scalars block bit-equal on every rank."""
    for r in range(1, run.world):
        assert torch.equal(run.opts[r].scalars, run.opts[0].scalars), (s, r)
        for p, q in zip(run.ps[r], run.ps[0]):
            assert torch.equal(p.detach(), q.detach()), (s, r, tuple(p.shape))


# ------------------------------------------------------------------------------------------------------------------
# 1: world 1 equals FusedAdamW
# ------------------------------------------------------------------------------------------------------------------

def test_world1_is_bit_identical_to_fused_adamw():
    ref, _, _ = fused_ref("main")
    run = Run("main", 1).run(same_grads=True)
    assert same(run.snapshot(), ref)
    assert int(run.opts[0].step_count) == STEPS and int(run.opts[0].last_step_skipped) == 0
    assert float(run.opts[0].clip_coef) == 1.0
    w, _ = data("main")
    assert any(not torch.equal(p.detach().cpu(), t) for p, t in zip(run.ps[0], w))  # (bf16 values did move)
    assert same(run.snapshot(), world1_ref("main"))  # run to run


@pytest.mark.parametrize("max_norm", [1.0, 0.1])
def test_world1_norm_and_clip_match_fused_adamw(max_norm):
    """The shard sums its ranges, FusedAdamW its chunks of bf16 values: another summation order, so 1e-5 rather than
    bit identity (n non-negative fp32 terms in a fixed-order tree: <= log2(n) 2^-24 ~ 2e-6)."""
    _, gn, cc = fused_ref("main", max_norm)
    run = Run("main", 1, max_grad_norm=max_norm).run(same_grads=True)
    o = run.opts[0]
    print(f"world 1 clip {max_norm}: norm {float(o.grad_norm):.9g} (fused {gn:.9g}) coef {float(o.clip_coef):.9g} "
          f"(fused {cc:.9g})")
    assert abs(float(o.grad_norm) - gn) <= 1e-5 * gn
    assert abs(float(o.clip_coef) - cc) <= 1e-5
    assert (cc < 1.0) == (max_norm == 0.1)
    ref, _, _ = fused_ref("main", max_norm)
    # the same update up to the coefficient's last bits: fp32 masters an ulp or two apart (2^-24 ~ 6e-8 each)
    assert rel(run.flat("master"), ref[0]) < 1e-6


# ------------------------------------------------------------------------------------------------------------------
# 2: sharding invariance
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharding_invariance(world):
    """Every rank has the same gradients, no clip.  1 / P and the P-term sum are exact for P = 2, 4: bit-identical to
    world 1.  P = 3 rounds (g / 3 three times is not g), so there only the ranks agree among themselves."""
    run = Run("main", world).run(same_grads=True, after_step=replicas_agree)
    if world == 3:  # (and close to world 1: gradients an ulp off move fp32 masters by an ulp or two, ~6e-8 each)
        assert rel(run.flat("master"), world1_ref("main")[0]) < 1e-6
    else:
        assert same(run.snapshot(), world1_ref("main"))
        for r in range(world):
            assert same([p.detach() for p in run.ps[r]], world1_ref("main")[3:])


# ------------------------------------------------------------------------------------------------------------------
# 3, 4: update parity with torch.optim.AdamW on the mean gradient; the replicas agree after every step
# ------------------------------------------------------------------------------------------------------------------

PARITY = {
    "script": dict(max_norm=1.0),
    "clip_active": dict(max_norm=0.1),  # the averaged gradient's norm is below 0.47: the coefficient is active
    "two_groups": dict(max_norm=1.0, groups=4, lr_scale=(1.0, 0.3)),
    "no_clip": dict(max_norm=None),
}


def torch_ref(world, dtype, max_norm, groups=None, lr_scale=(1.0,)):
    """torch.optim.AdamW + clip_grad_norm_ on `dtype` copies (CPU), stepped on the mean of the ranks' gradients taken
    in `dtype`; returns (master - initial, the norm of the last step's mean gradient)."""
    key = ("torch", world, dtype, max_norm, groups, lr_scale)
    if key in _REF:
        return _REF[key]
    w, gr = data("main")
    ps = [torch.nn.Parameter(t.to(dtype)) for t in w]
    if groups is None:
        pg = [dict(params=ps)]
    else:  # (the idle parameter sits at index 2 of the sharded run's list)
        k = groups - 1 if groups > 2 else groups
        pg = [dict(params=ps[:k]), dict(params=ps[k:])]
    opt = torch.optim.AdamW(pg, lr=LRS[0], betas=HYP["betas"], eps=HYP["eps"], weight_decay=HYP["weight_decay"])
    norm = 0.0
    for s in range(STEPS):
        for grp, sc in zip(opt.param_groups, lr_scale):
            grp["lr"] = LRS[s] * sc
        for i, p in enumerate(ps):
            p.grad = sum(gr[s][r][i].to(dtype) for r in range(world)) / world
        norm = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    d = torch.cat([(p.detach().double() - t.double()).reshape(-1) for p, t in zip(ps, w)])
    _REF[key] = (d, norm)
    return _REF[key]


def sharded_delta(run):
    """master - initial over the set's tensors (padding and the idle parameter left out), assembled from the shards."""
    w, _ = data(run.kind)
    m = run.flat("master").double().cpu()
    off = run.opts[0].flat_offset
    return torch.cat([m[off(p):off(p) + t.numel()] - t.double().reshape(-1) for p, t in zip(run.ps[0], w)])


@pytest.mark.parametrize("case", list(PARITY))
@pytest.mark.parametrize("world", [2, 3, 4])
def test_update_parity(world, case):
    """D = master after 5 steps - initial, assembled from the shards.  Gate (tests/test_optim_gpu.py's form):
    rel-L2(D, D_fp64) <= 2 x rel-L2(D_torch_fp32, D_fp64); both torch references step on the mean of the ranks'
    gradients taken in their own dtype.  The norm of the averaged gradient is within 1e-5 of the fp64 one.  After
    every step the bf16 parameters and the scalars block are bit-equal on all ranks.  (DESIGN.md §5 has the figures.)"""
    c = dict(PARITY[case])
    max_norm = c.pop("max_norm")
    d64, n64 = torch_ref(world, torch.float64, max_norm, c.get("groups"), c.get("lr_scale", (1.0,)))
    d32, _ = torch_ref(world, torch.float32, max_norm, c.get("groups"), c.get("lr_scale", (1.0,)))
    run = Run("main", world, groups=c.get("groups"), max_grad_norm=max_norm)
    run.run(lr_scale=c.get("lr_scale", (1.0,)), after_step=replicas_agree)
    df = sharded_delta(run)
    r_sh, r_t = rel(df, d64), rel(d32, d64)
    o = run.opts[0]
    e_n = abs(float(o.grad_norm) - n64) / n64
    print(f"parity[world {world}, {case}] sharded {r_sh:.3e}  torch-fp32 {r_t:.3e}  ratio {r_sh / r_t:.3f}  "
          f"norm {float(o.grad_norm):.9g} vs fp64 {n64:.9g}: rel {e_n:.2e}")
    assert torch.isfinite(df).all() and float(d64.norm()) > 0
    assert r_sh <= 2.0 * r_t
    assert e_n <= 1e-5
    if max_norm is not None:
        assert abs(float(o.clip_coef) - min(1.0, max_norm / (n64 + 1e-6))) <= 1e-5
    assert int(o.step_count) == STEPS and int(o.last_step_skipped) == 0
    for r in range(world):  # bf16 write-back on every rank: the parameters are bf16(master)
        m16 = run.flat("master").to(BF16)
        flat16 = run.opts[r].param_staging[:m16.numel()]
        for p0, p in zip(run.ps[0], run.ps[r]):
            o0 = run.opts[0].flat_offset(p0)
            assert torch.equal(p.detach().reshape(-1), m16[o0:o0 + p.numel()])
            assert torch.equal(flat16[o0:o0 + p.numel()], m16[o0:o0 + p.numel()])


def test_replicas_agree_and_idle_parameter_untouched():
    seen = []

    def check(run, s):
        replicas_agree(run, s)
        for r in range(run.world):
            idle, o = run.idle[r], run.opts[r]
            assert idle.grad is None and torch.equal(idle.detach(), torch.full((5,), 0.25, device=dev, dtype=BF16))
            assert len(o.state) == 0  # no per-parameter state grows: the state is the three flat shards
        off = run.opts[0].flat_offset(run.idle[0])
        assert torch.equal(run.flat("master")[off:off + 8], torch.tensor([0.25] * 5 + [0.0] * 3, device=dev))
        assert not run.flat("exp_avg")[off:off + 8].any() and not run.flat("exp_avg_sq")[off:off + 8].any()
        assert not run.opts[0].grad_staging[off:off + 8].any()  # its gradient region: zeros
        seen.append(s)

    run = Run("main", 3, max_grad_norm=1.0).run(after_step=check)
    assert seen == list(range(STEPS))
    per, total = run.opts[0].per, run.opts[0].total
    for name in ("master", "exp_avg", "exp_avg_sq"):  # padding is zero and stays zero
        full = torch.cat([getattr(o, name + "_shard") for o in run.opts])
        assert full.numel() == 3 * per and not full[total:].any()
    _, gr = data("main")
    for r in range(3):  # the gradients are left as they were (the clip is folded into the update)
        assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(run.ps[r], gr[STEPS - 1][r]))


# ------------------------------------------------------------------------------------------------------------------
# 5: ranks that own only padding
# ------------------------------------------------------------------------------------------------------------------

def test_padding_only_ranks():
    run4 = Run("small", 4, max_grad_norm=None).run(same_grads=True, after_step=replicas_agree)
    assert run4.opts[0].per == 8 and run4.opts[0].total == 16
    assert same(run4.snapshot(), world1_ref("small"))
    assert same(run4.snapshot(), fused_ref("small")[0])
    for r in (2, 3):
        o = run4.opts[r]
        assert o.n_ranges == 0
        assert not o.master_shard.any() and not o.exp_avg_shard.any() and not o.exp_avg_sq_shard.any()
        assert int(o.step_count) == STEPS
    assert run4.opts[0].n_ranges == 1 and run4.opts[1].n_ranges == 1


# ------------------------------------------------------------------------------------------------------------------
# 6: a non-finite value on one rank
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["other_shard", "own_shard"])
def test_nonfinite_on_one_rank_skips_every_rank(where):
    """One +inf in rank 1's gradient: in tensor [3072] (flat offset 24, rank 0's shard) or in [3, 5, 7] (the end of the
    flat space, rank 1's own shard).  A value check only."""
    run = Run("main", 2, max_grad_norm=1.0, skip_nonfinite=True, zero_grads=True)
    run.run(steps=range(2))
    o0 = run.opts[0]
    ti = 2 if where == "other_shard" else 5
    off = o0.flat_offset(run.ps[0][ti])
    assert (off + run.ps[0][ti].numel() <= o0.per) if where == "other_shard" else (off >= o0.per)
    before = run.snapshot() + [p.detach().clone() for p in run.ps[1]]
    for r in range(2):
        set_grads(run.ps[r], "main", 2, r)
    run.ps[1][ti].grad.view(-1)[17] = float("inf")
    run.step_all()
    assert same(run.snapshot() + [p.detach().clone() for p in run.ps[1]], before)
    for r in range(2):
        o = run.opts[r]
        assert int(o.last_step_skipped) == 1 and int(o.nonfinite) == 1 and int(o.step_count) == 2
        assert all(not p.grad.any() for p in run.ps[r])  # zero_grads: zeroed all the same
    replicas_agree(run)
    run.run(steps=[2])  # and the next good step is taken
    assert all(int(o.step_count) == 3 and int(o.last_step_skipped) == 0 and int(o.nonfinite) == 0 for o in run.opts)
    ref = Run("main", 2, max_grad_norm=1.0, skip_nonfinite=True, zero_grads=True).run(steps=range(3))
    assert same(run.snapshot(), ref.snapshot())


# ------------------------------------------------------------------------------------------------------------------
# 7: checkpoints move between world sizes and FusedAdamW
# ------------------------------------------------------------------------------------------------------------------

def test_checkpoint_interchange():
    from videopainter_amd import FusedAdamW
    a = Run("main", 2).run(steps=range(2), same_grads=True)
    full = a.comm.run(lambda r: a.opts[r].full_state_dict())
    sd = full[0]
    assert sd["step"] == 2 and sorted(sd) == ["param_groups", "state", "step"]
    for k in ("master", "exp_avg", "exp_avg_sq"):  # every rank assembles the same full state
        assert all(torch.equal(full[1]["state"][i][k], sd["state"][i][k]) for i in sd["state"])
    values = [p.detach().clone() for p in a.ps[0]]
    # into world 4
    b = Run("main", 4, params=values)
    for o in b.opts:
        o.load_state_dict(sd)
        assert int(o.step_count) == 2
    b.run(steps=range(2, STEPS), same_grads=True)
    assert same(b.snapshot(), world1_ref("main"))
    # into FusedAdamW (its own format: state[i] = per-parameter tensors of the parameter's shape)
    ps, _, allp = make_params("main")
    with torch.no_grad():
        for p, v in zip(ps, values):
            p.copy_(v)
    f = FusedAdamW(allp, lr=0.5, betas=(0.5, 0.5))
    f.load_state_dict(sd)
    assert f.param_groups[0]["betas"] == HYP["betas"] and int(f.step_count) == 2
    run_fused("main", steps=range(2, STEPS), opt=f, ps=ps)
    assert same(fused_snapshot(f, ps), world1_ref("main"))
    # and FusedAdamW's own state dict loads into a sharded optimizer
    g2, gps = run_fused("main", steps=range(2))
    c = Run("main", 3, params=[p.detach() for p in gps])
    for o in c.opts:
        o.load_state_dict(g2.state_dict())
    assert same(c.snapshot(), a.snapshot())
    # a local state dict reloads into the same world bit for bit
    local = [o.state_dict() for o in a.opts]
    assert local[1]["world"] == 2 and local[1]["rank"] == 1 and local[1]["per"] == a.opts[1].per
    d = Run("main", 2, params=values)
    for o, s in zip(d.opts, local):
        o.load_state_dict(s)
    assert same(d.snapshot(), a.snapshot()) and all(int(o.step_count) == 2 for o in d.opts)
    d.run(steps=range(2, STEPS), same_grads=True)
    assert same(d.snapshot(), world1_ref("main"))
    with pytest.raises(ValueError):
        d.opts[0].load_state_dict(local[1])  # another rank's shard


# ------------------------------------------------------------------------------------------------------------------
# 8: unaligned views, gradients reallocated every step
# ------------------------------------------------------------------------------------------------------------------

def test_unaligned_views_take_the_scalar_paths():
    """Parameters / gradients that are slices at odd element offsets run the scalar head / whole-chunk scalar paths of
    pack and unpack: bit-identical to FusedAdamW on aligned tensors, and nothing outside the views is written.
    Offsets (4, 4) give pack a head of 4 elements before its vector body (the fp32 staging can follow that phase);
    sizes below 8, 9 and CHUNK + 1 give pieces (chunks and ranges) of fewer elements than one vector, a vector with a
    one-element tail, and a second piece of one element."""
    from videopainter_amd import FusedAdamW, ShardedFusedAdamW
    from videopainter_amd.distributed import LocalComm
    from videopainter_amd.optim import CHUNK
    g = torch.Generator().manual_seed(5)
    for n in (CHUNK + 37, CHUNK + 1, 9, 7, 1):
        w = (torch.randn(n, generator=g) * 0.02).to(BF16).to(dev)
        gr = (torch.randn(n, generator=g) * 1e-3).to(BF16).to(dev)
        p0 = torch.nn.Parameter(w.clone())
        p0.grad = gr.clone()
        ref = FusedAdamW([p0], lr=1e-5, **HYP)
        ref.step()
        for po, go in ((0, 0), (3, 3), (3, 5), (1, 0), (4, 4)):
            pbuf = torch.zeros(n + 16, device=dev, dtype=BF16)
            gbuf = torch.zeros(n + 16, device=dev, dtype=BF16)
            p = torch.nn.Parameter(pbuf[po:po + n])
            p.data.copy_(w)
            p.grad = gbuf[go:go + n]
            p.grad.copy_(gr)
            opt = ShardedFusedAdamW([p], lr=1e-5, **HYP, comm=LocalComm(1), rank=0, zero_grads=(go >= 4))
            opt.step()
            assert torch.equal(p.detach(), p0.detach()), (n, po, go)
            st = ref.state[p0]
            assert torch.equal(opt.master_shard[:n], st["master"])
            assert torch.equal(opt.exp_avg_shard[:n], st["exp_avg"])
            assert torch.equal(opt.exp_avg_sq_shard[:n], st["exp_avg_sq"])
            assert not pbuf[:po].any() and not pbuf[po + n:].any() and not gbuf[:go].any() and not gbuf[go + n:].any()
            assert torch.equal(p.grad, torch.zeros_like(gr) if go >= 4 else gr)
        assert not torch.equal(ref.state[p0]["master"], w.float())


def test_reallocated_gradients():
    """Step 1 with persistent .grad tensors, step 2 after p.grad = None and fresh tensors at other addresses (the
    table re-upload), then a step where another subset has gradients (the range table is rebuilt)."""
    ref, _, _ = fused_ref("main", None, steps=2)
    run = Run("main", 2).run(steps=range(1), same_grads=True)
    old = [[p.grad for p in ps] for ps in run.ps]
    for r in range(2):
        for p in run.ps[r]:
            p.grad = None
        for grp in run.opts[r].param_groups:
            grp["lr"] = LRS[1]
        set_grads(run.ps[r], "main", 1, 0, persistent=False)
        assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(run.ps[r], old[r]))
    run.step_all()
    assert same(run.snapshot(), ref)
    for r in range(2):
        run.ps[r][0].grad = None
    before = run.snapshot()
    run.step_all()
    after = run.snapshot()
    off = run.opts[0].flat_offset(run.ps[0][1])
    assert all(torch.equal(x[:off], y[:off]) for x, y in zip(before[:3], after[:3]))  # tensor 0: untouched
    assert torch.equal(after[3], before[3]) and not torch.equal(after[0][off:], before[0][off:])
    replicas_agree(run)


# ------------------------------------------------------------------------------------------------------------------
# 9: the whole step through RCCL at world size 1
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
    """The reduce-scatter and both all-gathers run in RCCL on the device buffers (no host hop); the result is
    bit-identical to FusedAdamW; a step runs with torch's synchronisation check set to raise."""
    from videopainter_amd import ShardedFusedAdamW
    from videopainter_amd import distributed as VD
    ref, _, _ = fused_ref("main")
    ps, idle, allp = make_params("main")
    opt = ShardedFusedAdamW(allp, lr=LRS[0], **HYP)  # the default process group
    assert isinstance(opt.comm, VD.GroupComm) and (opt.world, opt.rank) == (1, 0)
    assert VD._staged(opt.grad_staging).host is False and VD._staged(opt.param_staging).host is False
    for s in range(STEPS):
        opt.param_groups[0]["lr"] = LRS[s]
        set_grads(ps, "main", s, 0)
        opt.step()
    n = opt.total
    got = [opt.master_shard[:n], opt.exp_avg_shard[:n], opt.exp_avg_sq_shard[:n]] + [p.detach() for p in ps]
    assert same(got, ref)
    fresh = [p.grad.clone() for p in ps]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        for p, g in zip(ps, fresh):  # reallocated gradients: the table upload
            p.grad = g
        opt.step()
        states = (opt.grad_norm, opt.clip_coef, opt.last_step_skipped, opt.step_count, opt.nonfinite)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in states) and int(opt.step_count) == STEPS + 2
    sd = opt.full_state_dict()  # (collective; world 1)
    assert sd["step"] == STEPS + 2 and torch.equal(sd["state"][0]["master"].reshape(-1), opt.master_shard[:1])


# ------------------------------------------------------------------------------------------------------------------
# 10: one step of the tiny model on two ranks
# ------------------------------------------------------------------------------------------------------------------

def _alphas():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, 0).float()


def test_tiny_model_step_two_ranks():
    """Two copies of the tiny branch (one frozen transformer); forward, loss and backward serially in the main thread
    with different noise and timesteps per rank; then step() on both through the communicator.  The branch parameters
    are bit-equal across the ranks afterwards, and D = master - initial passes test 3's gate against
    torch.optim.AdamW (no clip) in float64 / float32 stepped on the mean of the two recorded gradient sets, taken in
    float64 / float32 (no bf16 rounding of the mean)."""
    from tests.golden.cases import TINY_CFG, TINY_BRANCH_CFG, tiny_inputs, tiny_weights
    from videopainter_amd import (CogVideoXTransformer3DModel, CogvideoXBranchModel, ShardedFusedAdamW, device_scope,
                                  inpainting_v_loss)
    from videopainter_amd.distributed import LocalComm
    tsd, bsd = tiny_weights()
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**TINY_CFG)
        brs = [CogvideoXBranchModel(**TINY_BRANCH_CFG) for _ in range(2)]
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    for br in brs:
        br.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()})
        br.requires_grad_(True)
    i = tiny_inputs()
    b16 = lambda x: x.to(dev, BF16)  # noqa: E731
    ac, mask = _alphas().to(dev), b16(i["mask"])
    g = torch.Generator().manual_seed(8)
    comm = LocalComm(2)
    named = [list(br.named_parameters()) for br in brs]
    opts = [ShardedFusedAdamW([p for _, p in named[r]], lr=1e-5, **HYP, comm=comm, rank=r) for r in range(2)]
    start = [p.detach().clone() for _, p in named[0]]
    for r, br in enumerate(brs):
        noisy = b16(i["video"] + 0.1 * torch.randn(i["video"].shape, generator=g))
        target = b16(torch.randn(i["video"].shape, generator=g))
        ts = torch.full_like(i["timestep"], 200 + 500 * r).to(dev)
        samples = br(hidden_states=noisy, encoder_hidden_states=b16(i["enc"]), branch_cond=b16(i["branch_cond"]),
                     timestep=ts, image_rotary_emb=i["rope"], return_dict=False)[0]
        out = tr(hidden_states=b16(i["hidden"]), encoder_hidden_states=b16(i["enc"]), timestep=ts,
                 image_rotary_emb=i["rope"], branch_block_samples=samples, branch_block_masks=mask,
                 return_dict=False)[0]
        inpainting_v_loss(out, noisy, target, ts, ac, mask, 1.0).backward()
    has = [p.grad is not None for _, p in named[0]]
    assert any(has) and has == [p.grad is not None for _, p in named[1]]  # the caller's contract
    grads = [[p.grad.detach().clone().cpu() for _, p in nm if p.grad is not None] for nm in named]
    assert any(not torch.equal(a, b) for a, b in zip(*grads))  # the ranks did see different data
    comm.run(lambda r: opts[r].step())
    for (n0, p0), (n1, p1) in zip(*named):
        assert n0 == n1 and torch.equal(p0.detach(), p1.detach()), n0
    assert torch.equal(opts[0].scalars, opts[1].scalars) and int(opts[0].nonfinite) == 0
    assert int(opts[0].step_count) == 1
    master = torch.cat([o.master_shard for o in opts]).double().cpu()
    trained = [(p, s) for (_, p), s, h in zip(named[0], start, has) if h]
    d = torch.cat([master[opts[0].flat_offset(p):opts[0].flat_offset(p) + p.numel()] - s.double().cpu().reshape(-1)
                   for p, s in trained])
    moved = sum(int(not torch.equal(p.detach(), s)) for p, s in trained)

    def ref(dtype):
        ps = [torch.nn.Parameter(s.cpu().to(dtype)) for _, s in trained]
        opt = torch.optim.AdamW(ps, lr=1e-5, **HYP)
        for p, a, b in zip(ps, *grads):
            p.grad = (a.to(dtype) + b.to(dtype)) / 2
        opt.step()
        return torch.cat([(p.detach().double() - s.double().cpu()).reshape(-1) for p, (_, s) in zip(ps, trained)])

    d64, d32 = ref(torch.float64), ref(torch.float32)
    r_sh, r_t = rel(d, d64), rel(d32, d64)
    print(f"tiny model, 2 ranks: sharded {r_sh:.3e}  torch-fp32 {r_t:.3e}  ({moved} of {len(trained)} bf16 tensors "
          f"moved)")
    assert torch.isfinite(d).all() and float(d64.norm()) > 0
    assert r_sh <= 2.0 * r_t
    for p, _ in trained:  # the bf16 write-back
        o = opts[0].flat_offset(p)
        assert torch.equal(p.detach().reshape(-1).cpu(), master[o:o + p.numel()].float().to(BF16))
