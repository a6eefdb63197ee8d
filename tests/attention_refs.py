"""Plain-torch CPU float64 references of the flash-attention backward (csrc/attention_bwd.hip), written from the
formulas above vp_attn_bwd_desc in include/vp_hip.h, and the cases the attention-backward tests run.

With c = scale * log2 e, on exactly the tensors the kernel is handed (bf16 q, k, v, o, dO; fp32 lse in log2 units):
    P = exp2(c q.k - lse),  dP = dO . V^T,  D = rowsum(dO * O),  dS = P * (dP - D)
    dQ = scale * dS . K,    dK = scale * dS^T . Q,    dV = P^T . dO
`spec` is that, `rounded` the same with the kernel's documented roundings put in (two ways: the dQ kernel's and the
dK / dV kernel's), `mag` the same with absolute values (the size of the terms an fp32 evaluation cancels), `forward`
the o and lse the tests hand to the kernel.  No autograd, and nothing here imports the package under test;
tests/test_attention_refs_cpu.py checks `spec` against float64 autograd.

The gate (per head row r = the 64-vector of one (b, n, h), for each of dq, dk, dv):
    |got_r - spec_r|_2  <=  C * max(model_r, 2^-9 |spec_r|_2)  +  2^-16 |mag_r|_2
model_r: the larger |rounded_r - spec_r|_2 of the two sides; 2^-9: the half-ulp of the bf16 output; 2^-16: each of
the two 64-term fp32 dot products behind dP - D carries at most 64 * 2^-24 of its absolute sum.  C = C_GATE[group] is
measured on the references alone (below).  delta per element: |got - D| <= 2^-17 * sum |dO_i O_i|.

The cases (shapes, seeds, input builders) are at the end: the CPU test file and the GPU test file run the same ones.
"""
import functools
import math
from types import SimpleNamespace

import torch

from tests.backward_refs import rnd_bf16

F64 = torch.float64
BF = torch.bfloat16
LOG2E = 1.4426950408889634
U9 = 2.0 ** -9     # half an ulp of the bf16 output, relative
U16 = 2.0 ** -16   # two 64-term fp32 dot products: 64 * 2^-24 each, times |terms|
U17 = 2.0 ** -17   # delta: one 64-term fp32 FMA chain, times two

# C_GATE: how far two independent realisations of the same rounding budget lie apart.  Measured, not chosen:
# tests/test_attention_refs_cpu.py::test_c_gate takes, over every head row of dq, dk and dv of the cases below, the
# worst ratio between the two sides' gate terms max(|rounded_r - spec_r|_2, 2^-9 |spec_r|_2), doubles it and rounds
# up to an integer, at least 3.  Rows in which neither side reaches the 2^-9 floor, or the fp32 term, are left out:
# there the gate rests on a term without the model in it.  That test repeats the measurement and fails if it does
# not give these numbers.
# The ratio of two independent error norms has a heavy tail wherever the rounding of the scores operand outweighs
# the output's rounding (few effective keys, large gains): its worst value grows with the gains and with the number
# of rows.  One constant for all cases would be the score_range cases' and would leave the ordinary cases a gate
# of 2^-9 x that; so each group of cases has its own, by the same rule from its own rows, none wider than the one
# constant (their maximum) would be.  Worst ratios measured: lengths 9.080, strides 5.232, scale 8.382,
# score_range/peak 26.701, score_range/spread 91.239, extra_mass 3.786, k_len 6.991, tail_split 9.232.
# Where C is large the gate has little power over dq in peaked rows: where one key holds 0.9992 of a row, Sum_j dS_j = 0
# makes that key's dS what the others leave, the scores operand's rounding moves those by percents, and 54 x that
# model error covers even a second copy of the key.  Such cases carry rows whose scores stay small for what the
# peaked rows cannot show (the soft rows of score_range/peak_partial).
C_GATE = {"lengths": 19, "strides": 11, "scale": 17, "score_range/peak": 54, "score_range/spread": 183,
          "extra_mass": 8, "k_len": 14, "tail_split": 19}


def f32(x):
    """the value a C float argument takes"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def heads(t, H):
    """[B, N, H*64] (any dtype / strides) -> float64 [B, H, N, 64]"""
    t = t.detach().cpu().to(F64)
    return t.reshape(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def unheads(t):
    """[B, H, N, 64] -> [B, N, H*64]"""
    B, H, N, _ = t.shape
    return t.transpose(1, 2).reshape(B, N, H * 64)


def lengths(k_len, B, Nk):
    """min(max(k_len[b], 0), Nk) per batch row (Nk without k_len)"""
    if k_len is None:
        return [Nk] * B
    return [min(max(int(x), 0), Nk) for x in k_len]


MUTANTS = ("drop_last", "one_more", "neighbour_stats", "scale_dq", "scale_dk", "scale_c", "d_exact_o")


def _evaluate(q, k, v, o, do, lse, H, scale, k_len=None, side=None, mag=False, mutant=None, o_exact=None):
    """the header's formulas, one batch row at a time over the valid keys only (K / V rows at or past the length are
    never touched: they may hold NaN).  side "q" / "k": the kernels' roundings; mag: absolute values; mutant: one of
    MUTANTS, a deliberately wrong evaluation (tests/test_attention_refs_cpu.py: the gate must see it)."""
    assert not (mag and side) and mutant in (None,) + MUTANTS
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    scale = f32(scale)
    s_c = 0.125 if mutant == "scale_c" else scale
    s_dq = 0.125 if mutant == "scale_dq" else scale
    s_dk = 0.125 if mutant == "scale_dk" else scale
    c = s_c * LOG2E
    Q, K, V, G = heads(q, H), heads(k, H), heads(v, H), heads(do, H)
    O = heads(o, H) if not (mutant == "d_exact_o") else o_exact.detach().cpu().to(F64)
    lse = lse.detach().cpu().to(F64)
    rnd = rnd_bf16 if side else (lambda x: x)
    dq = torch.zeros(B, H, Nq, 64, dtype=F64)
    dk = torch.zeros(B, H, Nk, 64, dtype=F64)
    dv = torch.zeros(B, H, Nk, 64, dtype=F64)
    delta = torch.zeros(B, H, Nq, dtype=F64)
    for b, L in enumerate(lengths(k_len, B, Nk)):
        if mutant == "drop_last":
            L = max(L - 1, 0)
        kb, vb = K[b, :, :L], V[b, :, :L]
        if mutant == "one_more":  # the key at the length; past the buffer: the clamped last row, as a tile stages it
            e = min(L, Nk - 1)
            kb, vb = torch.cat([kb, K[b, :, e:e + 1]], 1), torch.cat([vb, V[b, :, e:e + 1]], 1)
        qb, gb, ob, lb = Q[b], G[b], O[b], lse[b]
        D = (gb * ob).sum(-1)
        if mag:
            Dm = (gb * ob).abs().sum(-1)
            delta[b] = Dm
        else:
            delta[b] = D
        if side:
            D = D.to(torch.float32).to(F64)
        if mutant == "neighbour_stats" and Nq >= 64:
            r = torch.arange(63, Nq, 64)
            lb, D = lb.clone(), D.clone()
            lb[:, r], D[:, r] = lb[:, r - 1], D[:, r - 1]
        if side == "q":
            s = rnd(c * qb) @ kb.transpose(-1, -2)
        elif side == "k":
            s = qb @ rnd(c * kb).transpose(-1, -2)
        else:
            s = c * (qb @ kb.transpose(-1, -2))
        P = torch.exp2(s - lb[..., None])
        if mag:
            dS = P * (gb.abs() @ vb.abs().transpose(-1, -2) + Dm[..., None])
            qb, kb, gb = qb.abs(), kb.abs(), gb.abs()
        else:
            dS = rnd(P * (gb @ vb.transpose(-1, -2) - D[..., None]))
        n = min(kb.shape[1], Nk)
        dq[b] = s_dq * (dS @ kb)
        dk[b, :, :n] = (s_dk * (dS.transpose(-1, -2) @ qb))[:, :n]
        dv[b, :, :n] = (rnd(P).transpose(-1, -2) @ gb)[:, :n]
    out = SimpleNamespace(dq=unheads(dq), dk=unheads(dk), dv=unheads(dv), delta=delta)
    if side:
        out.dq, out.dk, out.dv = rnd_bf16(out.dq), rnd_bf16(out.dk), rnd_bf16(out.dv)
    return out


def spec(q, k, v, o, do, lse, H, scale, k_len=None):
    """dq, dk, dv [B, N, H*64] and delta [B, H, Nq] in float64, unrounded"""
    return _evaluate(q, k, v, o, do, lse, H, scale, k_len)


def rounded(q, k, v, o, do, lse, H, scale, k_len=None, side="q"):
    """`spec` with the kernel's roundings: the scores operand bf16(c q) (side "q", the dQ kernel) or bf16(c k) (side
    "k", the dK / dV kernel); bf16(P) into dV; bf16(P (dP - D)) into dQ and dK; D in fp32; the outputs in bf16"""
    assert side in ("q", "k")
    return _evaluate(q, k, v, o, do, lse, H, scale, k_len, side=side)


def mag(q, k, v, o, do, lse, H, scale, k_len=None):
    """`spec` on absolute values: P as it is, |dP| + |D| for dP - D; delta = sum |dO_i O_i|"""
    return _evaluate(q, k, v, o, do, lse, H, scale, k_len, mag=True)


def mutant(name, q, k, v, o, do, lse, H, scale, k_len=None, o_exact=None):
    return _evaluate(q, k, v, o, do, lse, H, scale, k_len, mutant=name, o_exact=o_exact)


def forward(q, k, v, H, scale, k_len=None, extra=None, exact=False):
    """o [B, H, Nq, 64] and lse [B, H, Nq] (log2 units of c q.k) of softmax attention over the valid keys, in float64;
    extra [B, H, Nq]: log2 of more row mass than the keys give (the closed-form null keys' l_extra: lse includes it, o
    does not sum to one row of V).  Unless `exact`, o carries the bf16 rounding and lse the fp32 rounding of what the
    kernel is handed."""
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    c = f32(scale) * LOG2E
    Q, K, V = heads(q, H), heads(k, H), heads(v, H)
    o = torch.zeros(B, H, Nq, 64, dtype=F64)
    lse = torch.full((B, H, Nq), -math.inf, dtype=F64)
    for b, L in enumerate(lengths(k_len, B, Nk)):
        if L == 0 and extra is None:
            continue
        s = c * (Q[b] @ K[b, :, :L].transpose(-1, -2))
        if extra is not None:
            s = torch.cat([s, extra[b].to(F64)[..., None]], -1)
        m = s.max(-1).values
        lse[b] = m + torch.log2(torch.exp2(s - m[..., None]).sum(-1))
        o[b] = torch.exp2(s[..., :L] - lse[b][..., None]) @ V[b, :, :L]
    if not exact:
        o, lse = rnd_bf16(o), lse.to(torch.float32).to(F64)
    return o, lse


# ------------------------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------------------------

TENSORS = ("dq", "dk", "dv")


def row_norm(t, H):
    """[B, N, H*64] -> the 2-norm of every head row, [B, N, H]"""
    t = t.detach().cpu().to(F64)
    return t.reshape(t.shape[0], t.shape[1], H, 64).norm(dim=-1)


def gate_terms(spec_t, rq_t, rk_t, mag_t, H):
    """the per-row terms of one output tensor: both sides' model error, the output floor, the fp32 term"""
    return SimpleNamespace(mq=row_norm(rq_t - spec_t, H), mk=row_norm(rk_t - spec_t, H),
                           floor=U9 * row_norm(spec_t, H), f32=U16 * row_norm(mag_t, H))


def bound(t, C):
    return C * torch.maximum(torch.maximum(t.mq, t.mk), t.floor) + t.f32


def ratio_to(err, allowed):
    """err / allowed per element with 0 / 0 = 0; anything non-finite counts as infinitely wrong"""
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    return torch.nan_to_num(r, nan=math.inf, posinf=math.inf)


def gate(got, ref, name, side=None):
    """ratio of |got_r - spec_r|_2 to the bound for every head row of tensor `name` ([B, N, H]); <= 1 passes.
    side "q" / "k" (a report, never the test): the bound with that side's model alone and C = 1."""
    H = ref.H
    got = got.detach().cpu().to(F64)
    err = row_norm(torch.nan_to_num(got, nan=math.inf) - getattr(ref.spec, name), H)
    t = ref.terms[name]
    if side:
        return ratio_to(err, torch.maximum(t.mq if side == "q" else t.mk, t.floor) + t.f32)
    return ratio_to(err, bound(t, ref.C))


def delta_gate(got, ref):
    """|got - D| / (2^-17 sum |dO_i O_i|) per element of delta [B, H, Nq]"""
    got = got.detach().cpu().to(F64)
    return ratio_to((torch.nan_to_num(got, nan=math.inf) - ref.spec.delta).abs(), U17 * ref.mag_delta)


def worst(ratio, rows_last=False):
    """(ratio, text) of the worst row of a [B, N, H] (or, rows_last, [B, H, N]) ratio tensor"""
    if ratio.numel() == 0:
        return 0.0, "no rows"
    i = int(ratio.argmax())
    a, b, c_ = (int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
    b_, n, h = (a, c_, b) if rows_last else (a, b, c_)
    return float(ratio.flatten()[i]), f"(b, n, h) = ({b_}, {n}, {h}), n % 128 = {n % 128}, n % 64 = {n % 64}"


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------

def _ln(x):
    return (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)


def qk_ln(g, B, N, H, head_gain):
    """qk-LayerNorm-like rows in [B, H, N, 64] float32: per-head LayerNorm of randn times a per-channel gain
    head_gain[h] * U(0.5, 1.5)"""
    x = _ln(torch.randn(B, H, N, 64, generator=g))
    gain = torch.tensor(head_gain, dtype=torch.float32)[:, None] * (0.5 + torch.rand(H, 64, generator=g))
    return x * gain[None, :, None, :]


def to_bf(x):
    """[B, H, N, 64] -> bf16 [B, N, H*64]"""
    return unheads(x).to(BF)


class Case:
    """One launch of the backward: a shape, a seed and an input builder.  `layout` names how the GPU test lays the
    tensors out in memory (tests/test_attention_bwd_kernels_gpu.py); `degenerate`: a case whose reference is zero or
    mass-free by construction (one key, one query), exempt from the floor-share requirement."""

    def __init__(self, group, name, B, H, Nq, Nk, scale=0.125, kind="ln", k_len=None, seed=0, layout="plain",
                 degenerate=False, gains=None, **kw):
        self.group, self.name, self.B, self.H, self.Nq, self.Nk = group, name, B, H, Nq, Nk
        self.scale, self.kind, self.k_len, self.seed, self.layout = scale, kind, k_len, seed, layout
        self.degenerate, self.gains, self.kw = degenerate, gains, kw
        self.id = f"{group}/{name}"
        self.cgroup = f"{group}/{kind}" if group == "score_range" else group  # the key of its C_GATE

    def __repr__(self):
        return self.id


def _build(case):
    B, H, Nq, Nk = case.B, case.H, case.Nq, case.Nk
    g = torch.Generator().manual_seed(1000 + case.seed)
    gq, gk = case.gains if case.gains is not None else ([1.5] * H, [1.0] * H)
    q, k = qk_ln(g, B, Nq, H, gq), qk_ln(g, B, Nk, H, gk)
    v = torch.randn(B, H, Nk, 64, generator=g)
    do = torch.randn(B, H, Nq, 64, generator=g) * torch.exp2(4 * torch.rand(B, 1, Nq, 1, generator=g) - 2)
    c = f32(case.scale) * LOG2E
    if case.kind == "batch0":  # one batch row of keys and values, expanded
        k, v = k[:1].expand(B, -1, -1, -1), v[:1].expand(B, -1, -1, -1)
    if case.kind in ("peak", "spread"):
        # gains up to 6 (tests/test_kernels_gpu.py::test_attention_large_gamma_scores): scores over hundreds of
        # log2 units
        gam_q, gam_k = 6 * torch.rand(H, 64, generator=g), 6 * torch.rand(H, 64, generator=g)
        q = _ln(torch.randn(B, H, Nq, 64, generator=g)) * gam_q[None, :, None, :]
        k = _ln(torch.randn(B, H, Nk, 64, generator=g)) * gam_k[None, :, None, :]
    def lean(q, rows, keys, own, mass):
        """queries `rows`: q_i = own q_i + beta_i k_j with the smallest beta_i (bisection, on the bf16 operands) at
        which key j = keys[(position of i in rows) % len(keys)] holds `mass` of row i"""
        col = torch.tensor([keys[n % len(keys)] for n in range(len(rows))])
        kj, kbf = k[:, :, col], k.to(BF).double()

        def share(beta):
            qq = (own * q[:, :, rows] + beta[..., None] * kj).to(BF).double()
            p = torch.softmax(c * math.log(2.0) * (qq @ kbf.transpose(-1, -2)), -1)
            return p[..., torch.arange(len(rows)), col]

        lo, hi = torch.zeros(B, H, len(rows)), torch.full((B, H, len(rows)), 8.0)
        for _ in range(40):
            mid = (lo + hi) / 2
            ok = share(mid) >= mass
            lo, hi = torch.where(ok, lo, mid), torch.where(ok, mid, hi)
        q = q.clone()
        q[:, :, rows] = own * q[:, :, rows] + hi[..., None] * kj
        return q

    if "keys" in case.kw:  # every fourth query: a designated key holds `mass` of the row
        q = lean(q, torch.arange(0, Nq, 4), case.kw["keys"], 0.25, case.kw["mass"])
    if "soft_keys" in case.kw:
        # every eighth query is beta_i k_j alone, with 0.3 of its row on key j: all its scores stay within a few log2
        # units, so the rounding of the scores operand moves nothing by more than the output's rounding, and the key
        # counted twice shows in dq at these gains too (where it holds 0.9992, Sum_j dS_j = 0 hides it in the model)
        q = lean(q, torch.arange(2, Nq, 8), case.kw["soft_keys"], 0.0, 0.3)
    if case.kind == "spread":
        # a component a u shared by every key and t_i u in query i (|u| = 8: about 1 per channel, a and |t_i| about 5:
        # the size of the gained channels) moves row i's scores, and its lse, by c t_i a |u|^2 = U(-350, 350) without
        # changing its softmax
        u = torch.randn(64, generator=g)
        u = 8 * u / u.norm()
        a = math.sqrt(350.0 / (c * 64.0))
        t = a * (2 * torch.rand(B, H, Nq, 1, generator=g) - 1)
        q = q - ((q @ u) / 64.0)[..., None] * u + t * u  # q's own component along u replaced by t_i u
        k = k - ((k @ u) / 64.0)[..., None] * u + a * u  # and k's by a u: u . k_j = 64 a for every key
    if case.kind in ("peak", "spread"):
        # at these gains 2 to 3 % of rows give one key all but 1e-5 of their mass, and such a row's dq is zero up to
        # fp32 noise: every row whose top key holds more than 0.9992 is scaled down (bisection, on the bf16 operands)
        # until it holds that
        kbf = k.to(BF).double()

        def top_share(tau):
            return torch.softmax(c * math.log(2.0) * ((tau[..., None] * q).to(BF).double() @ kbf.transpose(-1, -2)),
                                 -1).max(-1).values

        lo, hi = torch.zeros(B, H, Nq), torch.ones(B, H, Nq)
        for _ in range(30):
            mid = (lo + hi) / 2
            ok = top_share(mid) <= 0.9992
            lo, hi = torch.where(ok, mid, lo), torch.where(ok, hi, mid)
        q = torch.where((top_share(torch.ones(B, H, Nq)) <= 0.9992)[..., None], q, lo[..., None] * q)
        # rows this peaked have dP_j - D cancel for their top key j; dO_i = 0.5 randn + m_i v_j (m_i the row's
        # magnitude) keeps dO_i . v_j itself free of cancellation, so that the fp32 term of the gate stays small
        top = (q.to(BF).double() @ k.to(BF).double().transpose(-1, -2)).argmax(-1)  # [B, H, Nq]
        vj = torch.gather(v, 2, top[..., None].expand(-1, -1, -1, 64))
        m = torch.exp2(4 * torch.rand(B, 1, Nq, 1, generator=g) - 2)
        do = m * (0.5 * torch.randn(B, H, Nq, 64, generator=g) + vj)
    if case.kind == "last":
        # the last key leans towards the queries (for one query: it holds a real share of the row), so that a key
        # dropped or counted twice at the end shows
        d = q.mean(2)
        k = k.clone()
        k[:, :, -1] += 4 * d / d.norm(dim=-1, keepdim=True)
    q, k, v, do = to_bf(q), to_bf(k), to_bf(v), to_bf(do)
    k_len = None if case.k_len is None else torch.tensor(case.k_len, dtype=torch.int32)
    if k_len is not None and len(k_len) != B:
        k_len = k_len.repeat((B + len(k_len) - 1) // len(k_len))[:B].contiguous()
    extra = None
    if case.kind in ("extra", "klen"):
        # log2 of the additional mass: 0.1 x .. 10 x the keys' own, per query (a row without keys: 2^U(-3, 3))
        _, own = forward(q, k, v, H, case.scale, k_len, exact=True)
        r = torch.rand(B, H, Nq, generator=g).double()
        extra = torch.where(torch.isfinite(own), own + math.log2(0.1) + r * math.log2(100.0), 6 * r - 3)
    o64, _ = forward(q, k, v, H, case.scale, k_len, extra, exact=True)
    o, lse = forward(q, k, v, H, case.scale, k_len, extra)
    if k_len is not None:  # the header's "never read": K / V rows at or past each length hold NaN
        k, v = k.clone(), v.clone()
        for b, L in enumerate(lengths(k_len, B, Nk)):
            k[b, L:] = math.nan
            v[b, L:] = math.nan
    return SimpleNamespace(q=q, k=k, v=v, do=do, o=unheads(o).to(BF), lse=lse.to(torch.float32), k_len=k_len,
                           extra=extra, o64=o64)


@functools.lru_cache(maxsize=4)
def inputs(case):
    return _build(case)


@functools.lru_cache(maxsize=4)
def reference(case):
    """spec, the gate's per-row terms for dq / dk / dv, and sum |dO O| for delta; computed once per case"""
    x = inputs(case)
    a = (x.q, x.k, x.v, x.o, x.do, x.lse, case.H, case.scale, x.k_len)
    sp, rq, rk, mg = spec(*a), rounded(*a, side="q"), rounded(*a, side="k"), mag(*a)
    terms = {n: gate_terms(getattr(sp, n), getattr(rq, n), getattr(rk, n), getattr(mg, n), case.H) for n in TENSORS}
    return SimpleNamespace(H=case.H, C=C_GATE[case.cgroup], spec=sp, terms=terms, mag_delta=mg.delta)


LENGTHS = (1, 31, 32, 33, 64, 65, 97, 128, 129, 200)
# the tail split needs more blocks than are resident at once (expected from the launch bounds: 2 x 256 dQ and 3 x 256
# dK / dV workgroups on an MI355X; the GPU test asserts that the split is active): B x H heads of few tokens.  A kernel
# splits when its block count n leaves a remainder r against the resident count s with r + s <= n.  dK / dV arm:
# 120 heads x 8 key blocks = 960 (r = 192 at s = 768; 448 at 512), dQ at 240 blocks; dQ arms: 100 heads x 8 query
# blocks = 800 (r = 288 at s = 512; 32 at 768), dK / dV at 200 blocks: in each arm only one kernel can split.
SPLIT_KLEN = (64, 130, 0, 200, 190, 33, 1, 129)  # 1 tile (empty pieces), 3 tiles in 4 pieces, none, full, ragged


def _cases():
    cs = []
    for nq in LENGTHS:
        for nk in LENGTHS:
            cs.append(Case("lengths", f"{nq}x{nk}", 1, 2, nq, nk, seed=len(cs), degenerate=nq == 1 or nk == 1,
                           kind="last", gains=([0.6, 2.4], [1.0, 1.0])))
    cs.append(Case("strides", "thirds", 2, 3, 200, 200, seed=200, layout="thirds"))
    cs.append(Case("strides", "distinct", 2, 3, 200, 330, seed=201, layout="distinct"))
    cs.append(Case("strides", "batch0", 2, 3, 200, 330, seed=202, layout="batch0", kind="batch0"))
    for i, s in enumerate((0.07, 0.125, 0.3)):
        cs.append(Case("scale", f"{s}", 1, 2, 129, 193, scale=s, seed=210 + i))
    cs.append(Case("score_range", "peak_partial", 1, 2, 640, 650, kind="peak", seed=220, keys=(649,), mass=0.9992,
                   soft_keys=(649,)))
    cs.append(Case("score_range", "peak_boundary", 1, 2, 640, 640, kind="peak", seed=221, keys=(63, 64, 639),
                   mass=0.9992))
    cs.append(Case("score_range", "spread", 1, 2, 640, 640, kind="spread", seed=222, keys=(639,), mass=0.9992))
    cs.append(Case("extra_mass", "extra", 1, 2, 200, 330, kind="extra", seed=230))
    cs.append(Case("k_len", "edges", 8, 2, 200, 330, kind="klen", seed=240, k_len=(0, 1, 32, 63, 64, 128, 330, 500)))
    cs.append(Case("k_len", "negative", 8, 2, 200, 330, kind="klen", seed=241,
                   k_len=(-7, 2, 31, 33, 65, 127, 329, 331)))
    cs.append(Case("k_len", "no_extra", 8, 2, 200, 330, seed=242, k_len=(200, 2, 31, 33, 65, 127, 329, 331)))
    cs.append(Case("tail_split", "dkdv", 60, 2, 200, 900, seed=250))
    cs.append(Case("tail_split", "dq", 50, 2, 900, 200, seed=251))
    cs.append(Case("tail_split", "dq_k_len", 50, 2, 900, 200, seed=252, kind="klen", k_len=SPLIT_KLEN))
    return cs


CASES = _cases()


def group(name):
    return [c for c in CASES if c.group == name]
