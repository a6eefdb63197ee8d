"""The references of tests/attention_refs.py checked against float64 autograd on the CPU, and what the gate of
tests/test_attention_bwd_kernels_gpu.py rests on, measured over exactly the GPU cases on the references alone: the
constant C_GATE, the gate's power against deliberately wrong evaluations, and the share of rows in which the fp32
term outweighs the rest of the bound.  Nothing here runs the code under test.

Measured (python -m pytest tests/test_attention_refs_cpu.py -s; profiles/attention_bwd_kernel_tests.log), worst
side-to-side ratio -> C = max(3, ceil(2 x ratio)) per group of cases:
  lengths 9.080 -> 19, strides 5.232 -> 11, scale 8.382 -> 17, score_range/peak 26.701 -> 54, score_range/spread
  91.239 -> 183, extra_mass 3.786 -> 8, k_len 6.991 -> 14, tail_split 9.232 -> 19; one constant for all: 183.
Mutants: a key dropped / counted twice at the length, the neighbour's lse and D on a tile's last row, scale 0.125 in
dq / dk / c are seen in every case they can change; D from the unrounded o (reported only) is seen in about a quarter
of the cases.
"""
import math

import pytest
import torch

from tests import attention_refs as A

F64 = torch.float64
LN2 = math.log(2.0)
REQUIRED = ("drop_last", "one_more", "neighbour_stats", "scale_dq", "scale_dk", "scale_c")


def _autograd(q, k, v, do, H, scale, k_len=None, extra=None):
    """float64 autograd through softmax(scale q k^T) v per head over the valid keys; `extra`: one more key per query
    with logit extra * ln 2 and a zero value.  Returns dq, dk, dv [B, N, H*64] (zero rows past a length)."""
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    Q, K, V, G = (A.heads(t, H).clone().requires_grad_() for t in (q, k, v, do))
    loss = 0
    for b, L in enumerate(A.lengths(k_len, B, Nk)):
        logit = A.f32(scale) * (Q[b] @ K[b, :, :L].transpose(-1, -2))
        val = V[b, :, :L]
        if extra is not None:
            logit = torch.cat([logit, extra[b][..., None] * LN2], -1)
            val = torch.cat([val, torch.zeros(H, 1, 64, dtype=F64)], 1)
        loss = loss + (torch.softmax(logit, -1) @ val * G[b].detach()).sum()
    dq, dk, dv = torch.autograd.grad(loss, (Q, K, V))
    return A.unheads(dq), A.unheads(dk), A.unheads(dv)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("k_len, with_extra", [(None, False), ((0, 5, 70), False), (None, True), ((0, 5, 70), True)])
def test_spec_matches_autograd(k_len, with_extra):
    """with o and lse left in float64, spec is autograd's gradient to 1e-12"""
    B, H, Nq, Nk, scale = 3, 2, 37, 70, 0.3
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(B, n, H * 64, generator=g, dtype=F64) for n in (Nq, Nk, Nk, Nq))
    extra = torch.randn(B, H, Nq, generator=g, dtype=F64) * 3 if with_extra else None
    if k_len is not None and not with_extra:
        k_len = (1,) + k_len[1:]  # (a row without keys and without extra mass has no softmax)
    o, lse = A.forward(q, k, v, H, scale, k_len, extra, exact=True)
    if k_len is not None:
        k, v = k.clone(), v.clone()
        for b, L in enumerate(A.lengths(k_len, B, Nk)):
            k[b, L:], v[b, L:] = math.nan, math.nan  # never touched
    s = A.spec(q, k, v, A.unheads(o), do, lse, H, scale, k_len)
    kz, vz = torch.nan_to_num(k), torch.nan_to_num(v)
    dq, dk, dv = _autograd(q, kz, vz, do, H, scale, k_len, extra)
    for name, want in (("dq", dq), ("dk", dk), ("dv", dv)):
        r = _rel(getattr(s, name), want)
        print(f"  spec vs autograd, k_len {k_len}, extra {with_extra}: {name} rel {r:.2e}")
        assert r <= 1e-12
    assert _rel(s.delta, (A.heads(do, H) * o).sum(-1)) <= 1e-14
    for b, L in enumerate(A.lengths(k_len, B, Nk)):
        assert not s.dk[b, L:].any() and not s.dv[b, L:].any()


def test_forward_rounds_what_the_kernel_is_handed():
    c = A.group("scale")[1]
    x = A.inputs(c)
    o, lse = A.forward(x.q, x.k, x.v, c.H, c.scale)
    assert torch.equal(A.unheads(o).to(A.BF), x.o) and torch.equal(lse.to(torch.float32), x.lse)
    s = A.f32(c.scale) * A.LOG2E * (A.heads(x.q, c.H) @ A.heads(x.k, c.H).transpose(-1, -2))
    p = torch.exp2(s - lse[..., None])
    assert float((p.sum(-1) - 1).abs().max()) < 1e-6  # (fp32 lse)


def _applies(m, case, x):
    if m == "drop_last":
        return max(A.lengths(x.k_len, case.B, case.Nk)) >= 1
    if m == "neighbour_stats":
        return case.Nq >= 64
    if m.startswith("scale"):
        return case.scale != 0.125
    return True


@pytest.fixture(scope="module")
def survey():
    """one pass over every GPU case: per tensor the side-to-side ratio and the fp32-dominated share, per mutant
    whether the gate sees it"""
    rows = []
    for case in A.CASES:
        x, ref = A.inputs(case), A.reference(case)
        rec = {"case": case, "ratio": {}, "share": {}, "mutants": {}}
        for n in A.TENSORS:
            t = ref.terms[n]
            hi, lo = torch.maximum(t.mq, t.mk), torch.minimum(t.mq, t.mk)
            keep = (hi >= t.floor) & (hi >= t.f32) & (hi > 0)
            r = torch.maximum(hi, t.floor)[keep] / torch.maximum(lo, t.floor)[keep]
            rec["ratio"][n] = float(r.max()) if r.numel() else 1.0
            rec["share"][n] = float((t.f32 > A.bound(t, ref.C) - t.f32).double().mean())
        for m in A.MUTANTS:
            if not _applies(m, case, x):
                continue
            mu = A.mutant(m, x.q, x.k, x.v, x.o, x.do, x.lse, case.H, case.scale, x.k_len, o_exact=x.o64)
            touched = seen = 0
            for n in A.TENSORS:
                d = A.row_norm(torch.nan_to_num(getattr(mu, n), nan=math.inf) - getattr(ref.spec, n), case.H)
                hit = d != 0
                touched += int(hit.sum())
                seen += int((hit & (A.gate(getattr(mu, n), ref, n) > 1)).sum())
            if touched or m not in ("drop_last", "one_more"):  # (one key: dS = 0 with the key twice, too)
                rec["mutants"][m] = (touched, seen)
        rows.append(rec)
    return rows


def test_c_gate(survey):
    """C_GATE[group] = max(3, ceil(2 x the worst side-to-side ratio)) over every row of the group's cases"""
    got = {}
    for g in dict.fromkeys(c.cgroup for c in A.CASES):
        worst, where = 0.0, ""
        for r in survey:
            for n, v in r["ratio"].items():
                if r["case"].cgroup == g and v > worst:
                    worst, where = v, f"{r['case'].id} {n}"
        assert math.isfinite(worst)
        got[g] = max(3, math.ceil(2 * worst))
        print(f"  side-to-side ratio, {g}: worst {worst:.3f} ({where}) -> C = max(3, ceil(2 x {worst:.3f})) = {got[g]}")
    print(f"  one constant for all cases would be {max(got.values())}")
    assert got == A.C_GATE


def test_gate_sees_the_mutants(survey):
    """the five wrong evaluations of tests/attention_refs.py MUTANTS against the gate, in every case they can affect:
    1 drop_last, 2 one_more, 3 neighbour_stats, 4 scale_dq / scale_dk / scale_c must violate it in rows they touch;
    5 d_exact_o (D from the unrounded o) is reported only"""
    missed = []
    for m in A.MUTANTS:
        recs = [r for r in survey if m in r["mutants"]]
        hit = [r for r in recs if r["mutants"][m][1] > 0]
        t, s = sum(r["mutants"][m][0] for r in recs), sum(r["mutants"][m][1] for r in recs)
        print(f"  mutant {m:16s}: seen in {len(hit):3d} of {len(recs):3d} cases, {s} of {t} touched rows violate")
        if m in REQUIRED:
            missed += [(m, r["case"].id) for r in recs if r["mutants"][m][1] == 0]
        else:
            print("    (sensitivity report, not required) seen in: " + ", ".join(r["case"].id for r in hit[:12])
                  + (" ..." if len(hit) > 12 else ""))
    print(f"  required and not seen: {missed}")
    assert not missed


def test_fp32_term_does_not_hide_failures(survey):
    """outside the degenerate cases the 2^-16 |mag| term exceeds the C max(..) term in at most 1 % of a tensor's rows"""
    bad = []
    for g in dict.fromkeys(c.group for c in A.CASES):
        recs = [r for r in survey if r["case"].group == g and not r["case"].degenerate]
        if recs:
            print(f"  fp32-dominated share of rows, {g}: "
                  + ", ".join(f"{n} max {100 * max(r['share'][n] for r in recs):.2f} %" for n in A.TENSORS))
    for r in survey:
        line = ", ".join(f"{n} {100 * v:.2f} %" for n, v in r["share"].items())
        if r["case"].group != "lengths" or r["case"].degenerate:
            print(f"    {r['case'].id}{' (degenerate)' if r['case'].degenerate else ''}: {line}")
        if not r["case"].degenerate:
            bad += [f"{r['case'].id} {n} {v:.4f}" for n, v in r["share"].items() if v > 0.01]
    assert not bad, bad


def test_score_range_cases_are_what_they_claim():
    for case in A.group("score_range"):
        x = A.inputs(case)
        c = A.f32(case.scale) * A.LOG2E
        s = c * (A.heads(x.q, case.H) @ A.heads(x.k, case.H).transpose(-1, -2))
        p = torch.exp2(s - x.lse.double()[..., None])
        print(f"  {case.id}: scores {float(s.min()):.0f} .. {float(s.max()):.0f} log2 units, "
              f"lse {float(x.lse.min()):.0f} .. {float(x.lse.max()):.0f}")
        assert float(s.max() - s.min()) >= 150
        if case.kind == "peak":
            keys = case.kw["keys"]
            top = p.max(-1)
            n = sum(int(((top.values >= 0.999) & (top.indices == j)).sum()) for j in keys)
            assert n >= case.B * case.H * case.Nq // 4, n
            assert all(int(((top.values >= 0.999) & (top.indices == j)).sum()) > 0 for j in keys)
        else:
            assert float(x.lse.min()) <= -300 and float(x.lse.max()) >= 300
    e = A.inputs(A.group("extra_mass")[0])
    own = torch.exp2(A.forward(e.q, e.k, e.v, 2, 0.125, exact=True)[1] - e.lse.double())  # the keys' share of the row
    assert 1 / 11.1 <= float(own.min()) and float(own.max()) <= 1 / 1.09
