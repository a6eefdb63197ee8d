"""tests/gemm_refs.py on the CPU: the references agree with one-line torch forms, the exactness preconditions of every
case hold, the gate (gemm_refs.check_output, the function tests/test_gemm_epilogues_gpu.py asserts with) accepts the
reference itself and rejects every mutant wherever the mutant can show, and the c_f32 constant of the forward head
vectors is what the measurement says."""
import pytest
import torch
import torch.nn.functional as F

from tests import backward_refs as R
from tests import gemm_refs as G
from tests import mx_ref

BF = torch.bfloat16


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rb(g, *shape, std=1.0):
    return (torch.randn(*shape, generator=g) * std).to(BF)


# ------------------------------------------------------------------------------------------------------------------
# the references against plain torch
# ------------------------------------------------------------------------------------------------------------------

def test_epilogue_ref_matches_one_line_torch_forms():
    g = _g(1)
    M, N, Kk = 37, 24, 40
    a, w, b = _rb(g, M, Kk), _rb(g, N, Kk, std=Kk ** -0.5), _rb(g, N, std=0.1)
    lin = F.linear(a.float(), w.float(), b.float())
    y = R.rnd_bf16(lin)
    U = G.U8

    def close(ref, plain, mag):  # ref carries up to 3 roundings to bf16 that the plain form does not
        assert bool(((ref.double() - plain.double()).abs() <= 3.01 * U * mag.double() + 1e-6).all())

    close(G.epilogue_ref(G.BIAS, y), lin, lin.abs())
    close(G.epilogue_ref(G.SCALE, y, alpha=0.37), lin * 0.37, lin.abs())
    gate, Rr, inj = _rb(g, M, N), _rb(g, M, N), _rb(g, M, N)
    on = torch.rand(M, generator=g) > 0.5
    plain = Rr.float() + gate.float() * lin + inj.float() * on[:, None]
    mag = Rr.float().abs() + (gate.float() * lin).abs() * 2 + inj.float().abs() + plain.abs()
    close(G.epilogue_ref(G.GATED, y, gate_rows=gate, R_rows=Rr, inject_rows=inj, inject_on=on), plain, mag)
    close(G.epilogue_ref(G.GATED, y, gate_rows=gate, R_rows=Rr), Rr.float() + gate.float() * lin, mag)
    add = _rb(g, M, N)
    close(G.epilogue_ref(G.ADDROWS, y, addrows_rows=add), lin + add.float(), lin.abs() + add.float().abs())
    # GELU / GELU_BWD: float64 of the exactly known y, against torch's tanh form and its autograd
    ge = G.epilogue_ref(G.GELU, y)
    assert ge.dtype == torch.float64
    assert float((ge - F.gelu(y.double(), approximate="tanh")).abs().max()) < 1e-12
    z = _rb(g, M, N, std=2.0)
    zz = z.double().requires_grad_()
    F.gelu(zz, approximate="tanh").backward(y.double())
    assert float((G.epilogue_ref(G.GELU_BWD, y, z=z) - zz.grad).abs().max()) < 1e-12


@pytest.mark.parametrize("T,rope,masked", [(0, True, False), (5, True, False), (5, False, False), (5, True, True)])
def test_head_norm_rope_ref_matches_layer_norm_and_the_oracles_rotary(T, rope, masked):
    from oracle.cogvideox_oracle import apply_rotary_emb
    cos, sin = R.head_rope()
    B, H, N = 2, 3, T + cos.shape[0]
    g = _g(2)
    x = _rb(g, B, N, H * 64, std=2.0)
    lw, lb = (1 + 0.2 * torch.randn(64, generator=g)).to(BF), (0.1 * torch.randn(64, generator=g)).to(BF)
    mask = G.head_fwd_mask(B, N) if masked else None
    r = G.head_norm_rope_ref(x, lw, lb, 1e-6, H, T, (cos, sin) if rope else None, mask=mask, pre_scale=0.5)
    xin = x.double() if mask is None else x.double() * mask[..., None].double() * 0.5
    n = F.layer_norm(xin.view(B, N, H, 64).transpose(1, 2), (64,), lw.double(), lb.double(), 1e-6)
    if rope:
        n = torch.cat([n[:, :, :T], apply_rotary_emb(n[:, :, T:].float(), cos, sin).double()], 2)
    want = n.transpose(1, 2).reshape(B, N, H * 64)
    assert float((r["y"] - want).abs().max()) < (2e-5 if rope else 1e-10)  # the oracle's rotation is fp32
    assert bool((r["E"] >= r["y"].abs() * (1 - 1e-12)).all()) and bool((r["mag"] >= r["y"].abs() * (1 - 1e-12)).all())
    if masked:  # a zeroed row is the (rotated) LayerNorm bias, exactly
        rows = (mask == 0)
        rows[:, T:] = False
        assert torch.equal(r["y"][rows], lb.double().repeat(H).expand(int(rows.sum()), H * 64))


def test_exact_y_is_the_rounded_linear():
    c = G.case("probe", G.BIAS, 37, 136, 24, nsegs=2, seed=3)
    t = G.inputs(c)
    o = t.ops
    lin = F.linear(o.a.double(), torch.cat(o.w).double(), torch.cat(o.bias).double())
    assert torch.equal(lin.float().double(), lin)  # exactly representable
    ex = G.expected(c, t)["C"]
    assert torch.equal(ex.buf[:c.M, :c.N].double(), R.rnd_bf16(lin))
    # y uses the whole bf16 mantissa: most sums need the rounding
    assert float((ex.buf[:c.M, :c.N].double() != lin).double().mean()) > 0.5


# ------------------------------------------------------------------------------------------------------------------
# preconditions, the gate on the reference itself, the mutants
# ------------------------------------------------------------------------------------------------------------------

LISTS = G.small_case_lists()

# (mutant, case list) pairs on which the mutant cannot show, by name: no case of the list meets mutant_applies
INVISIBLE = {
    "gate_prev_batch": {"rows_cols", "addrows", "qknorm"},
    "text_gate_at_T": {"rows_cols", "addrows", "qknorm"},
    "video_gate_at_Tm1": {"rows_cols", "addrows", "qknorm"},
    "neighbour_bias": {"main_loops"},
    "inject_on_masked": {"rows_cols", "addrows", "qknorm"},
    "inject_vtok_p1": {"rows_cols", "addrows", "qknorm"},
    "addrows_offset_p1": {"main_loops", "rows_cols", "gated", "a_tail", "qknorm"},
    "remap_last_row_p1": {"main_loops", "rows_cols", "splitk", "a_tail", "qknorm"},
    "drop_inner_rnd": {"rows_cols", "addrows", "qknorm"},
    "drop_last_8k": set(),
    "add_a_padding": {"gated", "addrows", "splitk", "qknorm", "mx"},
    "rope_last_text_row": {"main_loops", "rows_cols", "gated", "addrows", "splitk", "mx"},
    "eps_q_for_k": {"main_loops", "rows_cols", "gated", "addrows", "splitk", "mx"},
}


# case lists that the mutant sweep below leaves out altogether, by name and with the reason
NOT_SWEPT = {"tail": "4352 x 4096 outputs per case: its expectation is built once, in "
                     "test_tail_shape_preconditions_and_gate, with the one mutant that a large shape can add "
                     "(drop_last_8k); its epilogues and edges are those of the swept lists"}


def test_every_case_list_is_swept_or_named():
    assert set(G.all_case_lists()) == set(LISTS) | set(NOT_SWEPT) and not set(LISTS) & set(NOT_SWEPT)


def _got(ex):
    return {k: None if v is None else v.buf for k, v in ex.items()}


def _rejected(c, ex, wrong):
    """the gate on a wrong result: at least one of the launch's output buffers is refused"""
    hits = 0
    for k in ("C", "aux"):
        if ex[k] is None or (k == "C" and c.epi == G.GELU_MX):
            continue
        try:
            G.check_output(c.name, ex[k], wrong[k], quiet=True)
        except AssertionError:
            hits += 1
    return hits > 0


@pytest.mark.parametrize("name", sorted(LISTS))
def test_gate_accepts_the_reference_and_rejects_every_mutant(name):
    applied = {mu: 0 for mu in G.MUTANTS}
    for c in LISTS[name]:
        t = G.inputs(c)  # asserts the exactness precondition of the case's operands
        ex = G.expected(c, t)
        for k in ("C", "aux"):
            if ex[k] is not None:
                assert G.check_output(c.name, ex[k], ex[k].buf, quiet=True) <= 1.0
        for mu in G.MUTANTS:
            if not G.mutant_applies(mu, c, t):
                continue
            applied[mu] += 1
            assert _rejected(c, ex, _got(G.expected(c, t, mutant=mu))), f"mutant {mu} passes on {c.name}"
    # no mutant is skipped silently: the lists on which one cannot show are exactly the ones named above
    for mu in G.MUTANTS:
        assert (applied[mu] == 0) == (name in INVISIBLE[mu]), (mu, name, applied[mu])


def test_every_mutant_is_seen_somewhere():
    for mu in G.MUTANTS:
        assert set(LISTS) - INVISIBLE[mu], mu


def test_mx_operands_quantise_without_error():
    for c in G.mx_cases():
        o = G.inputs(c).ops
        for x in [o.a] + o.w:
            q, s = mx_ref.quantize(x)
            assert torch.equal(mx_ref.dequantize(q, s, x.shape[0], x.shape[1]), x.float()), c.name


def test_tail_shape_preconditions_and_gate():
    c = G.tail_cases()[0]
    t = G.inputs(c)
    ex = G.expected(c, t)["C"]
    assert G.check_output(c.name, ex, ex.buf, quiet=True) == 0.0
    wrong = G.expected(c, t, mutant="drop_last_8k")["C"].buf
    with pytest.raises(AssertionError):
        G.check_output(c.name, ex, wrong, quiet=True)


def test_sentinels_and_untouched_rows_are_part_of_the_gate():
    c = [c for c in G.gated_cases() if c.name == "gated remap per-row"][0]
    t = G.inputs(c)
    ex = G.expected(c, t)["C"]
    for r, col in ((0, 0), (c.ro + c.rpg, 3), (c.out_rows, 0), (c.ro, c.N)):  # skipped rows, guard row, ldc gap
        assert float(ex.buf[r, col]) == G.SENT
        wrong = ex.buf.clone()
        wrong[r, col] = 1.0
        with pytest.raises(AssertionError):
            G.check_output(c.name, ex, wrong, quiet=True)


# ------------------------------------------------------------------------------------------------------------------
# constants and bounds
# ------------------------------------------------------------------------------------------------------------------

def head_fwd_operands():
    """(x [B, N, H 64], lw, lb, eps, H, T, rope, mask, pre_scale) of every forward head-vector check of the GPU file"""
    out = []
    for c in G.qknorm_cases() + [c for c in G.a_tail_cases() if c.epi == G.QKNORM]:
        t = G.inputs(c)
        y = G.expected(c, t)["aux" if c.aux else "C"].buf[:c.M].float()
        for s in range(2):
            ys = R.rnd_bf16(t.ops.acc + t.ops.bias_row)[:, s * c.n_seg:(s + 1) * c.n_seg]
            if c.aux:
                assert torch.equal(ys, y[:, s * c.n_seg:(s + 1) * c.n_seg])
            out.append((ys.reshape(c.B, c.tpb, c.n_seg), t.lnw[s], t.lnb[s], t.eps[s], c.H, c.T, t.rope, None, 1.0))
    for H, T, kind in R.HEAD_CASES:
        c = R.head_case(H, T, kind)
        for which in (0, 1):
            x, _, rope = R.head_operands(c, H, which)
            out.append((x, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope, None, 1.0))
            out.append((x, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope, G.head_fwd_mask(R.HEAD_B, c["N"]), 0.5))
    return out


def test_c_f32_head_fwd():
    """C_F32_HEAD_FWD = 8 x the worst fp32-vs-fp64 error of head_norm_rope_ref in units of E (rounded up)"""
    worst = 0.0
    for x, lw, lb, eps, H, T, rope, mask, ps in head_fwd_operands():
        r64 = G.head_norm_rope_ref(x, lw, lb, eps, H, T, rope, mask=mask, pre_scale=ps)
        r32 = G.head_norm_rope_ref(x, lw, lb, eps, H, T, rope, mask=mask, pre_scale=ps, dt=torch.float32)
        worst = max(worst, R.worst_ratio((r32["y"].double() - r64["y"]).abs(), r64["E"]))
    print(f"c_f32 forward head vectors: worst |fp32 - fp64| / E = {worst:.3e}, x 8 = {8 * worst:.3e}, constant "
          f"{G.C_F32_HEAD_FWD:.3e}")
    assert G.C_F32_HEAD_FWD / 2 <= 8 * worst <= G.C_F32_HEAD_FWD


@pytest.mark.parametrize("K", G.ACCUM_KS)
def test_accum_bound_holds_for_fp32_and_sees_a_dropped_k_block(K):
    a, w, b = G.accum_case(77, 40, K, 300 + K)
    y64, allowed = G.accum_bound(a, w, b)
    got = (a.float() @ w.float().T + b.float()).to(BF).double()
    ratio = R.worst_ratio((got - y64).abs(), allowed)
    print(f"accum K = {K}: fp32 torch worst error / allowed = {ratio:.4f}")
    assert ratio <= 1.0
    wrong = (a.float()[:, :K - 8] @ w.float()[:, :K - 8].T + b.float()).to(BF).double()
    assert R.worst_ratio((wrong - y64).abs(), allowed) > 1.0


# ------------------------------------------------------------------------------------------------------------------
# zeroed rows behind LN + RoPE, and the AdaLN modulation's exact chain
# ------------------------------------------------------------------------------------------------------------------

def test_zeroed_rows_are_the_rotated_bias_exactly():
    """head_norm_rope_ref on a masked (zeroed) row is the rotation of the LayerNorm bias with no LN error at all, and
    rot_bias_bits (the kernel's fp32 order) is that value rounded: at most 1 bf16 ulp from the direct rounding, equal
    almost everywhere"""
    H, T = 3, 8
    c = R.head_case(H, T, "rope")
    x, _, rope = R.head_operands(c, H, 1)
    B, N = R.HEAD_B, c["N"]
    mask = G.head_fwd_mask(B, N)
    r = G.head_norm_rope_ref(x, c["lw"], c["lb"], R.HEAD_EPS, H, T, rope, mask=mask, pre_scale=0.5)
    b = c["lb"].double()
    cos, sin = (t.double() for t in rope)
    want = torch.stack((b[0::2] * cos[:, 0::2] - b[1::2] * sin[:, 0::2],
                        b[1::2] * cos[:, 1::2] + b[0::2] * sin[:, 1::2]), -1).flatten(-2).repeat(1, H)  # [Nv, H 64]
    bits = G.rot_bias_bits(c["lb"], H, rope)
    n_rows = 0
    for bi in range(B):
        for n in range(N):
            if mask[bi, n] == 0:
                n_rows += 1
                if n < T:
                    assert torch.equal(r["y"][bi, n], b.repeat(H))
                else:
                    assert torch.equal(r["y"][bi, n], want[n - T])
    assert n_rows > 4
    u = R.bf16_ulps(bits, R.rnd_bf16(want).to(BF))
    assert int(u.max()) <= 1 and float((u == 0).double().mean()) > 0.99
    assert torch.equal(G.rot_bias_bits(c["lb"], H, None)[0], c["lb"].repeat(H))


@pytest.mark.parametrize("D", G.ADALN_EXACT_DS)
def test_adaln_exact_ref_is_the_documented_chain(D):
    """the exact-case chain against the float64 references of backward_refs (their allowance), the exactness of its
    LayerNorm, and the mutant without rnd(n s1): it changes bits, so a bit comparison rejects it"""
    c = G.adaln_exact_case(D)
    eps = G.ADALN_EXACT_EPS
    x = c["x"].double()
    assert bool((x.mean(-1) == 0).all()) and bool((((x - x.mean(-1, keepdim=True)) ** 2).mean(-1) + eps == 1.0).all())
    for T in (0, 5, G.ADALN_EXACT_N):
        got = G.adaln_exact_ref(c, T)
        r = R.adaln_modulate_ref(c["x"], c["mod"], c["lw"], c["lb"], eps, T)
        assert R.worst_ratio((got.double() - r["y"]).abs(), G.U8 * r["mag"] + R.C_F32_ADALN * r["E"]) <= 1.0
        wrong = G.adaln_exact_ref(c, T, product_rnd=False)
        assert float((wrong.float() != got.float()).double().mean()) > 0.05
    ones, zeros = torch.ones(D).to(BF), torch.zeros(D).to(BF)
    for T in (0, 5):
        got = G.adaln_exact_ref(c, T, final=True)
        r = R.final_norm_ref(c["x"], T, ones, zeros, c["lw"], c["lb"], eps, c["mod"][:, :2 * D])
        assert R.worst_ratio((got.double() - r["y"]).abs(), G.U8 * r["mag"] + R.C_F32_ADALN * r["E"]) <= 1.0
        assert float((G.adaln_exact_ref(c, T, final=True, product_rnd=False).float() != got.float()).double().mean()) > 0.05
