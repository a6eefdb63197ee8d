"""vp_attention_bwd_bf16 (csrc/attention_bwd.hip: the delta pass, the dQ and dK / dV kernels, the tail merge) per head
row against the float64 references of tests/attention_refs.py, at its edges.  The cases, the gate and its constants
come from that file and are checked on the CPU by tests/test_attention_refs_cpu.py; nothing here runs the forward
kernel: o and lse are the float64 forward's, rounded to what the kernel is handed.

For each of dq, dk, dv and every (b, n, h):  |got_r - spec_r|_2 <= C max(model_r, 2^-9 |spec_r|_2) + 2^-16 |mag_r|_2;
delta per element: |got - D| <= 2^-17 sum |dO_i O_i|.  Every output lies inside a larger NaN-filled buffer: after the
call the guard rows and columns must hold the same NaN bits and the result must be finite.  Each case prints its worst
ratio to the bound per tensor (python -m pytest -s; profiles/attention_bwd_kernel_tests.log is such a run: worst dq
0.125, dk 0.125, dv 0.125, delta 0.031; no defect found)."""
import ctypes as C
import math

import pytest
import torch

from tests import attention_refs as A

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
G = 2  # guard rows before and after, and 8 guard columns on either side


@pytest.fixture(scope="module")
def K():
    from videopainter_amd import kernels
    print("\nC (tests/attention_refs.py C_GATE; measured by tests/test_attention_refs_cpu.py::test_c_gate as twice the "
          "worst side-to-side ratio of the two rounded references, per group of cases): "
          + ", ".join(f"{g} {c}" for g, c in A.C_GATE.items()))
    return kernels


def strided(t, row_stride, slack_rows=0, batch0=False):
    """t [B, N, D] on the device with the given row stride (and batch stride (N + slack_rows) * row_stride); batch0: one
    batch row expanded with batch stride 0"""
    B, N, D = t.shape
    if batch0:
        assert all(torch.equal(t[0].view(torch.int16), t[b].view(torch.int16)) for b in range(B))
        B = 1
    buf = torch.zeros(B, N + slack_rows, row_stride, device=dev, dtype=t.dtype)
    buf[:, :N, :D].copy_(t[:B])
    return buf[:, :N, :D].expand(t.shape[0], -1, -1) if batch0 else buf[:, :N, :D]


class Guarded:
    """a [B, N, width] region of a NaN-filled bf16 buffer with G guard rows and 8 guard columns around it (`pad`
    more columns: another row stride)"""

    def __init__(self, B, N, width, pad=0):
        self.buf = torch.full((B, N + 2 * G, width + 16 + pad), math.nan, device=dev, dtype=BF)
        self.bits = int(self.buf.view(torch.int16)[0, 0, 0])
        self.region = self.buf[:, G:G + N, 8:8 + width]

    def guards_intact(self):
        """(after the results were read) the region refilled with NaN, the whole buffer holds the fill's bits"""
        self.region.fill_(math.nan)
        return bool((self.buf.view(torch.int16) == self.bits).all())


def launch(K, case, x):
    """lay the case's tensors out as its layout says, run the backward, check the guards; returns the results on the
    CPU and the arguments (for the workspace query)"""
    B, H, Nq, Nk, D = case.B, case.H, case.Nq, case.Nk, case.H * 64
    if case.layout == "thirds":  # training's layout: q | k | v and dq | dk | dv as column thirds of [B, N, 3D] buffers
        assert Nq == Nk
        qkv = torch.zeros(B, Nq, 3 * D, device=dev, dtype=BF)
        for i, t in enumerate((x.q, x.k, x.v)):
            qkv[..., i * D:(i + 1) * D].copy_(t)
        q, k, v = (qkv[..., i * D:(i + 1) * D] for i in range(3))
        o, do = strided(x.o, D + 64), strided(x.do, D + 128)
        g = Guarded(B, Nq, 3 * D)
        outs, dq, dk, dv = [g], *(g.region[..., i * D:(i + 1) * D] for i in range(3))
    else:
        if case.layout == "distinct":  # eight pairwise different row strides, batch strides with slack
            rs = [D + 8 * m for m in (1, 2, 3, 5, 6)]
            q, k, v, o, do = (strided(t, s, slack_rows=3) for t, s in zip((x.q, x.k, x.v, x.o, x.do), rs))
            pads = (40, 64, 88)
        else:
            b0 = case.layout == "batch0"
            q, o, do = strided(x.q, D), strided(x.o, D), strided(x.do, D)
            k, v = strided(x.k, D, batch0=b0), strided(x.v, D, batch0=b0)
            pads = (0, 0, 0)
        outs = [Guarded(B, n, D, p) for n, p in zip((Nq, Nk, Nk), pads)]
        dq, dk, dv = (g.region for g in outs)
    strides = [t.stride(1) for t in (q, k, v, o, do, dq, dk, dv)]
    if case.layout == "distinct":
        assert len(set(strides)) == 8 and all(s % 8 == 0 for s in strides), strides
    if case.layout == "batch0":
        assert k.stride(0) == 0 and v.stride(0) == 0
    n = B * H * Nq
    dbuf = torch.full((n + 32,), math.nan, device=dev, dtype=torch.float32)
    delta = dbuf[16:16 + n].view(B, H, Nq)
    k_len = None if x.k_len is None else x.k_len.to(dev)
    args = dict(q=q, k=k, v=v, o=o, do=do, lse=x.lse.to(dev), dq=dq, dk=dk, dv=dv, k_len=k_len, delta=delta)
    K.attention_bwd(q, k, v, o, do, args["lse"], H, scale=case.scale, dq=dq, dk=dk, dv=dv, k_len=k_len, delta=delta)
    torch.cuda.synchronize()
    got = {"dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu(), "delta": delta.cpu()}
    for name, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), f"{case.id} {name}: non-finite result"
    assert all(g.guards_intact() for g in outs), f"{case.id}: a guard row or column of dq / dk / dv was written"
    delta.fill_(math.nan)
    assert bool((dbuf.view(torch.int32) == int(dbuf.view(torch.int32)[0])).all()), f"{case.id}: delta's guards"
    return got, args


def judge(case, got, tag=""):
    """the gate on dq, dk, dv and the per-element bound on delta; prints the worst ratio of each, names the worst row
    of a failing one"""
    ref = A.reference(case)
    res, bad = [], []
    for name in A.TENSORS:
        r, where = A.worst(A.gate(got[name], ref, name))
        # (reported, not asserted: the same error against the model of the kernel that writes this tensor, C = 1)
        own = A.worst(A.gate(got[name], ref, name, side="q" if name == "dq" else "k"))[0]
        res.append(f"{name} {r:.3f} (own side, C = 1: {own:.2f})")
        if not r <= 1.0:
            bad.append(f"{name}: worst row {where}: error / bound = {r:.3f}")
    r, where = A.worst(A.delta_gate(got["delta"], ref), rows_last=True)
    res.append(f"delta {r:.3f}")
    if not r <= 1.0:
        bad.append(f"delta: worst element {where}: error / bound = {r:.3f}")
    print(f"  {case.id}{tag}: worst error / bound: " + ", ".join(res))
    return bad


def zero_past_length(case, got):
    """rows at or past each length of dk / dv: exact zeros"""
    x = A.inputs(case)
    for b, L in enumerate(A.lengths(x.k_len, case.B, case.Nk)):
        for name in ("dk", "dv"):
            assert not got[name][b, L:].float().any(), f"{case.id} {name}: batch {b}, a row past length {L} is not zero"


def run(K, case, tag=""):
    got, args = launch(K, case, A.inputs(case))
    if case.k_len is not None:
        zero_past_length(case, got)
    return judge(case, got, tag), args


def descriptor(a, B, H, Nq, Nk, scale=0.125, head_dim=64):
    from videopainter_amd import _native as N_
    d = N_.AttnBwdDesc()
    d.B, d.H, d.Nq, d.Nk, d.head_dim, d.scale = B, H, Nq, Nk, head_dim, scale
    fields = {"q": "Q", "k": "K", "v": "V", "o": "O", "do": "dO", "dq": "dQ", "dk": "dK", "dv": "dV"}
    for n, f in fields.items():
        setattr(d, f, a[n].data_ptr())
        setattr(d, f"{n}_sb", a[n].stride(0))
        setattr(d, f"{n}_sn", a[n].stride(1))
    d.lse, d.delta = a["lse"].data_ptr(), a["delta"].data_ptr()
    if a.get("k_len") is not None:
        d.k_len = a["k_len"].data_ptr()
    return d


@pytest.mark.parametrize("Nk", A.LENGTHS)
def test_lengths(K, Nk):
    """Nq x Nk over {1, 31, 32, 33, 64, 65, 97, 128, 129, 200}^2 (one lane, the lim <= 32 half-skip, a full tile, a
    tile plus one key, a full block, a block plus one, two blocks with a ragged tile), two heads with gains 4 x apart"""
    bad = []
    for case in A.group("lengths"):
        if case.Nk == Nk:
            bad += [f"{case.id} {b}" for b in run(K, case)[0]]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", A.group("strides"), ids=lambda c: c.name)
def test_strides(K, case):
    """q | k | v and dq | dk | dv as column thirds of [B, N, 3D] buffers with o and dO on padded rows; eight pairwise
    different row strides with slack between batch rows; k and v as one batch row expanded with batch stride 0"""
    bad, _ = run(K, case)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", A.group("scale"), ids=lambda c: c.name)
def test_scale(K, case):
    bad, _ = run(K, case)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", A.group("score_range"), ids=lambda c: c.name)
def test_score_range(K, case):
    """gains up to 6 (scores over hundreds of log2 units); a key with 0.9992 of the mass of a quarter of the queries
    in the peeled partial tile / at keys 63, 64 and 639; the rows' lse spread over +-300"""
    bad, _ = run(K, case)
    assert not bad, "\n".join(bad)


def test_extra_mass(K):
    """lse carries 0.1 x .. 10 x the keys' own mass more (the closed-form null keys): P sums to less than one"""
    bad, _ = run(K, A.group("extra_mass")[0])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", A.group("k_len"), ids=lambda c: c.name)
def test_k_len(K, case):
    """k_len = 0, 1, 32, 63, 64, 128, Nk, above Nk / a negative entry: K and V rows at or past each length hold NaN, dk
    and dv start as NaN and come back as exact zeros past it"""
    bad, _ = run(K, case)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", A.group("tail_split"), ids=lambda c: c.name)
def test_tail_split_small(K, knobs, case):
    """the grid-tail split with many heads of few tokens, one kernel at a time (the other stays at <= 256 blocks), with
    k_len leaving pieces empty and tile counts the piece count does not divide; and the same unsplit"""
    from videopainter_amd import _native as N_
    bad, a = run(K, case, " (split)")
    nbytes = N_.lib().vp_attention_bwd_workspace_bytes(C.byref(descriptor(a, case.B, case.H, case.Nq, case.Nk)))
    assert nbytes > 0, f"{case.id}: the split is not active for this shape"
    # the plan the arm is shaped for: only the named kernel splits, its tail blocks in S = 4 pieces each (the other
    # dimension has 4 tiles: under k_len lengths of 1 and 3 tiles leave pieces empty / uneven).  One piece record is
    # 128 rows x 64 (dQ) or 128 (dK | dV) fp32
    rec = 128 * (128 if case.name == "dkdv" else 64) * 4
    blocks = case.B * case.H * (((case.Nk if case.name == "dkdv" else case.Nq) + 127) // 128)
    other = case.B * case.H * (((case.Nq if case.name == "dkdv" else case.Nk) + 127) // 128)
    tail = nbytes // (4 * rec)
    print(f"  {case.id}: workspace {nbytes} bytes = {tail} tail blocks of {blocks} x 4 pieces x {rec} bytes "
          f"(the other kernel: {other} blocks, unsplit)")
    assert nbytes == tail * 4 * rec and 0 < tail < blocks - tail and other <= 256, (nbytes, tail, blocks, other)
    knobs.setenv("VP_ATTN_NO_SPLIT", "1")
    assert N_.lib().vp_attention_bwd_workspace_bytes(C.byref(descriptor(a, case.B, case.H, case.Nq, case.Nk))) == 0
    bad += run(K, case, " (VP_ATTN_NO_SPLIT=1)")[0]
    assert not bad, "\n".join(bad)


def test_refusals(K, knobs):
    """the header's error codes, all returned before any launch"""
    from videopainter_amd import _native as N_
    L = N_.lib()
    B, H, Nq, Nk = 1, 1, 64, 64
    names = ("q", "k", "v", "o", "do", "dq", "dk", "dv")
    t = {n: torch.zeros(B, Nq, 72, device=dev, dtype=BF)[..., :64] for n in names}
    t["lse"] = torch.zeros(B, H, Nq, device=dev)
    t["delta"] = torch.zeros(B, H, Nq, device=dev)
    lens = torch.full((4,), Nk, device=dev, dtype=torch.int32)

    def rc(d):
        return L.vp_attention_bwd_bf16(C.byref(d), None), L.vp_attention_bwd_workspace_bytes(C.byref(d))

    assert L.vp_attention_bwd_workspace_bytes(C.byref(descriptor(t, B, H, Nq, Nk))) == 0  # (valid; too small to split)
    for field in ("q_sn", "k_sn", "v_sn", "o_sn", "do_sn", "dq_sn", "dk_sn", "dv_sn", "q_sb", "dv_sb"):
        d = descriptor(t, B, H, Nq, Nk)
        setattr(d, field, getattr(d, field) + 4)  # not a multiple of 8
        assert rc(d) == (N_.ERR_ARG, -1), field
    assert rc(descriptor(t, B, H, Nq, Nk, head_dim=128)) == (N_.ERR_UNSUPPORTED, -1)
    d = descriptor(t, B, H, Nq, Nk)
    d.k_len = lens.data_ptr() + 2  # not 4-byte aligned
    assert rc(d) == (N_.ERR_ARG, -1)
    d = descriptor(t, B, H, 0, Nk)
    assert rc(d) == (N_.ERR_ARG, -1)
    d = descriptor(t, B, H, Nq, Nk)
    d.dQ = None
    assert rc(d) == (N_.ERR_ARG, -1)
    knobs.setenv("VP_ATTN_BWD_VARIANT", "0")
    d = descriptor(dict(t, k_len=lens), B, H, Nq, Nk)
    assert L.vp_attention_bwd_bf16(C.byref(d), None) == N_.ERR_UNSUPPORTED
    torch.cuda.synchronize()
