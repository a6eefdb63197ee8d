"""The fp8 path under the Ulysses head-parallel split (GPU only; P ranks as P threads of one process, ThreadComm):
the two kernels of its exchange byte for byte against the launches they replace — vp_qkv_heads_pack_fp8 against
vp_head_norm_rope_fp8 on each head group's columns, vp_mx_quantize_heads_bf16 against vp_mx_quantize_bf16 of the
re-laid-out tensor — and the split models against the unsplit fp8 forward of the same models.  The MX-FP8 AdaLN,
projections and FeedForward are row-local and the fp8 attention runs one workgroup per (batch, head, query block) over
all keys, so the split is expected to be bit-identical: the noise predictions are compared with torch.equal.

Sizes of tests/test_ulysses_gpu.py: 4 heads (D = 256), 10 text rows, N = 298 joint rows, B = 2 — at P = 4 shards of 75
rows, the last padded, ranks 1-3 without text rows; at P = 2 rank 0 holds text and video rows."""
import contextlib
import types

import numpy as np
import pytest
import torch

from tests import mx_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
T, NTOK, B = 10, 298, 2


def rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------
# the send packer
# ------------------------------------------------------------------------------------------------------------------

def _norm(g, scale=1.0):
    return types.SimpleNamespace(weight=(1.0 + 0.3 * torch.randn(64, generator=g)).mul(scale).to(dev).bfloat16(),
                                 bias=(0.2 * torch.randn(64, generator=g)).to(dev).bfloat16(), eps=1e-6)


def _pack_case(P, H, text_len, with_rope, ld_extra=0, n=75):
    from videopainter_amd import kernels as K
    g = torch.Generator().manual_seed(100 * P + H + text_len)
    D = H * 64
    Dp = D // P
    buf = (2.0 * torch.randn(B, n, 3 * D + ld_extra, generator=g)).to(dev).bfloat16()
    qkv = buf[..., :3 * D]
    nq, nk = _norm(g), _norm(g, 1.5)
    rope = None
    if with_rope:  # the shard's tables: its video rows, the last ones zero as `Shard.rope` pads them
        ang = 6.283 * torch.rand(n - text_len, 64, generator=g)
        cos, sin = torch.cos(ang), torch.sin(ang)
        cos[-3:] = 0.0
        sin[-3:] = 0.0
        rope = (cos.to(dev).contiguous(), sin.to(dev).contiguous())
    q_mul, k_mul = 0.125 * K.LOG2E * 2.0 ** 3, 2.0 ** 4
    send = K.qkv_heads_pack_fp8(qkv, H, P, text_len, nq, nk, rope, q_mul, k_mul)
    assert send.shape == (P, n, B, 4 * Dp) and send.dtype == torch.uint8
    hp = H // P
    for j in range(P):
        cols = slice(j * Dp, (j + 1) * Dp)
        q_ref = K.head_norm_rope_fp8(qkv[..., :D][..., cols], hp, text_len, nq.weight, nq.bias, nq.eps, rope, q_mul)
        k_ref = K.head_norm_rope_fp8(qkv[..., D:2 * D][..., cols], hp, text_len, nk.weight, nk.bias, nk.eps, rope,
                                     k_mul)
        chunk = send[j].transpose(0, 1)  # [B, n, 4 Dp]
        assert torch.equal(chunk[..., :Dp], q_ref), (j, "q")
        assert torch.equal(chunk[..., Dp:2 * Dp], k_ref), (j, "k")
        v = chunk[..., 2 * Dp:].contiguous().view(torch.bfloat16)
        assert torch.equal(v, qkv[..., 2 * D:][..., cols]), (j, "v")
    # (the e4m3 bytes are not all one value: the norm ran)
    assert send[0, :, :, :Dp].float().std() > 1.0


@pytest.mark.parametrize("with_rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("text_len", [0, 10])
@pytest.mark.parametrize("P,H", [(1, 4), (2, 4), (4, 4), (2, 8)])
def test_pack_kernel_matches_head_norm_rope_fp8(P, H, text_len, with_rope):
    """(1, 4): four heads per group, the norm kernel's 4-heads-per-lane-group path in the reference launch too;
    (4, 4): one head per group (its 1-head path); (2, 8): the 8-head qkv split two ways.  75 rows x 2 batches: more
    than one workgroup, the last one partly empty."""
    _pack_case(P, H, text_len, with_rope)


def test_pack_kernel_strided_rows():
    """A qkv view whose row stride exceeds 3 D (the first columns of a wider buffer)."""
    _pack_case(2, 4, 10, True, ld_extra=64)


def test_pack_kernel_rejects_bad_arguments():
    from videopainter_amd import kernels as K
    g = torch.Generator().manual_seed(1)
    qkv = torch.zeros(B, 8, 3 * 256, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        K.qkv_heads_pack_fp8(qkv, 4, 3, 0, _norm(g), _norm(g), None, 1.0, 1.0)       # 4 heads, 3 ways
    flat = torch.zeros(qkv.numel() + 8, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):  # rows that are only 8-byte aligned
        K.qkv_heads_pack_fp8(flat[4:4 + qkv.numel()].view(qkv.shape), 4, 2, 0, _norm(g), _norm(g), None, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        K.qkv_heads_pack_fp8(qkv, 4, 2, 0, _norm(g), _norm(g), None, 0.0, 1.0)       # a factor of 0


# ------------------------------------------------------------------------------------------------------------------
# the receive-side gather + MX quantiser
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,Dp,n", [(1, 256, 75), (2, 128, 75), (4, 64, 75), (4, 128, 150)])
def test_gather_quantise_matches_mx_quantize(P, Dp, n):
    """M = 150 rows sit inside one 256-row scale tile, M = 300 cross a tile boundary."""
    from videopainter_amd import kernels as K
    g = torch.Generator().manual_seed(7 * P + Dp + n)
    x = torch.randn(P, n, B, Dp, generator=g) * torch.exp2(torch.randint(-12, 9, (P, n, B, Dp // 32, 1),
                                                                         generator=g).float()).expand(
        P, n, B, Dp // 32, 32).reshape(P, n, B, Dp)
    x[0, 1, 0, :32] = 0.0  # an all-zero block: scale byte 0
    x = x.to(dev).bfloat16()
    M, Kk = B * n, P * Dp
    got = K.mx_quantize_heads(x)
    flat = x.permute(2, 1, 0, 3).reshape(M, Kk).contiguous()
    want = K.mx_quantize(flat)
    assert got.rows == M and got.K == Kk
    assert torch.equal(got.q[:M], want.q[:M])
    rr, kk = np.meshgrid(np.arange(M), np.arange(Kk // 32), indexing="ij")
    off = torch.from_numpy(mx_ref.scale_offset(rr, kk, Kk)).to(dev)
    assert torch.equal(got.scales[off], want.scales[off])
    # and the host reference of the format agrees (the quantiser really ran on the gathered rows)
    q_host, s_host = mx_ref.quantize(flat)
    assert torch.equal(got.q[:M].cpu(), q_host) and torch.equal(got.scales.cpu()[off.cpu()], s_host[off.cpu()])
    with pytest.raises(ValueError):
        K.mx_quantize_heads(x[..., :32].contiguous())  # not whole heads


# ------------------------------------------------------------------------------------------------------------------
# the split models
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def env():
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel, device_scope
    from videopainter_amd.embeddings import prepare_rotary_positional_embeddings
    from tests.golden.cases import TINY_CFG
    cfg = dict(TINY_CFG, num_attention_heads=4, max_text_seq_length=T, num_layers=3)
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**cfg)
        br = CogvideoXBranchModel(**dict(cfg, num_layers=2))
        trr = CogVideoXTransformer3DModel(**dict(cfg, id_pool_resample_learnable=True))
    tr.init_synthetic_weights_(11)
    br.init_synthetic_weights_(12)
    trr.init_synthetic_weights_(11)
    g = torch.Generator().manual_seed(13)
    F, H, W = 3, 16, 24
    video = torch.randn(B, F, 16, H, W, generator=g)
    mask = torch.zeros(B, F, 1, H, W)
    mask[:, 1:, :, 4:12, 6:18] = 1.0
    hidden = torch.cat([video, torch.randn(B, F, 16, H, W, generator=g)], 2)
    inp = dict(video=video.to(dev).bfloat16(), hidden=hidden.to(dev).bfloat16(),
               hidden2=(hidden + 0.5 * torch.randn(hidden.shape, generator=g)).to(dev).bfloat16(),
               cond=torch.cat([video * (1 - mask), mask], 2).to(dev).bfloat16(),
               enc=torch.randn(B, T, 32, generator=g).to(dev).bfloat16(), mask=mask.to(dev).bfloat16(),
               ts=torch.tensor([500, 500], device=dev),
               rope=tuple(t.to(dev) for t in prepare_rotary_positional_embeddings(H * 8, W * 8, F, 64)))
    return dict(tr=tr, br=br, trr=trr, inp=inp, refs={})


MODES = {"all": dict(), "attention": dict(ffn=False, qkv=False, out=False)}


@contextlib.contextmanager
def fp8(models, **switches):
    for m in models:
        m.enable_fp8(**switches)
    try:
        yield
    finally:
        for m in models:
            m.enable_fp8(False, False, False, False)


def _unsplit(env, mode):
    """The unsplit forward of branch + transformer in the models' current mode, computed once per mode."""
    if mode not in env["refs"]:
        i = env["inp"]
        with torch.no_grad():
            bs = env["br"](hidden_states=i["video"], encoder_hidden_states=i["enc"], branch_cond=i["cond"],
                           timestep=i["ts"], image_rotary_emb=i["rope"], return_dict=False)[0]
            ref, hs = env["tr"](hidden_states=i["hidden"], encoder_hidden_states=i["enc"], timestep=i["ts"],
                                image_rotary_emb=i["rope"], branch_block_samples=bs, branch_block_masks=i["mask"],
                                return_hidden_states=True, return_dict=False)[:2]
        env["refs"][mode] = (ref.clone(), [h.clone() for h in hs], [b.clone() for b in bs])
    return env["refs"][mode]


def _split(env, P):
    from videopainter_amd import ulysses as U
    i = env["inp"]
    comm = U.ThreadComm(P)

    def rank_fn(r):
        samples = U.branch_forward(env["br"], comm, r, i["video"], i["enc"], i["cond"], i["ts"], i["rope"])
        out, hsl = U.transformer_forward(env["tr"], comm, r, i["hidden"], i["enc"], i["ts"], i["rope"], samples,
                                         i["mask"], return_hidden_states=True)
        return out, hsl, samples

    return comm.run(rank_fn)


class _Calls:
    """Records every kernels.attention_fp8 call (heads, keyword names) while it is patched in."""

    def __init__(self, monkeypatch):
        from videopainter_amd import kernels as K
        self.calls = []
        real = K.attention_fp8

        def wrapped(q8, k8, vp, out, heads, *a, **kw):
            self.calls.append((heads, q8.shape[1], k8.shape[1], {k for k, v in kw.items() if v is not None}))
            return real(q8, k8, vp, out, heads, *a, **kw)
        monkeypatch.setattr(K, "attention_fp8", wrapped)


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("mode", list(MODES))
def test_fp8_split_matches_unsplit(env, monkeypatch, mode, P):
    from videopainter_amd import ulysses as U
    with fp8((env["tr"], env["br"]), **MODES[mode]):
        ref, hs, bs = _unsplit(env, mode)
        rec = _Calls(monkeypatch)
        res = _split(env, P)
    torch.cuda.synchronize()
    # the fp8 kernel ran in every block of both models on every rank, on the rank's H / P heads, every row of the
    # head group (padding included) against the N real keys
    nblk = len(env["tr"].transformer_blocks) + len(env["br"].transformer_blocks)
    n = -(-NTOK // P)
    assert len(rec.calls) == nblk * P, len(rec.calls)
    assert all(c[:3] == (4 // P, P * n, NTOK) for c in rec.calls), rec.calls[:3]
    for r, (out, hsl, samples) in enumerate(res):
        print(f"{mode} P={P} rank {r}: noise prediction rel {rel(out, ref):.2e}")
        assert out.shape == ref.shape and torch.equal(out, ref)
        sh = U.Shard(NTOK, T, P, r)
        for k, h in enumerate(hsl):
            assert rel(h[:, :sh.valid], hs[k][:, sh.r0:sh.r0 + sh.valid]) < 1e-3, (r, k)
        for j, s in enumerate(samples):
            k = max(0, min(sh.nv, NTOK - T - sh.v0))
            assert rel(s[:, :k], bs[j][:, sh.v0:sh.v0 + k]) < 1e-3, (r, j)
    assert all(torch.equal(res[0][0], o[0]) for o in res)


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("resample", [True, False], ids=["resample", "standard"])
def test_fp8_window_handoff(env, monkeypatch, P, resample):
    """The two cases of test_ulysses_any_length_window_handoff on fp8: the standard processor's prev-clip blend under
    enable_fp8() (the previous window's K | V cross in bf16 and are quantised on the head group), the ID-resample
    processor under enable_fp8(resample_attention=True) (bf16 exchange, the two-segment fp8 kernel per head group) —
    window 0 and the later window against the unsplit fp8 forward of the same model."""
    from videopainter_amd import ulysses as U
    i = env["inp"]
    tr = env["trr"] if resample else env["tr"]
    kw = dict(encoder_hidden_states=i["enc"], timestep=i["ts"], image_rotary_emb=i["rope"],
              branch_block_masks=i["mask"], id_pool_resample_learnable=resample, return_dict=False)
    with fp8((tr,), resample_attention=resample):
        key = ("handoff", resample)
        if key not in env["refs"]:
            with torch.no_grad():
                bs = env["br"](hidden_states=i["video"], encoder_hidden_states=i["enc"], branch_cond=i["cond"],
                               timestep=i["ts"], image_rotary_emb=i["rope"], return_dict=False)[0]
                ref0, hs0, rm0 = tr(hidden_states=i["hidden"], branch_block_samples=bs, return_hidden_states=True,
                                    return_resample_mask=True, **kw)
                ref1 = tr(hidden_states=i["hidden2"], branch_block_samples=bs,
                          attention_kwargs={"prev_hidden_states": dict(enumerate(hs0)), "prev_clip_weight": 0.5,
                                            "prev_resample_mask": rm0}, **kw)[0]
            env["refs"][key] = (ref0.clone(), ref1.clone(), rm0.clone())
        ref0, ref1, rm0 = env["refs"][key]
        comm = U.ThreadComm(P)

        def rank_fn(r):
            samples = U.branch_forward(env["br"], comm, r, i["video"], i["enc"], i["cond"], i["ts"], i["rope"])
            out0, hsl = U.transformer_forward(tr, comm, r, i["hidden"], i["enc"], i["ts"], i["rope"], samples,
                                              i["mask"], return_hidden_states=True,
                                              id_pool_resample_learnable=resample)
            out1 = U.transformer_forward(tr, comm, r, i["hidden2"], i["enc"], i["ts"], i["rope"], samples, i["mask"],
                                         id_pool_resample_learnable=resample,
                                         prev_hidden_states=dict(enumerate(hsl)), prev_clip_weight=0.5,
                                         prev_resample_mask=rm0)[0]
            return out0, out1

        rec = _Calls(monkeypatch)
        res = comm.run(rank_fn)
    torch.cuda.synchronize()
    nblk = len(tr.transformer_blocks)
    # per rank and block: window 0 one call; the later window one two-segment call (resample) or the blend's two
    assert len(rec.calls) == nblk * P * (2 if resample else 3), len(rec.calls)
    assert all(c[0] == 4 // P for c in rec.calls)
    if resample:  # the two-segment launch: the masked keys, their pack, the count, the null-key mass
        assert all({"k2", "vp2", "k2_len", "l_extra"} <= c[3] for c in rec.calls), rec.calls[0]
    for r, (out0, out1) in enumerate(res):
        print(f"P={P} {'resample' if resample else 'standard'} rank {r}: window 0 rel {rel(out0, ref0):.2e}, "
              f"window 1 rel {rel(out1, ref1):.2e}")
        assert torch.equal(out0, ref0) and torch.equal(out1, ref1), r


def test_back_to_bf16(env):
    """The switches cleared after an fp8 split forward: the split is the bf16 one again, bit for bit."""
    with fp8((env["tr"], env["br"])):
        res8 = _split(env, 2)
    ref, _, _ = _unsplit(env, "bf16")
    res = _split(env, 2)
    for (out, _, _), (out8, _, _) in zip(res, res8):
        assert torch.equal(out, ref)
        assert not torch.equal(out8, ref)  # (the fp8 forward was a different one)
