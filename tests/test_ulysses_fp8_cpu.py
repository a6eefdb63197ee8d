"""The fp8 exchange format of the head-parallel split on the CPU (no native library): `ulysses.heads_fp8_views`
turns the first all-to-all's receive buffer uint8 [P, n, B, 4 Dp] into the attention's q8 / k8 / v operands as strided
views, checked on buffers filled by a torch packer written here (the layout vp_qkv_heads_pack_fp8 documents:
per head group, row, batch: q bytes | k bytes | v bf16) and carried through `ThreadComm.all_to_all`."""
import pytest
import torch

B, N, H = 2, 298, 4
D = H * 64


def pack(q8, k8, v, P):
    """Shard tensors q8 / k8 uint8 [B, n, D] and v bf16 [B, n, D] -> the send buffer uint8 [P, n, B, 4 Dp]."""
    n, Dp = q8.shape[1], D // P
    send = torch.empty(P, n, B, 4 * Dp, dtype=torch.uint8)
    for j in range(P):
        cols = slice(j * Dp, (j + 1) * Dp)
        send[j, :, :, :Dp] = q8[:, :, cols].transpose(0, 1)
        send[j, :, :, Dp:2 * Dp] = k8[:, :, cols].transpose(0, 1)
        send[j, :, :, 2 * Dp:] = v[:, :, cols].transpose(0, 1).contiguous().view(torch.uint8)
    return send


@pytest.fixture(scope="module")
def full():
    g = torch.Generator().manual_seed(5)
    q8 = torch.randint(0, 256, (B, N, D), generator=g, dtype=torch.uint8)
    k8 = torch.randint(0, 256, (B, N, D), generator=g, dtype=torch.uint8)
    v = torch.randn(B, N, D, generator=g).bfloat16()
    return q8, k8, v


@pytest.mark.parametrize("P", [1, 2, 4])
def test_receive_views_through_thread_comm(full, P):
    from videopainter_amd import ulysses as U
    q8, k8, v = full
    n, Dp = -(-N // P), D // P
    assert n == {1: 298, 2: 149, 4: 75}[P]
    comm = U.ThreadComm(P)

    def rank_fn(r):
        sh = U.Shard(N, 10, P, r)
        send = pack(sh.rows(q8), sh.rows(k8), sh.rows(v), P)
        recv = comm.all_to_all(r, send)
        assert recv.shape == send.shape and recv.dtype == torch.uint8
        # the exchange moves chunks whole: chunk j of the result is the sender j's chunk for this rank
        return send, recv, U.heads_fp8_views(recv, N)

    res = comm.run(rank_fn)
    for r, (send, recv, (rq, rk, rv)) in enumerate(res):
        for j in range(P):
            assert torch.equal(recv[j], res[j][0][r])
        cols = slice(r * Dp, (r + 1) * Dp)
        assert rq.shape == (B, P * n, Dp) and rk.shape == (B, N, Dp) and rv.shape == (B, N, Dp)
        assert rq.dtype == rk.dtype == torch.uint8 and rv.dtype == torch.bfloat16
        # every row of this rank's head group, in row order; q8 also carries the last shard's zero padding
        assert torch.equal(rq[:, :N], q8[:, :, cols]) and not rq[:, N:].any()
        assert torch.equal(rk, k8[:, :, cols])
        assert torch.equal(rv, v[:, :, cols])
        # views of the receive buffer, no copy: the same storage, a contiguous last dimension, 16-byte strides
        for t in (rq, rk, rv):
            assert t.untyped_storage().data_ptr() == recv.untyped_storage().data_ptr()
            assert t.stride(-1) == 1
            assert all(s * t.element_size() % 16 == 0 for s in t.stride()[:-1])
            assert t.storage_offset() * t.element_size() % 16 == 0
        assert rq.stride(1) * rq.element_size() == B * 4 * Dp and rq.stride(0) == 4 * Dp
        assert rv.stride(1) * rv.element_size() == B * 4 * Dp and rv.stride(0) * rv.element_size() == 4 * Dp
        # writing through the buffer shows in the views
        recv[0, 0, 1, 0] ^= 0xFF
        assert rq[1, 0, 0] == recv[0, 0, 1, 0]


def test_receive_views_reject_other_buffers():
    from videopainter_amd import ulysses as U
    with pytest.raises(ValueError):
        U.heads_fp8_views(torch.zeros(2, 5, 2, 4 * 64).bfloat16(), 8)        # not bytes
    with pytest.raises(ValueError):
        U.heads_fp8_views(torch.zeros(2, 5, 2, 4 * 32, dtype=torch.uint8), 8)  # not whole heads
    with pytest.raises(ValueError):
        U.heads_fp8_views(torch.zeros(2, 5, 4 * 64, 2, dtype=torch.uint8).transpose(2, 3), 8)  # not contiguous
