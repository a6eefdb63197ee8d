"""One launch for the AdaLN modulation linears of a forward (vp_linear_small_batched_bf16), GPU only: bit-equal to
the per-block `modulation()` calls, and its cached pointer table follows the parameters."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _norms(G, K_, D):
    from videopainter_amd import device_scope
    from videopainter_amd.transformer import CogVideoXLayerNormZero
    g = torch.Generator().manual_seed(3)
    with device_scope(dev):
        norms = [CogVideoXLayerNormZero(K_, D) for _ in range(G)]
    with torch.no_grad():
        for n in norms:
            n.linear.weight.copy_(torch.randn(6 * D, K_, generator=g) * K_ ** -0.5)
            n.linear.bias.copy_(torch.randn(6 * D, generator=g) * 0.1)
    return norms, (torch.randn(2, K_, generator=g) * 2.0).to(dev, BF16)


@torch.no_grad()
def test_batched_modulations_bit_equal_and_table_follows_weights():
    """G = 5 groups, B = 2, K = 512, 6 D outputs with D = 128 (24 workgroups per group, the last columns of a
    workgroup's range in use): equal bit for bit to the five separate calls; after one weight tensor is replaced the
    cached table is rebuilt and the results follow the new weight."""
    from videopainter_amd import kernels as K
    norms, temb = _norms(5, 512, 128)
    lins = [n.linear for n in norms]
    holder = {}
    tab = K.LinearGroupTable.cached(holder, lins)
    got = K.linear_small_batched(temb, tab, act_in=K.ACT_SILU)
    assert tuple(got.shape) == (5, 2, 6 * 128) and got.dtype == BF16
    for g_, n in enumerate(norms):
        assert torch.equal(got[g_], n.modulation(temb)), g_
    assert K.LinearGroupTable.cached(holder, lins) is tab  # unchanged parameters: the cached table
    # a weight reload that replaces the tensor (new storage)
    old = norms[3].linear.weight
    norms[3].linear.weight = torch.nn.Parameter((old.float() * -0.5).to(BF16), requires_grad=False)
    assert norms[3].linear.weight.data_ptr() != old.data_ptr()
    tab2 = K.LinearGroupTable.cached(holder, lins)
    assert tab2 is not tab
    got2 = K.linear_small_batched(temb, tab2, act_in=K.ACT_SILU)
    for g_, n in enumerate(norms):
        assert torch.equal(got2[g_], n.modulation(temb)), g_
    assert not torch.equal(got2[3], got[3]) and torch.equal(got2[2], got[2])


@torch.no_grad()
def test_batched_modulations_odd_width_and_single_row():
    """N = 6 * 20 = 120 columns (not a multiple of the 32 columns of a workgroup), K = 32 (4 of 64 lanes hold a
    chunk), one input row."""
    from videopainter_amd import kernels as K
    norms, temb = _norms(3, 32, 20)
    got = K.linear_small_batched(temb[:1], K.LinearGroupTable([n.linear for n in norms]), act_in=K.ACT_SILU)
    for g_, n in enumerate(norms):
        assert torch.equal(got[g_], n.modulation(temb[:1])), g_


@torch.no_grad()
def test_model_forward_uses_the_batched_modulations(knobs):
    """The tiny transformer's output with the one-launch modulations equals, bit for bit, its output with every
    block computing its own (VP_MOD_BATCHED=0)."""
    from tests.golden.cases import TINY_CFG, tiny_inputs, tiny_weights
    from videopainter_amd import CogVideoXTransformer3DModel, device_scope
    tsd, _ = tiny_weights()
    with device_scope(dev):
        tr = CogVideoXTransformer3DModel(**TINY_CFG)
    tr.load_diffusers_state_dict({k: torch.from_numpy(v) for k, v in tsd.items()})
    i = tiny_inputs()
    kw = dict(hidden_states=i["hidden"].to(dev, BF16), encoder_hidden_states=i["enc"].to(dev, BF16),
              timestep=i["timestep"].to(dev), image_rotary_emb=i["rope"], return_dict=False)
    a = tr(**kw)[0]
    assert "_vp_linear_group_table" in tr.__dict__
    knobs.setenv("VP_MOD_BATCHED", "0")
    b = tr(**kw)[0]
    assert torch.equal(a, b)
