"""The launch sequences of a whole model forward on the CPU: `CogVideoXTransformer3DModel.forward` and
`CogvideoXBranchModel.forward` in their inference forms, and the head-parallel split of both (`ulysses.branch_forward`,
`ulysses.transformer_forward`, the `UlyssesModels` call form) on every rank at P = 1, 2 and 4, issue the kernel launches
recorded from the commit BEFORE the split's forwards became the models' own forward bodies
(tests/golden/model_launches.json) — entry, every scalar argument, and shape / strides / dtype of every tensor argument.

The recorder is tests/launch_recorder.py (the block test's).  Under `ThreadComm` the ranks are threads: each records
into lists of its own, and the traces are compared per rank.

The size is that of tests/test_ulysses_gpu.py with fewer layers: 10 text rows, 298 joint rows, so at P = 4 rank 0 holds
text and video rows and the last shard is padded (300 rows).

To record the fixture (against a checkout of the commit the traces are to be compared with, from its root):
    python -c "from tests.test_model_launches_cpu import write_fixture; write_fixture('model_launches.json')"
"""
import json
import os

import pytest
import torch

from tests.launch_recorder import into, recording

GOLD = os.path.join(os.path.dirname(__file__), "golden", "model_launches.json")
B, F, HL, WL, T = 2, 3, 16, 24, 10
NV = F * (HL // 2) * (WL // 2)
RANKS = (1, 2, 4)


def _models():
    from tests.golden.cases import TINY_CFG
    from videopainter_amd import CogVideoXTransformer3DModel, CogvideoXBranchModel
    cfg = dict(TINY_CFG, num_attention_heads=4, max_text_seq_length=T, num_layers=2)
    tr = CogVideoXTransformer3DModel(**cfg).init_synthetic_weights_(11)
    trr = CogVideoXTransformer3DModel(**dict(cfg, id_pool_resample_learnable=True)).init_synthetic_weights_(11)
    br = CogvideoXBranchModel(**dict(cfg, num_layers=1)).init_synthetic_weights_(12)
    brw = CogvideoXBranchModel(**dict(cfg, num_layers=1, wo_text=True)).init_synthetic_weights_(12)
    return tr, trr, br, brw


def _inputs():
    from videopainter_amd.embeddings import prepare_rotary_positional_embeddings
    g = torch.Generator().manual_seed(13)
    bf = torch.bfloat16
    video = torch.randn(B, F, 16, HL, WL, generator=g)
    mask = torch.zeros(B, F, 1, HL, WL)
    mask[:, 1:, :, 4:12, 6:18] = 1.0
    return dict(video=video.to(bf), hidden=torch.cat([video, torch.randn(B, F, 16, HL, WL, generator=g)], 2).to(bf),
                cond=torch.cat([video * (1 - mask), mask], 2).to(bf), enc=torch.randn(B, T, 32, generator=g).to(bf),
                mask=mask.to(bf), ts=torch.tensor([500, 500]),
                rope=tuple(prepare_rotary_positional_embeddings(HL * 8, WL * 8, F, 64)))


def record_all() -> dict:
    """{case: [launch, ...]} of every case, from the code importable as `videopainter_amd`."""
    from videopainter_amd import attention_processor as AP
    from videopainter_amd import ulysses as U
    tr, trr, br, brw = _models()
    i = _inputs()
    out = {}

    def run(name, fn):
        AP._MASK_PLANS.clear()  # (a trace holds the mask plan's launches: never found from a case before)
        with recording() as log, torch.no_grad():
            res = fn()
        out[name] = log
        return res

    # -- the single-GPU branch --
    bkw = dict(hidden_states=i["video"], encoder_hidden_states=i["enc"], branch_cond=i["cond"], timestep=i["ts"],
               image_rotary_emb=i["rope"], return_dict=False)
    bs = run("b_plain", lambda: br(**bkw))[0]
    run("b_scale", lambda: br(conditioning_scale=0.5, **bkw))
    run("b_wo_text", lambda: brw(wo_text=True, **bkw))

    # -- the single-GPU transformer --
    kw = dict(hidden_states=i["hidden"], encoder_hidden_states=i["enc"], timestep=i["ts"], image_rotary_emb=i["rope"],
              branch_block_samples=bs, return_dict=False)
    run("t_plain", lambda: tr(branch_block_masks=i["mask"], **kw))
    run("t_add_first", lambda: tr(branch_block_masks=i["mask"], add_first=True, **kw))
    _, hs0, rm0 = run("t_states_and_mask", lambda: tr(branch_block_masks=i["mask"], return_hidden_states=True,
                                                      return_resample_mask=True, **kw))
    later = {"prev_hidden_states": dict(enumerate(hs0)), "prev_clip_weight": 0.5, "prev_resample_mask": rm0}
    run("t_later_dict", lambda: tr(branch_block_masks=i["mask"], attention_kwargs=later, **kw))
    run("t_later_tensor", lambda: tr(branch_block_masks=i["mask"],
                                     attention_kwargs=dict(later, prev_hidden_states=hs0[0]), **kw))
    run("t_resample_w0", lambda: trr(branch_block_masks=i["mask"], id_pool_resample_learnable=True,
                                     return_hidden_states=True, return_resample_mask=True, **kw))
    run("t_resample_later", lambda: trr(branch_block_masks=i["mask"], id_pool_resample_learnable=True,
                                        attention_kwargs=later, **kw))
    guide = [torch.zeros(B, NV, 256, dtype=torch.bfloat16) for _ in tr.transformer_blocks]
    run("t_guided_masks", lambda: tr(branch_block_masks=i["mask"], self_guidance_hidden_states=guide, **kw))
    run("t_guided_own_masks", lambda: tr(self_guidance_hidden_states=guide, self_guidance_masks=i["mask"], **kw))
    run("t_cfg_shared", lambda: tr(branch_block_masks=i["mask"], cfg_shared_video=True, **kw))

    # -- the split: every rank's branch, window 0 and a later window, with both processors --
    pos = (i["enc"], i["ts"], i["rope"])
    for P in RANKS:
        comm = U.ThreadComm(P)
        for proc, model in (("standard", tr), ("resample", trr)):
            rs = proc == "resample"
            prev_masks = [rm0.clone() for _ in range(P)]  # (one tensor per rank, as one process per rank holds)

            def rank_fn(r):
                with into([]) as lb:
                    smp = U.branch_forward(br, comm, r, i["video"], i["enc"], i["cond"], *pos[1:])
                with into([]) as l0:
                    _, hsl = U.transformer_forward(model, comm, r, i["hidden"], *pos, smp, i["mask"],
                                                   return_hidden_states=True, id_pool_resample_learnable=rs)
                with into([]) as l1:
                    U.transformer_forward(model, comm, r, i["hidden"], *pos, smp, i["mask"],
                                          id_pool_resample_learnable=rs, prev_hidden_states=dict(enumerate(hsl)),
                                          prev_clip_weight=0.5, prev_resample_mask=prev_masks[r])
                return lb, l0, l1

            for r, (lb, l0, l1) in enumerate(run(f"s_P{P}_{proc}", lambda: comm.run(rank_fn))):
                if not rs:  # (the branch does not know the transformer's processor)
                    out[f"s_P{P}_r{r}_branch"] = lb
                out[f"s_P{P}_r{r}_{proc}_w0"], out[f"s_P{P}_r{r}_{proc}_later"] = l0, l1
            assert out.pop(f"s_P{P}_{proc}") == []  # every launch went to its rank's lists

    # -- the harness's call form, with the returned resample mask --
    comm = U.ThreadComm(2)

    def view_fn(r):
        m = U.UlyssesModels(tr, br, comm, rank=r)
        with into([]) as lv:
            smp = m.branch(**bkw)[0]
            m.transformer(branch_block_masks=i["mask"], return_hidden_states=True, return_resample_mask=True,
                          **dict(kw, branch_block_samples=smp))
        return lv

    for r, lv in enumerate(run("v", lambda: comm.run(view_fn))):
        out[f"v_P2_r{r}_call_forms"] = lv
    assert out.pop("v") == []
    return out


def case_names():
    names = ["b_plain", "b_scale", "b_wo_text", "t_plain", "t_add_first", "t_states_and_mask", "t_later_dict",
             "t_later_tensor", "t_resample_w0", "t_resample_later", "t_guided_masks", "t_guided_own_masks",
             "t_cfg_shared", "v_P2_r0_call_forms", "v_P2_r1_call_forms"]
    for P in RANKS:
        for r in range(P):
            names += [f"s_P{P}_r{r}_branch"] + [f"s_P{P}_r{r}_{proc}_{w}" for proc in ("standard", "resample")
                                               for w in ("w0", "later")]
    return names


def write_fixture(path: str = GOLD) -> None:
    """The traces repeat most launches (a layer's in the next layer, a rank's on the next rank): the fixture holds
    every distinct launch once, one per line, and each case as indices into them."""
    launches, index, cases = [], {}, {}
    for name, log in record_all().items():
        keys = [json.dumps(l, sort_keys=True) for l in log]
        for k in keys:
            if k not in index:
                index[k] = len(launches)
                launches.append(k)
        cases[name] = [index[k] for k in keys]
    with open(path, "w") as f:
        f.write('{"cases": {\n' + ",\n".join(f"{json.dumps(n)}: {json.dumps(cases[n])}" for n in sorted(cases))
                + '\n},\n"launches": [\n' + ",\n".join(launches) + "\n]}\n")


# ------------------------------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def traces():
    return json.loads(json.dumps(record_all()))  # (tuples -> lists, as the fixture went through JSON)


@pytest.fixture(scope="module")
def golden():
    with open(GOLD) as f:
        g = json.load(f)
    return {name: [g["launches"][k] for k in idx] for name, idx in g["cases"].items()}


def test_same_cases_as_the_fixture(traces, golden):
    assert sorted(traces) == sorted(golden) == sorted(case_names())


@pytest.mark.parametrize("case", case_names())
def test_trace_equals_the_recorded_one(traces, golden, case):
    got, want = traces[case], golden[case]
    if case.endswith("call_forms"):
        # the one launch that left with the refactor: the recorded view patchified the masks a second time after its
        # forward, for the resample mask it returns; it now returns the one its forward built
        assert want[-1]["entry"] == "patch_mask" and want[-1] in want[:-1]
        want = want[:-1]
    assert [l["entry"] for l in got] == [l["entry"] for l in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: launch {k} ({g['entry']}) differs"


def _core(trace):
    """A trace without what the design lets the split and the single-GPU forward differ in (the modulation launches
    leave; their number is returned):
      * the split computes each block's modulations itself (two linear_small per block), the single-GPU forward all of
        them in one linear_small_batched;
      * the split's blocks hand the AdaLN no output buffer (the `attend` hook projects q | k | v itself, so there is no
        K-augmented operand to write into) — the launch is the same, `out` is allocated by the entry;
      * the split's row-local RoPE table is a slice of the whole one and carries no video grid;
      * the split injects the branch's shard samples as the views they are, the single-GPU forward copies the samples
        to contiguous bf16 first: the strides of `inject` differ.
    Not visible in a trace: the split passes the blocks no ping-pong `out` buffer, has no self-guidance and no
    cfg_shared_video, pads the last shard with zero rows (none at P = 1), runs each branch output linear right after
    its block (one branch layer here), and norms the previous window's K per head group on the whole rows."""
    core = []
    for l in trace:
        if l["entry"] in ("linear_small", "linear_small_batched"):
            continue
        a = dict(l["args"])
        if l["entry"] == "adaln_modulate":
            a.pop("out")
        if l["entry"] == "gemm":
            if isinstance(a["rope"], dict):
                a["rope"] = a["rope"]["rope"]
            for k in ("inject_ld", "inject_bstride"):
                a.pop(k)
            if a["inject"] is not None:
                a["inject"] = dict(a["inject"], stride=None)
        core.append({"entry": l["entry"], "args": a})
    return core, sum(l["entry"] == "linear_small" for l in trace), \
        sum(l["entry"] == "linear_small_batched" for l in trace)


@pytest.mark.parametrize("single, split, layers", [
    ("b_plain", "s_P1_r0_branch", 1), ("t_states_and_mask", "s_P1_r0_standard_w0", 2),
    ("t_later_dict", "s_P1_r0_standard_later", 2), ("t_resample_w0", "s_P1_r0_resample_w0", 2),
    ("t_resample_later", "s_P1_r0_resample_later", 2)])
def test_one_rank_split_is_the_single_gpu_forward(traces, single, split, layers):
    """At P = 1 the split issues the single-GPU forward's launches, except for the listed disagreements (_core)."""
    a, a_small, a_batched = _core(traces[single])
    b, b_small, b_batched = _core(traces[split])
    assert a == b
    assert (a_batched, b_batched) == (1, 0) and b_small - a_small == 2 * layers
