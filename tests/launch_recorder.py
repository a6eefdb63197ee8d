"""The launch recorder of the CPU launch-trace tests (tests/test_block_launches_cpu.py, test_model_launches_cpu.py,
test_block_backward_launches_cpu.py): the `videopainter_amd.kernels` entry points a block's forward and backward or a
whole model forward call are replaced, INSIDE THOSE TESTS
ONLY, by recorders that log the entry, every scalar argument, and shape / strides / dtype of every tensor argument, and
return their `out` argument (or an empty tensor of the documented shape).  The product path has no such substitute.

A thread may redirect what it records into a list of its own (`into`): the ranks of a `ulysses.ThreadComm` are threads,
and each rank's trace is compared on its own.
"""
import contextlib
import inspect
import threading

import torch


class _Table:  # what LinearGroupTable.cached returns, without a device (the real one takes device pointers)
    def __init__(self, linears):
        self.G, (self.N, self.K) = len(linears), linears[0].weight.shape


def _describe(v):
    if isinstance(v, torch.Tensor):
        return {"shape": list(v.shape), "stride": list(v.stride()), "dtype": str(v.dtype).replace("torch.", "")}
    if isinstance(v, torch.nn.Module):
        return {"module": type(v).__name__, "eps": getattr(v, "eps", None),
                "params": [_describe(p) for p in v.parameters()]}
    if isinstance(v, _Table):
        return {"table": [v.G, v.N, v.K]}
    if isinstance(v, (list, tuple)):
        d = [_describe(e) for e in v]
        return {"rope": d, "grid": _describe(v.grid)} if hasattr(v, "grid") else d
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"recorder: unexpected argument {type(v)}")


def _empty(*shape, like, dtype=torch.bfloat16):
    return torch.empty(*shape, device=like.device, dtype=dtype)


def _tokens(a, src):
    B, F, _, H, W = a[src].shape
    return B, F * (H // a["p"]) * (W // a["p"])


def _rows(t):
    return t.numel() // t.shape[-1]


# what an entry returns when it is given no `out`: an empty tensor of the documented shape
_RETURNS = {
    "gemm": lambda a: a["out"],
    "adaln_modulate": lambda a: a["out"] if a["out"] is not None else torch.empty_like(a["x"]),
    "attention": lambda a: a["out"],
    "attention_merge": lambda a: a["out"],
    "linear_small": lambda a: a["out"] if a["out"] is not None else _empty(a["x"].shape[0], a["weight"].shape[0],
                                                                          like=a["x"]),
    "head_norm_rope": lambda a: a["x_out"],
    "mask_scale_rows": lambda a: a["out"],
    "partition_rows_index": lambda a: (_empty(*a["tok_mask"].shape, like=a["tok_mask"], dtype=torch.int32),
                                       _empty(a["tok_mask"].shape[0], like=a["tok_mask"], dtype=torch.int32)),
    # a whole model forward's
    "timestep_embedding": lambda a: _empty(a["timesteps"].shape[0], a["dim"], like=a["timesteps"]),
    "patchify": lambda a: _empty(_tokens(a, "src1")[0] * _tokens(a, "src1")[1], a["kpad"], like=a["src1"]),
    "patch_mask": lambda a: torch.zeros(*_tokens(a, "mask"), device=a["mask"].device, dtype=torch.uint8),
    "linear_small_batched": lambda a: _empty(a["table"].G, a["x"].shape[0], a["table"].N, like=a["x"]),
    "linear": lambda a: a["out"] if a["out"] is not None else _empty(*a["x"].shape[:-1], a["weight"].shape[0],
                                                                    like=a["x"]),
    "final_norm": lambda a: a["out"] if a["out"] is not None else _empty(
        a["x"].shape[0], a["x"].shape[1] - a["text_len"], a["x"].shape[2], like=a["x"]),
    "unpatchify": lambda a: _empty(a["B"], a["F"], a["Cout"], a["H"], a["W"], like=a["proj"]),
    "guide_rows": lambda a: a["x"],
    "mask_null_segments": lambda a: (_empty(a["tok_mask"].shape[0] * a["grid"][0] * a["grid"][1], 16,
                                            like=a["tok_mask"], dtype=torch.uint8),
                                     _empty(a["tok_mask"].shape[0] * (a["grid"][0] + 1), like=a["tok_mask"],
                                            dtype=torch.int32)),
    "null_key_mass": lambda a: _empty(a["q"].shape[0], a["heads"], a["q"].shape[1], like=a["q"], dtype=torch.float32),
    # a block's backward
    "attention_bwd": lambda a: tuple(a[d] if a[d] is not None else _empty(*a[s].shape, like=a[s])
                                     for d, s in (("dq", "q"), ("dk", "k"), ("dv", "v"))),
    "rowscale": lambda a: a["out"],
    "adaln_bwd": lambda a: a["dx"],
    "colsum": lambda a: a["out"] if a["out"] is not None else _empty(
        _rows(a["a"]) // (a["tokens_per_batch"] or _rows(a["a"])), 2, a["a"].shape[-1], like=a["a"],
        dtype=torch.float32),
    "wgrad": lambda a: _empty(a["dy"].shape[-1], a["x"].shape[-1], like=a["dy"]),
    "transpose": lambda a: a["out"] if a["out"] is not None else _empty(
        a["x"].shape[-1], -(-_rows(a["x"]) // a["pad_to"]) * a["pad_to"], like=a["x"]),
    "axpy": lambda a: a["out"] if a["out"] is not None else torch.empty_like(a["a"]),
    "silu": lambda a: torch.empty_like(a["x"]),
    "silu_bwd": lambda a: torch.empty_like(a["x"]),
    "head_norm_rope_bwd": lambda a: a["dx"],
    "gather_add_rows": lambda a: a["y"],
    "null_key_mass_bwd": lambda a: a["dq"],
}


class _Event:  # (the resample processor's mask plan orders its reuse with a device event: none on the CPU)
    def record(self, stream=None):
        pass


class _Stream:
    def wait_event(self, event):
        pass


_OWN = threading.local()


@contextlib.contextmanager
def into(log: list):
    """The calling thread's launches go to `log` instead of the list `recording()` yielded."""
    _OWN.log = log
    try:
        yield log
    finally:
        _OWN.log = None


@contextlib.contextmanager
def recording():
    """Replaces the kernel entry points with recorders; yields the list they append to.  Arguments are bound to the
    real entry's signature with its defaults applied, so a default passed explicitly records like one left out.
    Host-side helpers that need the device or the library (the batched linears' pointer table, the null-key kernels'
    size predicates) are replaced too, unrecorded: they are no launches."""
    from videopainter_amd import kernels as K
    log, saved = [], {}

    def recorder(name, real):
        sig = inspect.signature(real)

        def rec(*args, **kw):
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            own = getattr(_OWN, "log", None)
            (log if own is None else own).append({"entry": name,
                                                  "args": {k: _describe(v) for k, v in ba.arguments.items()}})
            return _RETURNS[name](ba.arguments)
        return rec

    patches = [(K, n, recorder(n, getattr(K, n))) for n in _RETURNS]
    patches += [(torch.cuda, "Event", _Event), (torch.cuda, "current_stream", lambda device=None: _Stream()),
                (K.LinearGroupTable, "cached", staticmethod(lambda holder, linears: _Table(linears))),
                (K, "null_key_mass_supported", lambda grid: True),
                (K, "null_key_mass_bwd_supported", lambda grid: True)]
    try:
        for obj, n, f in patches:
            saved[(obj, n)] = obj.__dict__[n] if isinstance(obj, type) else getattr(obj, n)
            setattr(obj, n, f)
        yield log
    finally:
        for (obj, n), f in saved.items():
            setattr(obj, n, f)
