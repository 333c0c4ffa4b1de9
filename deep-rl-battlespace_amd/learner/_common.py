"""What more than one kernel family of the learner package uses: the ranges of the hyper-parameters, the current stream, the address of
an optional tensor, a float32 allocator, the check of a one-element int64 device word, and the capture of an update as one graph."""
import torch

from .._args import _need, _number

# the ranges of the hyper-parameters, stated once: ppo_head, td_head, adam_hyper, both learners and their set_lr all check through _hyper
_SHARE = (lambda x: 0.0 < x < 1.0, "a number in (0, 1)")
_WEIGHT = (lambda x: x >= 0.0, "a number >= 0")
_POSITIVE = (lambda x: x > 0.0, "a number > 0")
_BETA = (lambda x: 0.0 <= x < 1.0, "a number in [0, 1)")
_UNIT = (lambda x: 0.0 <= x <= 1.0, "a number in [0, 1]")
_HYPER = {"clip": _SHARE, "c_v": _WEIGHT, "c_e": _WEIGHT, "temperature": _POSITIVE, "vclip": _POSITIVE, "lr": _WEIGHT, "betas[0]": _BETA,
          "betas[1]": _BETA, "eps": _WEIGHT, "max_grad_norm": _WEIGHT, "tau": _UNIT, "gamma": _UNIT}       # (max_grad_norm 0: adam_hyper's spelling of "no clipping")


def _hyper(name, x, rng=None):
    return _number(x, name, *(rng or _HYPER[name]))


_U64 = (1 << 64) - 1                                            # a seed or a sequence number as the uint64 the C entries take


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(x):
    """The address of an optional tensor: None (NULL) for None."""
    return x.data_ptr() if x is not None else None


def _f32(make, dev):
    """make: torch.empty or torch.zeros -> f(*shape), a float32 tensor of that shape on dev."""
    return lambda *shape: make(shape, dtype=torch.float32, device=dev)


def _int64_word(x, name, dev, anchor):
    """x must be an int64 tensor of ONE element (of any shape), contiguous, on dev: a counter the kernels read on the device."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    _need(x, name, tuple(x.shape) if x.numel() == 1 else (1,), (torch.int64,), dev, anchor)


def _capture(run, state, dev):
    """run() recorded as one graph on one stream -> the graph.  One eager run() goes first as the warm-up (buffers, kernel modules)
    and is undone: the tensors of state() -- every tensor a run writes that outlives it -- are bit for bit what they were."""
    with torch.no_grad():
        keep = [t.detach().clone() for t in state()]
        run()
        for t, k in zip(state(), keep):
            t.detach().copy_(k)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    return graph
