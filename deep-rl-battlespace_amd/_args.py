"""Argument checks of the learner-side bindings (advantage.py, learner/): one tensor check, one number check, one workspace helper."""
import math

import torch

_F32, _FLAG = (torch.float32,), (torch.uint8, torch.bool)


def _need(x, name, shape, dtypes, dev, anchor):
    """x must be a contiguous tensor of `shape`, of one of `dtypes`, on `dev` -- the device of the call's first tensor, named `anchor`."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if x.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(x.shape)}")
    if x.device != dev:
        raise ValueError(f"{name} is on {x.device}, {anchor} on {dev}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _number(x, name, ok, what):
    """float(x), which must be finite and pass ok(); `what` words the range for the message."""
    try:
        x = float(x)
        good = ok(x) and math.isfinite(x)
    except (TypeError, ValueError):
        good = False
    if not good:
        raise ValueError(f"{name} must be {what}, got {x!r}")
    return x


def _workspace(ws, nbytes, dev):
    """A workspace of at least `nbytes` bytes on `dev`, 8-byte aligned: a new one (ws None), or the caller's after a check."""
    if ws is None:
        return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    if not isinstance(ws, torch.Tensor) or ws.device != dev or not ws.is_contiguous() or ws.numel() * ws.element_size() < nbytes:
        raise ValueError(f"workspace must be a contiguous tensor of at least {nbytes} bytes on {dev}")
    return ws
