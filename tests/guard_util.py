"""Guard slabs for the tests that a device call writes nothing outside its buffers: every buffer of the call is the inner view of a
larger allocation whose bytes before and after it hold a sentinel, checked after the calls.  Also make_layout (csrc/bsx_state.h)
restated, for the state block's alignment padding."""
import math

import torch

SENTINEL = 0xA5
STATE_PAD = 32768        # guard bytes on either side of a state block: more than the widest stray first-row load a layout ever allowed


def slab(n, dtype, fill, pad=256):
    """A tensor of n elements with `pad` guard elements on either side: (whole slab, the inner view)."""
    t = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
    return t, t[pad:pad + n]


def guards_intact(slab, fill, n, pad=256):
    return bool((slab[:pad] == fill).all()) and bool((slab[pad + n:] == fill).all())


class Buffers:
    """Allocator of named device buffers.  Guarded: each buffer sits inside a uint8 slab with `pad` sentinel bytes before and after it
    (a multiple of 256: the inner view keeps the allocation's alignment); exact: plain tensors of exactly the requested size, for the
    same calls' reference results."""

    def __init__(self, guarded):
        self.guarded, self.slabs = guarded, {}

    def __call__(self, name, shape, dtype, init=0, pad=1024):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        if not self.guarded:
            return torch.full(shape, init, dtype=dtype, device="cuda")
        assert name not in self.slabs, name
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        s = torch.full((pad + nbytes + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
        inner = s[pad:pad + nbytes].view(dtype).view(shape)
        inner.fill_(init)
        self.slabs[name] = (s, pad, nbytes)
        return inner

    def stray(self):
        """Names of the buffers with a guard byte that no longer holds the sentinel."""
        return [name for name, (s, pad, nb) in self.slabs.items()
                if not (bool((s[:pad] == SENTINEL).all()) and bool((s[pad + nb:] == SENTINEL).all()))]


def group_width(n):
    g = 2
    while g < 2 * n:
        g *= 2
    return g


def pools(E, n):
    """wave_blocks: one bullet pool per wave the widest launch over E games starts (the fused rollout's G/2 waves per 32 games, n <= 4)."""
    G = group_width(n)
    return -(-E // 32) * (G // 2) if n <= 4 else -(-E // (64 // G))


def layout(E, n):
    """make_layout: [(field, offset, bytes the field uses)], total bytes."""
    EA, NB = E * 2 * n, pools(E, n)
    used = (("lut", 361 * 16), ("envc", E * 8), ("envd", E * 8), ("cnt", E * 16), ("plane", EA * 8), ("pdirf", EA * 8),
            ("bcnt", NB * 4), ("bent", NB * 768 * 8), ("bdir", 12 * EA * 8), ("bd", 12 * EA * 16))
    out, o = [], 0
    for name, nb in used:
        out.append((name, o, nb))
        o = (o + nb + 255) & ~255
    return out, o
