"""Shuffled minibatches on device (csrc/bsx_shuffle.hip): a keyed permutation of the rows and the gather of one minibatch through it.

  shuffle_rows(N, first, R, seed, seq, ...)                     a keyed permutation of [0, N) evaluated per position (bsx_shuffle_rows)
  minibatch_gather(src, dst, first, R, seed, seq, ...)          one shuffled minibatch's records through it, one launch (bsx_minibatch_gather)
"""
from collections import namedtuple
from functools import partial

import torch

from .. import _lib
from .._args import _F32, _FLAG, _need
from ._common import _int64_word, _stream

GATHER_ROWS = 32                         # destination rows per workgroup of bsx_minibatch_gather (csrc/bsx_shuffle.hip: ROWS)
_I64 = (torch.int64,)
# One minibatch's records, source or destination: obs f32 [rows, A, D], rec f32 [rows, A, 4], logp, adv, ret f32 [rows, A], mask uint8 or
# bool [rows, A], value f32 [rows, A] or None, and on the destination idx int64 [rows]
Minibatch = namedtuple("Minibatch", "obs rec logp adv ret mask value idx", defaults=(None, None))


def _word(x, name):
    """int(x) in [0, 2^64): a Philox seed or sequence number."""
    if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < 1 << 64:
        raise ValueError(f"{name} must be an int in [0, 2^64), got {x!r}")
    return x


def _rows(N, first, R):
    """(N, first, R) as ints: 1 <= N < 2^31 and a non-empty range [first, first + R) inside [0, N)."""
    N, first, R = int(N), int(first), int(R)
    if not 1 <= N < 1 << 31:
        raise ValueError(f"N must be in [1, 2^31), got {N}")
    if R < 1 or first < 0 or first + R > N:
        raise ValueError(f"rows [{first}, {first} + {R}) are not a non-empty range inside [0, {N})")
    return N, first, R


def _seq_base(seq_base, dev):
    if seq_base is None:
        return None
    _int64_word(seq_base, "seq_base", dev, "the call's tensors")
    return seq_base.data_ptr()


def shuffle_rows(N, first, R, seed, seq, seq_base=None, out=None, device="cuda"):
    """Positions [first, first + R) of the keyed permutation of [0, N) (csrc/bsx_shuffle.hip, `bsx_shuffle_rows`; the construction is
    written out in include/battlespace_hip.h) -> int64 [R] on the device: the source row of every position.  A bijection of [0, N) for
    every (seed, seq + seq_base): seed, seq ints in [0, 2^64); seq_base an int64 device tensor of one element, read on the device at
    every launch (a captured call draws afresh once the caller advances it), or None.  One launch on the current stream, no host
    synchronisation.  out: an int64 [R] tensor to write into (nothing is allocated then); its device is the call's."""
    N, first, R = _rows(N, first, R)
    seed, seq = _word(seed, "seed"), _word(seq, "seq")
    if out is None:
        out = torch.empty(R, dtype=torch.int64, device=device)
    elif not isinstance(out, torch.Tensor):
        raise TypeError("out must be a torch.Tensor")
    dev = out.device
    if dev.type != "cuda":
        raise ValueError("shuffle_rows runs on the GPU: out is on " + str(dev))
    _need(out, "out", (R,), _I64, dev, "out")
    _lib.check(_lib.load().bsx_shuffle_rows(N, first, R, seed, seq, _seq_base(seq_base, dev), out.data_ptr(), _stream(dev)),
               "bsx_shuffle_rows")
    return out


def minibatch_gather(src, dst, first, R, seed, seq, seq_base=None):
    """One minibatch of a shuffled epoch in one launch (csrc/bsx_shuffle.hip, `bsx_minibatch_gather`): for r in [0, R), dst.idx[r] =
    perm(first + r) and row r of every field of dst = row dst.idx[r] of src, bit for bit -> dst.

    src, dst: a learner.Minibatch (or any sequence in its order).  src holds the N rows the permutation is over -- obs f32 [N, A, D]
    (leading axes are flattened: a rollout's [T, E, A, D] records are N = T E rows), rec f32 [N, A, 4], logp, adv, ret f32 [N, A], mask
    uint8 or bool [N, A], value f32 [N, A] or None --, dst the same fields with R rows and idx int64 [R]; value on both sides or on
    neither.  seed, seq, seq_base: shuffle_rows'.  The M calls first = m R of one (seed, seq) hold every source row exactly once.
    Contiguous tensors on one GPU; dst must not overlap src.  No host synchronisation, nothing allocated."""
    src, dst = Minibatch(*src), Minibatch(*dst)
    obs = src.obs
    if not isinstance(obs, torch.Tensor) or obs.dim() < 3:
        raise ValueError("src.obs must be a float32 [N, A, D] tensor")
    dev, A, D = obs.device, obs.shape[-2], obs.shape[-1]
    if dev.type != "cuda":
        raise ValueError("minibatch_gather runs on the GPU: src.obs is on " + str(dev))
    if A < 2 or A % 2 or A > 2 * _lib.MAX_N or not 1 <= D <= 3 * _lib.MAX_N + 2:
        raise ValueError(f"src.obs has shape {tuple(obs.shape)}: an even A in 2 .. {2 * _lib.MAX_N} and D in 1 .. {3 * _lib.MAX_N + 2} are needed")
    lead = tuple(obs.shape[:-2])
    N, first, R = _rows(obs.numel() // (A * D), first, R)
    seed, seq = _word(seed, "seed"), _word(seq, "seq")
    if (src.value is None) != (dst.value is None):
        raise ValueError("value goes on both sides or on neither: src.value and dst.value")
    need = partial(_need, dev=dev, anchor="src.obs")
    io = _lib.BsxMinibatchIo()
    for side, t, rows, pre in (("src", src, lead, ""), ("dst", dst, (R,), "dst_")):
        for f, tail, dtypes in (("obs", (A, D), _F32), ("rec", (A, 4), _F32), ("logp", (A,), _F32), ("adv", (A,), _F32), ("ret", (A,), _F32),
                                ("mask", (A,), _FLAG), ("value", (A,), _F32)):
            x = getattr(t, f)
            if f == "value" and x is None:
                continue
            need(x, f"{side}.{f}", (*rows, *tail), dtypes)
            setattr(io, pre + f, x.data_ptr())
    need(dst.idx, "dst.idx", (R,), _I64)
    io.idx = dst.idx.data_ptr()
    _lib.check(_lib.load().bsx_minibatch_gather(_lib.ctypes.byref(io), N, first, R, A, D, seed, seq, _seq_base(seq_base, dev), _stream(dev)),
               "bsx_minibatch_gather")
    return dst
