"""The keyed row permutation and the minibatch gather on the GPU (learner.shuffle_rows / minibatch_gather; csrc/bsx_shuffle.hip) against
the numpy restatement (tests/shuffle_util.py), exactly: every size class of the permutation up to N = 2^31 - 1, the seq_base word, and
the gather between guard slabs -- indices, every field as bits (NaN payloads, -0.0, denormals), ragged slabs around the kernel's rows
per workgroup, a null value, the partition of an epoch, determinism and replays of a captured call."""
import functools

import numpy as np
import pytest
import torch

import guard_util as G
import shuffle_util as S

pytestmark = pytest.mark.gpu
SEED, SEQ = 41, 7
FLOATS = ("obs", "rec", "logp", "adv", "ret", "value")
SPECIAL = (0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7FA00000, 0xFFC12345, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000)


@functools.lru_cache(maxsize=None)
def _perm(N, seed=SEED, seq=SEQ):
    p = S.perm(N, seed, seq)
    p.setflags(write=False)
    return p


def _widths(A, D):
    return dict(obs=(A, D), rec=(A, 4), logp=(A,), adv=(A,), ret=(A,), value=(A,), mask=(A,))


def _source(N, A, D):
    """Guarded source buffers of N rows: random bits in every word (so NaNs of many payloads, infinities, denormals), the SPECIAL
    patterns in the first words of every float field and spread over obs; random bytes in the mask."""
    buf, gen = G.Buffers(True), torch.Generator().manual_seed(1000 * A + D + N)
    src = {}
    for f, tail in _widths(A, D).items():
        if f == "mask":
            src[f] = buf("src_" + f, (N, *tail), torch.uint8)
            src[f].copy_(torch.randint(0, 256, (N, *tail), generator=gen, dtype=torch.uint8))
            continue
        bits = torch.randint(-2 ** 31, 2 ** 31, (N, *tail), generator=gen, dtype=torch.int64).to(torch.int32)
        flat = bits.view(-1)
        special = torch.from_numpy(np.array(SPECIAL, dtype=np.uint32).view(np.int32))
        for spread in (flat, flat[::37]):
            k = min(len(SPECIAL), spread.numel())
            spread[:k] = special[:k]
        src[f] = buf("src_" + f, (N, *tail), torch.float32)
        src[f].view(torch.int32).copy_(bits)
    return buf, src


def _dest(R, A, D):
    buf, dst = G.Buffers(True), {}
    for f, tail in _widths(A, D).items():
        dst[f] = buf("dst_" + f, (R, *tail), torch.uint8 if f == "mask" else torch.float32, init=0x5B if f == "mask" else 1.5)
    dst["idx"] = buf("idx", (R,), torch.int64, init=-1)
    return buf, dst


def _mb(d, value=True, idx=True):
    from deep_rl_battlespace_amd.learner import Minibatch
    return Minibatch(d["obs"], d["rec"], d["logp"], d["adv"], d["ret"], d["mask"], d["value"] if value else None, d.get("idx") if idx else None)


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _slabs(N, W):
    """(first, R): R in {1, W - 1, W, W + 1, 3 W + 5} from a `first` that is no multiple of W, where they fit; the slab that ends at N."""
    out = [(3, R) for R in (1, W - 1, W, W + 1, 3 * W + 5) if 3 + R <= N]
    tail = min(N, 3 * W + 5)
    return out + [(N - tail, tail)]


def _check_slab(src, N, A, D, first, R, value, seq=SEQ, seq_base=None, base=0):
    from deep_rl_battlespace_amd.learner import minibatch_gather
    buf, dst = _dest(R, A, D)
    minibatch_gather(_mb(src, value, idx=False), _mb(dst, value), first, R, SEED, seq, seq_base)
    torch.cuda.synchronize()
    want = torch.from_numpy(_perm(N, SEED, seq + base)[first:first + R].copy()).cuda()
    assert torch.equal(dst["idx"], want), (N, first, R)
    for f in _widths(A, D):
        if f == "value" and not value:
            assert bool((dst[f] == 1.5).all()), "a null value must leave the destination untouched"
            continue
        assert torch.equal(_bits(dst[f]), _bits(src[f]).index_select(0, want)), (f, N, first, R)
    assert buf.stray() == [], buf.stray()
    return dst


def test_shuffle_rows_is_the_restatement_at_every_size_class():
    from deep_rl_battlespace_amd.learner import shuffle_rows
    for N in (1, 5, 7, 768, 2 ** 16, 2 ** 16 + 1):
        buf = G.Buffers(True)
        out = buf("idx", (N,), torch.int64, init=-1)
        assert shuffle_rows(N, 0, N, SEED, SEQ, out=out) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), _perm(N)), N
        assert buf.stray() == []
    # a slab from the middle, into a fresh tensor
    got = shuffle_rows(2 ** 16 + 1, 12345, 1000, SEED, SEQ)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), _perm(2 ** 16 + 1)[12345:13345])
    # the widest domain: b = 16, where x reaches 2^32 - 1 -- both ends of the range
    N = 2 ** 31 - 1
    for first in (0, N - 4096):
        got = shuffle_rows(N, first, 4096, SEED, SEQ).cpu().numpy()
        assert np.array_equal(got, S.perm_at(N, SEED, SEQ, np.arange(first, first + 4096))), first


def test_the_seq_base_word_is_added_to_seq_on_the_device():
    from deep_rl_battlespace_amd.learner import shuffle_rows
    N = 768
    plain = shuffle_rows(N, 0, N, SEED, SEQ, seq_base=None).cpu().numpy()
    assert np.array_equal(plain, _perm(N))
    for base in (3, 2 ** 32 + 3):
        word = torch.tensor([base], dtype=torch.int64, device="cuda")
        got = shuffle_rows(N, 0, N, SEED, SEQ, seq_base=word).cpu().numpy()
        assert np.array_equal(got, S.perm(N, SEED, SEQ + base)), base
        assert not np.array_equal(got, plain)
        assert int(word) == base


CASES = [(A, D, N) for A, D in ((2, 8), (6, 11), (8, 14), (32, 50)) for N in (1, 5, 768)] + [(2, 8, 2 ** 16 + 1)]


@pytest.mark.parametrize("A,D,N", CASES)
def test_the_gather_copies_the_restated_rows_bit_for_bit_and_nothing_else(A, D, N):
    from deep_rl_battlespace_amd.learner import GATHER_ROWS as W
    sbuf, src = _source(N, A, D)
    kept = {f: x.clone() for f, x in src.items()}
    for k, (first, R) in enumerate(_slabs(N, W)):
        _check_slab(src, N, A, D, first, R, value=k % 2 == 0)
    torch.cuda.synchronize()
    assert sbuf.stray() == [] and all(torch.equal(_bits(src[f]), _bits(kept[f])) for f in src)      # the source is read only


def test_a_null_value_on_both_sides_leaves_the_destination_value_alone():
    A, D, N = 6, 11, 768
    _, src = _source(N, A, D)
    _check_slab(src, N, A, D, 5, 133, value=False)
    _check_slab(src, N, A, D, 5, 133, value=True)


def test_the_minibatches_of_one_epoch_hold_every_row_exactly_once():
    A, D, N, M = 2, 8, 768, 4
    _, src = _source(N, A, D)
    R = N // M
    idx = torch.cat([_check_slab(src, N, A, D, m * R, R, value=True)["idx"] for m in range(M)])
    assert torch.equal(idx.sort().values, torch.arange(N, device="cuda"))
    other = torch.cat([_check_slab(src, N, A, D, m * R, R, value=True, seq=SEQ + 1)["idx"] for m in range(M)])
    assert torch.equal(other.sort().values, torch.arange(N, device="cuda")) and not torch.equal(other, idx)


def test_two_calls_give_the_same_bits_and_a_captured_call_follows_seq_base():
    from deep_rl_battlespace_amd.learner import minibatch_gather
    A, D, N, first, R = 6, 11, 768, 70, 133
    _, src = _source(N, A, D)
    base = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = _check_slab(src, N, A, D, first, R, value=True, seq_base=base)
    b = _check_slab(src, N, A, D, first, R, value=True, seq_base=base)
    assert all(torch.equal(_bits(a[f]), _bits(b[f])) for f in a)
    buf, dst = _dest(R, A, D)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        minibatch_gather(_mb(src, idx=False), _mb(dst), first, R, SEED, SEQ, base)
    seen = []
    for value in (0, 1, 2 ** 32 + 5):
        base.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        want = torch.from_numpy(_perm(N, SEED, SEQ + value)[first:first + R].copy()).cuda()
        assert torch.equal(dst["idx"], want), value
        for f in _widths(A, D):
            assert torch.equal(_bits(dst[f]), _bits(src[f]).index_select(0, want)), (f, value)
        seen.append(dst["idx"].clone())
    assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], a["idx"]) and buf.stray() == []
