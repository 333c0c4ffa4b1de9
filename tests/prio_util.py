"""The prioritised replay ring (csrc/bsx_replay_prio.hip, replay.PrioritizedReplayBuffer) restated in numpy, from the contract of
include/battlespace_hip.h alone.  Priorities are integers and every tree node is an exact int64 sum, so all of this but the two powf is
exact, and the GPU tests compare bit for bit:

  levels, tree_levels, node_buffer   the levels' (offset, count) and their sums from the leaves
  draw_r, draw_u, draw_rows          r from the Philox words (philox_util.philox4x32_10), u = mulhi64(r, total) in Python ints, the rows
                                     by cumsum + searchsorted;  descend: the same rows by the level-by-level descent a kernel makes
  append_range, update_max           the leaves after an append of `stored` rows and after an update, in integers
  priority_ref / priority_yard       p from TD errors: float64 (unrounded, clamped) and the float32 torch evaluation, rounded as the kernel rounds
  weights_ref / weights_yard         (p_min / p) ^ beta in float64 and in float32 torch
  random_leaves, needle_leaves, heavy_leaves, edge_rows   leaf patterns: log-uniform with zeros, a few non-zero rows at the node boundaries
                                     of every level, and all near 2^31 with an odd total (past 2^53 at five levels)
  stamp_ring, stamps                 the row index written into the ring's rows, and read back from a gathered batch
Nothing here imports the native library."""
import functools

import numpy as np
import torch

import philox_util as P

FAN, ONE, P_MAX, SALT = 64, 65536, 1 << 31, 0x3C6EF372
# The sizes at which the tree is checked at depth: 64^2 and 64^3 exact (two and three levels, all of them the tail workgroup's), 64^3 + 1
# (four levels, every level ragged: its last node has one child) and 64^4 + 67 (five levels; rows 2^24 + 1 and 2^24 + 3 exist)
M4, M5 = 64 ** 3 + 1, 64 ** 4 + 67
DEEP_SIZES = (64 ** 2, 64 ** 3, M4, M5)


def levels(M):
    """[(offset, count)] of the int64 levels over M rows, bottom-up: ceil(M / 64) nodes, then ceil(previous / 64), down to one root."""
    out, off, n = [], 0, -(-int(M) // FAN)
    while True:
        out.append((off, n))
        if n == 1:
            return out
        off, n = off + n, -(-n // FAN)


def unsigned(x):
    """int32-typed bits (a tensor or an array) -> the uint32 values as int64 numpy."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.astype(np.int64) & 0xFFFFFFFF


def tree_levels(leaves):
    """leaves: the M priorities (integers) -> the list of int64 arrays, one per level, each node the sum of its (up to) 64 children."""
    x, out = np.asarray(leaves, np.int64), []
    while True:
        x = np.concatenate([x, np.zeros(-len(x) % FAN, np.int64)]).reshape(-1, FAN).sum(1)
        out.append(x)
        if len(x) == 1:
            return out


def node_buffer(leaves):
    return np.concatenate(tree_levels(leaves))


def draw_r(seed, seq, B):
    """r[b] = (w.y << 32) | w.x of the block (b, b >> 32, seq, seq >> 32) under key (seed, (seed >> 32) ^ SALT) -> a list of Python ints."""
    b = np.arange(B, dtype=np.uint64)
    seed, seq = int(seed), int(seq)
    w = P.philox4x32_10(b & P.MASK, b >> np.uint64(32), seq & 0xFFFFFFFF, seq >> 32, seed & 0xFFFFFFFF, (seed >> 32) ^ SALT)
    return [(int(hi) << 32) | int(lo) for lo, hi in zip(w[0], w[1])]


def draw_u(seed, seq, B, total):
    """u[b] = mulhi64(r[b], total): the high 64 bits of the 128-bit product, in Python ints -> int64 [B] (u < total < 2^62)."""
    return np.array([(r * int(total)) >> 64 for r in draw_r(seed, seq, B)], np.int64)


def rows_of(leaves, u):
    """searchsorted(cumsum(leaves), u, side="right"): the first row whose inclusive prefix sum exceeds u."""
    return np.searchsorted(np.cumsum(np.asarray(leaves, np.int64)), u, side="right").astype(np.int64)


def draw_rows(leaves, seed, seq, B):
    """The rows sample() draws at sequence word seq -> int64 [B]; all 0 for an empty ring (total = 0)."""
    total = int(np.asarray(leaves, np.int64).sum())
    return rows_of(leaves, draw_u(seed, seq, B, total)) if total else np.zeros(B, np.int64)


def descend(leaves, u):
    """The same rows by the descent: from the root, at each node the first child whose inclusive prefix exceeds u, minus the exclusive."""
    lv = tree_levels(leaves)
    below = [np.concatenate([np.asarray(leaves, np.int64), np.zeros(-len(leaves) % FAN, np.int64)])] + lv[:-1]
    u, node = np.asarray(u, np.int64).copy(), np.zeros(len(u), np.int64)
    for children in reversed(below):
        c = np.concatenate([children, np.zeros(-len(children) % FAN, np.int64)]).reshape(-1, FAN)[node]      # [B, 64]
        incl = np.cumsum(c, 1)
        j = (incl > u[:, None]).argmax(1)
        u -= incl[np.arange(len(u)), j] - c[np.arange(len(u)), j]
        node = node * FAN + j
    return node


def append_range(leaves, counter, stored, max_priority):
    """The leaves after an append that kept `stored` rows and left the ring's counter at `counter`: rows (counter - s + j) mod M, j < s =
    min(stored, M), get max_priority."""
    out, M = np.asarray(leaves, np.int64).copy(), len(leaves)
    s = min(int(stored), M)
    out[(int(counter) - s + np.arange(s)) % M] = int(max_priority)
    return out


def update_max(leaves, idx, p):
    """The leaves after an update: every named row holds the largest p of its occurrences; the others are untouched."""
    out = np.asarray(leaves, np.int64).copy()
    out[idx] = 0
    np.maximum.at(out, idx, np.asarray(p, np.int64))
    return out


def priority_ref(q, y, hyper):
    """float64: clamp(pi * 65536, 1, 2^31), pi = (min(max_i |q - y|, delta_max) + eps) ^ alpha, a NaN error = delta_max; NOT rounded.
    q, y float32 arrays [B, nA]; hyper: the float32 row (alpha, beta, eps, delta_max)."""
    alpha, _, eps, dmax = (float(np.float32(h)) for h in hyper)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(q, np.float64) - np.asarray(y, np.float64))
    d = np.where(np.isnan(d), dmax, np.minimum(d, dmax)).max(1)
    return np.clip((d + eps) ** alpha * ONE, 1.0, float(P_MAX))


def priority_yard(q, y, hyper):
    """The same as a torch user writes it in float32 on the CPU, rounded as the kernel rounds (rint, clamp) -> float64 [B]."""
    alpha, _, eps, dmax = (torch.tensor(float(h), dtype=torch.float32) for h in hyper)
    d = (torch.as_tensor(q, dtype=torch.float32) - torch.as_tensor(y, dtype=torch.float32)).abs()
    d = torch.where(d.isnan(), dmax, torch.minimum(d, dmax)).max(1).values
    x = torch.round(torch.pow(d + eps, alpha) * 65536.0)
    return x.clamp(1.0, float(P_MAX)).double().numpy()


def weights_ref(p, beta):
    """float64 (p_min / p) ^ beta over the batch's non-zero leaves p (integers); a zero leaf's weight is 0."""
    p = np.asarray(p, np.float64)
    if not (p > 0).any():
        return np.zeros(len(p))
    with np.errstate(divide="ignore"):
        return np.where(p > 0, (p[p > 0].min() / p) ** float(np.float32(beta)), 0.0)


def weights_yard(p, beta):
    """float32 torch: pow(float(p_min) / float(p), beta) -> float64 [B]."""
    p = torch.as_tensor(np.asarray(p, np.int64))
    if not bool((p > 0).any()):
        return np.zeros(len(p))
    pf = p.float()
    w = torch.pow(pf[p > 0].min() / pf, torch.tensor(float(beta), dtype=torch.float32))
    return torch.where(p > 0, w, torch.zeros(())).double().numpy()


def random_leaves(M, seed=0):
    """M priorities spanning 1 .. 2^31 (log-uniform, both ends present when M >= 3), about a third of them 0."""
    g = np.random.default_rng(7000 + seed + M)
    p = np.minimum(np.floor(2.0 ** g.uniform(0.0, 31.0, M)).astype(np.int64), P_MAX)
    if M >= 3:
        p[g.permutation(M)[:2]] = (1, P_MAX)
        zero = g.random(M) < 1.0 / 3.0
        zero[np.isin(p, (1, P_MAX))] = False
        p[zero] = 0
    return p


def needle_leaves(M, rows, p=ONE):
    """All M leaves 0 but the named rows, which hold p: a draw can only land on them, wherever in the tree they sit."""
    out = np.zeros(int(M), np.int64)
    out[np.asarray(rows, np.int64)] = int(p)
    return out


def edge_rows(M):
    """The rows on either side of every node boundary of every level (64^k - 1 and 64^k), the first row and the last two, and where
    M reaches them 2^24 + 1 and 2^24 + 3 (odd integers no float32 holds) -> the sorted int64 rows below M."""
    rows = {0, M - 2, M - 1, (1 << 24) + 1, (1 << 24) + 3}
    edge = FAN
    while edge <= M:
        rows |= {edge - 1, edge}
        edge *= FAN
    return np.array(sorted(r for r in rows if 0 <= r < M), np.int64)


def heavy_leaves(M):
    """Every leaf 2^31 or 2^31 - 1, an odd number of them the latter: an odd total, so its lowest bit is set and a total carried through a
    double anywhere past 2^53 (reached from M = 2^22 + 1 on) would come out wrong."""
    g = np.random.default_rng(9000 + M)
    less = g.random(int(M)) < 0.5
    less[0] ^= less.sum() % 2 == 0
    p = P_MAX - less.astype(np.int64)
    total = int(p.sum())
    assert total % 2 == 1 and (M < (1 << 24) or total > 1 << 53)
    return p


PATTERNS = ("random", "needles", "heavy")


@functools.lru_cache(maxsize=None)
def pattern_leaves(M, pattern):
    """random_leaves(M), equal needles on edge_rows(M) or heavy_leaves(M), built once per process and read-only (five levels: seconds)."""
    p = {"random": random_leaves, "needles": lambda m: needle_leaves(m, edge_rows(m)), "heavy": heavy_leaves}[pattern](M)
    p.flags.writeable = False
    return p


def stamp_ring(buf):
    """The row index, as an int32 bit pattern, into word 0 of every row of the ring's three wide fields: a gathered batch then carries
    the rows it was read from in its own bits, whatever last_idx says.  Stands in for a fill where a test is about the draw."""
    stamp = torch.arange(buf.mem_size, dtype=torch.int32, device=buf.actor_states.device)
    for field in (buf.actor_states, buf.actor_new_states, buf.action_mem):
        field.view(torch.int32).view(buf.mem_size, -1)[:, 0] = stamp


def stamps(batch_field):
    """Word 0 of every row of a gathered [B, nA, W] field, as the int64 row indices stamp_ring wrote."""
    return batch_field.view(torch.int32).view(batch_field.shape[0], -1)[:, 0].cpu().numpy().astype(np.int64)


def as_leaves(p, device="cuda"):
    """Integer priorities -> the int32-typed bits `priorities` holds."""
    return torch.from_numpy(np.asarray(p, np.int64).astype(np.uint32).view(np.int32).copy()).to(device)
