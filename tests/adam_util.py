"""What the tests of the fused optimiser step (learner.adam_step, csrc/bsx_adam_step.hip) share:

  reference_step     the contract of include/battlespace_hip.h (bsx_adam_step) restated in float64 numpy: torch's clip_grad_norm_ followed
                     by Adam.step(), no weight decay, no amsgrad, over a flat list of arrays
  hyper32            hyperparameters as the float32 values the device reads (`hyper` is a float32 tensor): the restatement, torch's own
                     float32 Adam and the kernel are all given exactly these numbers
  row_to_tensors / tensors_to_row   a [A, G] row in bsx_actor_grad's layout <-> the ten parameter shapes of a StackedActor
  random_rows        gradient rows with magnitudes spread over 1e-4 .. 1, the pad columns of w3 / b3 at +0
  pad_mask           where those pad columns are in a row
  w2b_words          the bfloat16 part of StackedActor.pack()'s blob restated on uint32 bit patterns (round to nearest even by hand, residuals
                     in float32, the blob's index map), and w2_edge_weights, a w2 that forces ties, their neighbours, carries and +-0

The bars a step is held to are yardstick_util's, pooled over a network's ten tensors."""
import numpy as np
import torch

import yardstick_util as Y

PARAMS = ("w1", "b1", "g1", "h1", "w2", "b2", "g2", "h2", "w3", "b3")
H = 64


def grad_floats(D):
    return H * D + H * H + 6 * H + H * 4 + 4


def hyper32(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.0):
    """dict of Python floats that are exactly representable in float32: what the device reads from `hyper`."""
    f = lambda x: float(np.float32(x))     # noqa: E731
    return dict(lr=f(lr), beta1=f(beta1), beta2=f(beta2), eps=f(eps), max_grad_norm=f(max_grad_norm))


def reference_step(params, grads, m, v, t, hp):
    """One step in float64.  params, grads, m, v: lists of numpy arrays of matching shapes (any float dtype: converted); t: the steps
    taken so far; hp: hyper32(...) -> (params, m, v, t + 1, norm, coef), new arrays.
      norm = sqrt(sum of g^2 over everything);  coef = min(1, max_norm / (norm + 1e-6)) (1 with max_norm = 0);  g = coef grad
      m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps),  t the NEW count"""
    lr, b1, b2, eps, mx = hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["max_grad_norm"]
    g64 = [np.asarray(g, np.float64) for g in grads]
    norm = float(np.sqrt(sum(float((g * g).sum()) for g in g64)))
    coef = min(1.0, mx / (norm + 1e-6)) if mx > 0.0 else 1.0
    t = int(t) + 1
    step_size, c2 = lr / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t)
    P, M, V = [], [], []
    for p, g, m_, v_ in zip(params, g64, m, v):
        g = coef * g
        mn = b1 * np.asarray(m_, np.float64) + (1.0 - b1) * g
        vn = b2 * np.asarray(v_, np.float64) + (1.0 - b2) * g * g
        P.append(np.asarray(p, np.float64) - step_size * mn / (np.sqrt(vn) / c2 + eps))
        M.append(mn)
        V.append(vn)
    return P, M, V, t, norm, coef


def row_to_tensors(row, n_actions):
    """row [A, G] (numpy or torch, bsx_actor_grad's layout: w1[D][64] | b1 | g1 | h1 | w2[64][64] | b2 | g2 | h2 | w3[64][4] | b3[4]) -> the ten
    arrays in PARAMS order in a StackedActor's shapes, w3 / b3 cut to n_actions columns (contiguous copies)."""
    A, G = row.shape
    D = (G - grad_floats(0)) // H
    assert grad_floats(D) == G, G
    out, o = [], 0
    for k in PARAMS:
        shape = dict(w1=(D, H), w2=(H, H), w3=(H, 4), b3=(1, 4)).get(k, (1, H))
        n = shape[0] * shape[1]
        x = row[:, o:o + n].reshape(A, *shape)
        o += n
        if k in ("w3", "b3"):
            x = x[:, :, :n_actions]
        out.append(x.copy() if isinstance(x, np.ndarray) else x.contiguous().clone())
    assert o == G
    return out


def tensors_to_row(tensors):
    """The inverse: ten numpy arrays -> a float64 [A, G] row, the pad columns of w3 / b3 at 0."""
    A = tensors[0].shape[0]
    cols = []
    for k, x in zip(PARAMS, tensors):
        x = np.asarray(x, np.float64)
        if k in ("w3", "b3") and x.shape[2] < 4:
            x = np.concatenate([x, np.zeros((A, x.shape[1], 4 - x.shape[2]))], axis=2)
        cols.append(x.reshape(A, -1))
    return np.concatenate(cols, axis=1)


def random_rows(A, D, n_actions, gen, scale=1.0):
    """float32 [A, G] on the CPU: sign * 10^U(-4, 0) * scale per element, +0 in the pad columns of w3 / b3.  gen: a torch.Generator."""
    G = grad_floats(D)
    mag = torch.pow(10.0, -4.0 * torch.rand((A, G), generator=gen, dtype=torch.float64))
    sign = torch.where(torch.rand((A, G), generator=gen) < 0.5, -1.0, 1.0).double()
    row = (scale * sign * mag).float()
    tail = row[:, G - (H * 4 + 4):].view(A, H + 1, 4)
    tail[:, :, n_actions:] = 0.0
    return row


def pad_mask(D, n_actions):
    """bool [G]: True at the elements of a gradient (or moment) row with no parameter behind them, columns n_actions..3 of w3[64][4] and
    b3[4] -- 65 (4 - n_actions) of them, none for a 4-column network."""
    G = grad_floats(D)
    mask = np.zeros(G, dtype=bool)
    mask[G - (H * 4 + 4):].reshape(H + 1, 4)[:, n_actions:] = True
    return mask


# ---- W2B, the bfloat16 part of the packed blob, restated on bit patterns (StackedActor.pack(); bsx_adam_step.hip: bf16_rne, w2b_term)
W2B_FLOATS = 2 * 4 * 3 * 64 * 8 // 2            # the blob's last floats: [mo 2][s 4][term 3][lane 64][i 8] bfloat16, two per float


def bf16_rne_bits(u):
    """uint32 bit patterns of finite float32 -> the 16 bits of the nearest bfloat16, ties to the even one."""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint32)


def bf16_bits_to_float(h):
    return (np.asarray(h, np.uint32) << 16).view(np.float32)


def w2b_split(w):
    """float32 array -> (h, m, l), uint32 arrays of bfloat16 bits: h = bf16(w), m = bf16(w - h), l = bf16((w - h) - m), the residuals
    taken in float32."""
    w = np.ascontiguousarray(w, np.float32)
    h = bf16_rne_bits(w.view(np.uint32))
    r1 = w - bf16_bits_to_float(h)
    m = bf16_rne_bits(r1.view(np.uint32))
    r2 = r1 - bf16_bits_to_float(m)
    return h, m, bf16_rne_bits(r2.view(np.uint32))


def w2b_words(w2):
    """w2 float32 [A, 64, 64] -> uint32 [A, W2B_FLOATS], the bits of the blob's W2B part: element [mo][s][term][lane][i] is term `term`
    of w2[nid(s >> 1, 8 (s & 1) + i, lane >> 5)][32 mo + (lane & 31)], nid(m, v, hh) = 32 m + (v & 3) + 8 (v >> 2) + 4 hh; the even i of a
    pair sits in the low half of its float."""
    w2 = np.ascontiguousarray(w2, np.float32)
    A = w2.shape[0]
    assert w2.shape == (A, H, H), w2.shape
    mo, s, lane, i = np.ogrid[0:2, 0:4, 0:64, 0:8]
    v = 8 * (s & 1) + i
    k, j = np.broadcast_arrays(32 * (s >> 1) + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5) + 0 * mo, 32 * mo + (lane & 31) + 0 * s + 0 * i)
    terms = np.stack(w2b_split(w2[:, k, j]), axis=3)                    # [A, mo, s, term, lane, i]
    pairs = terms.reshape(A, W2B_FLOATS, 2)
    return (pairs[:, :, 0] | (pairs[:, :, 1] << 16)).astype(np.uint32)


W2_EDGE_EXPONENTS = (-60, -20, -1, 0, 7, 60)
W2_EDGE_UPPER = (0x00, 0x01, 0x3a, 0x7e, 0x7f)                          # the seven mantissa bits a bfloat16 keeps
W2_EDGE_LOW = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)          # the sixteen it drops: below, at and above the tie


def w2_edge_weights(A, seed):
    """float32 [A, 64, 64] for a network's w2, where round-to-nearest-even is decided: per agent, in an order shuffled per agent, every
    (exponent, upper mantissa, low half, sign) of the tables above -- ties (low half 0x8000) over an even and an odd kept mantissa, one
    bit either side of a tie, the smallest and largest remainders, and with upper 0x7f the round-ups that carry into the exponent --
    then +0 and -0, then random bit patterns with exponents in -60 .. 60.  Within 2^+-60 neither a term nor a float32 residual
    (a multiple of the weight's ulp, at least 2^-83) is subnormal or overflows: no result depends on a denormal mode."""
    rng = np.random.default_rng(seed)
    crafted = np.array([(sg << 31) | ((e + 127) << 23) | (up << 16) | lo for e in W2_EDGE_EXPONENTS for up in W2_EDGE_UPPER
                        for lo in W2_EDGE_LOW for sg in (0, 1)] + [0x00000000, 0x80000000], dtype=np.uint32)
    out = np.empty((A, H * H), dtype=np.uint32)
    for a in range(A):
        k = H * H - crafted.size
        rand = (rng.integers(0, 2, k, dtype=np.uint32) << 31) | (rng.integers(127 - 60, 127 + 60 + 1, k, dtype=np.uint32) << 23) | \
            rng.integers(0, 1 << 23, k, dtype=np.uint32)
        out[a] = rng.permutation(np.concatenate([crafted, rand]))
    return out.view(np.float32).reshape(A, H, H)


def net_arrays(net):
    """A StackedActor's ten parameters as float32 numpy arrays (copies)."""
    return [getattr(net, k).detach().cpu().numpy().copy() for k in PARAMS]


def check_step(got, ref, yard, what, out=None, names=("p", "m", "v", "target")):
    """yardstick_util's bars on one network's optimiser step, each of `names` pooled over the network's tensors.  got, ref, yard: {name:
    list of arrays} from the device, the float64 step and the float32 yardstick (off float64 somewhere).  Prints, keeps the ratios in `out`."""
    assert all(e > 0.0 for k in names for e in Y.errors(yard[k], ref[k])), what
    r, bad = Y.check_tensors([(k, got[k], ref[k], yard[k], Y.FACTORS) for k in names], what, "pooled")
    (out if out is not None else {}).update({f"{what}.{k}": [round(v[0], 4), round(v[1], 4)] for k, v in r.items()})
    assert not bad, (what, bad, r)
