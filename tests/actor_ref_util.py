"""A float64 reference of the per-agent actor MLP (rollout.StackedActor, csrc/bsx_actor_core.h) and what goes with it:

  to_float64 / head_sums64   the network in float64 on the CPU: the head sums BEFORE tanh, the reference every actor kernel is held to
  head_sums32                the same sums from torch float32 on the CPU: the yardstick e_t ("what float32 loses on these inputs")
  split_model64              float64 everywhere except that the operands of the 64 x 64 layer are split in 2 or 3 bfloat16 terms the way
                             pack() and tile_forward split them: what a split mode is ALLOWED to lose (e_m); independent of the kernels
  as_critics                 one single-output StackedActor per head column: fed as a value head, the kernel writes that column's raw
                             head sum in the call's precision mode -- the head sums observable before tanh with no kernel change
  mfma_emulation             the kernels' index arithmetic lane by lane on the documented MFMA fragment maps (pins the blob layout)
  input classes              functions of (n, seed) returning (actor, obs) on the CPU: fresh, shipped, trained_like, flat_rows, dead_half,
                             wide_obs; localisation_case for the one-neuron networks
  bounds / score_budget      the conditions of tests/test_hip_actor_float64.py, stated once

Nothing here imports the native library except kernel_outputs (GPU callers only)."""
import functools
import os

import numpy as np
import torch

from trace_util import GOLDEN
from yardstick_util import FACTORS as F32_FACTORS      # mean(e_k) <= 2 mean(e_t), max(e_k) <= 4 max(e_t): yardstick_util says where 2 and 4 come from

MODES = ("f32", "bf16x6", "bf16x3")
TERMS = {"bf16x3": 2, "bf16x6": 3}
PARAMS = ("w1", "b1", "g1", "h1", "w2", "b2", "g2", "h2", "w3", "b3")
BODY = PARAMS[:8]
# class -> the team sizes it is run at (shipped: the checkpoints are 2v2 networks; trained_like: where no checkpoint exists)
CLASS_SIZES = {"fresh": (1, 2, 3, 4, 6, 8), "shipped": (2,), "trained_like": (1, 3, 4), "flat_rows": (1, 2, 3, 4),
               "dead_half": (1, 2, 3, 4), "wide_obs": (1, 2, 3, 4)}
ULP1 = 2.0 ** -24                 # half a float32 spacing just below 1: the unit of the absolute slack on a tanh output


def dense_games(n):
    """Games per launch of the dense comparisons: ragged (the last wave's tiles are partly empty), about 5 000."""
    return 5001 - 2 * n


# ------------------------------------------------------------------------------------------------ the reference and the split model
def _new(A, D, na, dtype=torch.float32, device=None):
    from deep_rl_battlespace_amd.rollout import StackedActor
    return StackedActor(A, D, na, dtype=dtype, device=device)


def to(actor, device="cpu", dtype=torch.float32):
    """A StackedActor copy of `actor` on `device` in `dtype` (float32 -> float64 is exact)."""
    a = _new(actor.n_actors, actor.obs_len, actor.n_actions, dtype=dtype, device=device)
    with torch.no_grad():
        for k in PARAMS:
            getattr(a, k).copy_(getattr(actor, k).detach().to(device=device, dtype=dtype))
    return a


to_float64, to_cpu32 = functools.partial(to, dtype=torch.float64), to


def head_sums64(actor, obs):
    """float64 [E, A, n_actions]: the head sums before tanh."""
    with torch.no_grad():
        return to_float64(actor)(obs.detach().cpu().double(), squash=False).numpy()


def head_sums32(actor, obs):
    """The same sums from torch float32 ON THE CPU (so that the yardstick does not move with a GPU GEMM library), widened to float64."""
    with torch.no_grad():
        return to_cpu32(actor)(obs.detach().cpu().float(), squash=False).double().numpy()


def bf16_terms(x32, terms):
    """x = t0 + t1 (+ t2) + residue: t0 = bf16(x), t1 = bf16(x - t0), t2 = bf16(x - t0 - t1), each round-to-nearest-even, the
    differences exact in float32 -- pack()'s split of W2 and tile_forward's split of the activations.  float64 tensors."""
    assert x32.dtype == torch.float32
    out, r = [], x32.clone()
    for _ in range(terms):
        t = r.to(torch.bfloat16).float()
        out.append(t.double())
        r = r - t
    return out


def split_model64(actor, obs, terms):
    """The forward in float64 except for the 64 x 64 layer: its activations are rounded to float32, both operands are split in `terms`
    bfloat16 terms, and the products of order below `terms` are kept -- two terms: wh*xh + wh*xm + wm*xh; three terms: those and
    wl*xh + wm*xm + wh*xl, the six the kernel keeps -- accumulated in float64, smallest first.  float64 [E, A, n_actions]."""
    a = to_float64(actor)
    with torch.no_grad():
        x = obs.detach().cpu().double().transpose(0, 1)
        h = torch.relu(a._ln(torch.baddbmm(a.b1, x, a.w1), a.g1, a.h1))
        xs = bf16_terms(h.float(), terms)
        ws = bf16_terms(actor.w2.detach().cpu().float(), terms)
        acc = a.b2.expand(-1, h.shape[1], -1).clone()
        for order in range(terms - 1, -1, -1):
            for i in range(order + 1):
                acc = acc + torch.bmm(xs[order - i], ws[i])
        h = torch.relu(a._ln(acc, a.g2, a.h2))
        return torch.baddbmm(a.b3, h, a.w3).transpose(0, 1).numpy()


def as_critics(actor):
    """For a policy with 3 or 4 outputs: one StackedActor(A, D, 1) per head column k, carrying the policy's body and column k of w3 / b3
    (on the policy's device).  Its packed blob is the policy's with the other head columns zeroed, moved to column 0."""
    out = []
    for k in range(actor.n_actions):
        c = _new(actor.n_actors, actor.obs_len, 1, device=actor.w1.device)
        with torch.no_grad():
            for name in BODY:
                getattr(c, name).copy_(getattr(actor, name))
            c.w3.copy_(actor.w3[:, :, k:k + 1]); c.b3.copy_(actor.b3[:, :, k:k + 1])
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic on the host
def _mfma_32x32x2(avec, bvec, acc):
    """v_mfma_f32_32x32x2_f32 on host arrays indexed by lane: A[i = l&31][k = l>>5], B[k = l>>5][j = l&31],
    D[i = (v&3) + 8(v>>2) + 4(l>>5)][j = l&31] in register v of lane l (cdna_hip_programming.md section 3)."""
    lanes = np.arange(64)
    Am = np.zeros((32, 2)); Bm = np.zeros((2, 32))
    Am[lanes & 31, lanes >> 5] = avec
    Bm[lanes >> 5, lanes & 31] = bvec
    Dm = Am @ Bm
    for v in range(16):
        acc[v] += Dm[(v & 3) + 8 * (v >> 2) + 4 * (lanes >> 5), lanes & 31]


def _mfma_32x32x16(a8, b8, acc):
    """v_mfma_f32_32x32x16_bf16 on host arrays [lane, 8]: A[i = l&31][k = 8(l>>5) + e], B[k = 8(l>>5) + e][j = l&31], same D map."""
    lanes = np.arange(64)
    Am = np.zeros((32, 16)); Bm = np.zeros((16, 32))
    for e in range(8):
        Am[lanes & 31, 8 * (lanes >> 5) + e] = a8[:, e]
        Bm[8 * (lanes >> 5) + e, lanes & 31] = b8[:, e]
    Dm = Am @ Bm
    for v in range(16):
        acc[v] += Dm[(v & 3) + 8 * (v >> 2) + 4 * (lanes >> 5), lanes & 31]


def _bf16(x):
    """round-to-nearest-even float32 -> bfloat16, returned as float64 values"""
    return torch.as_tensor(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def mfma_emulation(act, obs):
    """StackedActor.pack() + the kernel's index arithmetic (csrc/bsx_actor.hip, bsx_actor_core.h), emulated lane by lane on the host
    with the documented MFMA fragment maps, in float64, for ONE wave of 64 rows (obs [64, A, D]).  Returns, per agent, the layer-2
    accumulators before the LayerNorm -- acc2 (float32 path), acc2b (two bf16 terms, three products), acc2c (three terms, six
    products), each [mo 2][nt 2][v 16][lane 64] -- and `sums`: the head sums before tanh of the three paths, [64, 4] each."""
    A, D = act.n_actors, act.obs_len
    blob = act.pack().numpy()
    Dp = (D + 1) & ~1
    ow2 = 64 * Dp; osm = ow2 + 4096; ow3 = osm + 384; ob3 = ow3 + 256
    assert blob.shape == (A, ob3 + 4 + 6144)
    lanes = np.arange(64); hh = lanes >> 5
    res = []
    for a in range(A):
        W = blob[a]
        sm = W[osm:osm + 384].reshape(6, 2, 2, 16)                    # [vector][hh][mo][v]
        x = obs[:, a, :].numpy()
        acc1 = np.zeros((2, 2, 16, 64))
        for mo in range(2):
            for nt in range(2):
                acc1[mo, nt] = sm[0][hh, mo].T
        for s in range(Dp // 2):
            k = 2 * s + hh
            for mo in range(2):
                avec = W[(mo * (Dp // 2) + s) * 64:(mo * (Dp // 2) + s) * 64 + 64]
                for nt in range(2):
                    bvec = np.where(k < D, x[32 * nt + (lanes & 31), np.minimum(k, D - 1)], 0.0)
                    _mfma_32x32x2(avec, bvec, acc1[mo, nt])

        def ln(acc, gi, bi):
            for nt in range(2):
                for c in range(32):
                    cols = [c, c + 32]
                    vals = acc[:, nt][:, :, cols].reshape(-1)
                    mean = vals.mean(); rstd = 1 / np.sqrt(((vals - mean) ** 2).mean() + 1e-5)
                    for h2 in range(2):
                        for mo in range(2):
                            acc[mo, nt, :, c + 32 * h2] = np.maximum((acc[mo, nt, :, c + 32 * h2] - mean) * rstd * sm[gi, h2, mo] + sm[bi, h2, mo], 0)
        ln(acc1, 1, 2)
        acc2 = np.zeros((2, 2, 16, 64))
        for mo in range(2):
            for nt in range(2):
                acc2[mo, nt] = sm[3][hh, mo].T
        w2 = W[ow2:ow2 + 4096].reshape(2, 2, 4, 64, 4)
        for mt in range(2):
            for v in range(16):
                for mo in range(2):
                    for nt in range(2):
                        _mfma_32x32x2(w2[mo, mt, v >> 2, :, v & 3], acc1[mt, nt, v], acc2[mo, nt])
        # the same layer from the bfloat16 section: W2B[mo][s][term 3][lane][i]; "bf16x3" = three products of the first two terms per
        # K step, "bf16x6" = six products of all three terms (float32-class accuracy)
        w2b = (W[ob3 + 4:ob3 + 4 + 6144].view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(2, 4, 3, 64, 8)
        acc2b = np.zeros((2, 2, 16, 64)); acc2c = np.zeros((2, 2, 16, 64))
        for mo in range(2):
            for nt in range(2):
                acc2b[mo, nt] = sm[3][hh, mo].T; acc2c[mo, nt] = sm[3][hh, mo].T
        for s4 in range(4):
            for nt in range(2):
                xk = np.stack([acc1[s4 >> 1, nt, 8 * (s4 & 1) + i] for i in range(8)], axis=1)         # [lane, 8]
                xk = xk.astype(np.float32).astype(np.float64)                            # the kernel splits float32 accumulator values
                xh = _bf16(xk); xm = _bf16(xk - xh); xl = _bf16(xk - xh - xm)
                for mo in range(2):
                    wh, wm, wl = w2b[mo, s4, 0], w2b[mo, s4, 1], w2b[mo, s4, 2]
                    _mfma_32x32x16(wm, xh, acc2b[mo, nt]); _mfma_32x32x16(wh, xm, acc2b[mo, nt]); _mfma_32x32x16(wh, xh, acc2b[mo, nt])
                    for wa, xa in ((wl, xh), (wm, xm), (wh, xl), (wm, xh), (wh, xm), (wh, xh)):
                        _mfma_32x32x16(wa, xa, acc2c[mo, nt])
        pre = dict(acc2=acc2.copy(), acc2b=acc2b.copy(), acc2c=acc2c.copy())
        ln(acc2, 4, 5); ln(acc2b, 4, 5); ln(acc2c, 4, 5)
        w3 = W[ow3:ow3 + 256].reshape(2, 2, 16, 4); b3 = W[ob3:ob3 + 4]
        sums = {}
        for name, acc in (("f32", acc2), ("bf16x3", acc2b), ("bf16x6", acc2c)):
            out = np.zeros((64, 4))
            for nt in range(2):
                for c in range(32):
                    o = sum(acc[mt, nt, v, c + 32 * h2] * w3[h2, mt, v] for h2 in range(2) for mt in range(2) for v in range(16))
                    out[32 * nt + c] = o + b3
            sums[name] = out
        res.append(dict(pre, sums=sums))
    return res


# ------------------------------------------------------------------------------------------------ input classes: (n, seed) -> (actor, obs)
def _fresh_actor(n, seed, outputs=None):
    """The initialisation of the existing actor tests (test_fused_actor_matches_torch_fp32_reference): the reference's init with
    LayerNorm gains in [0.5, 1.5], LayerNorm biases in +-0.3 and w3 * 50; three outputs (the continuous head) where n % 3 == 0."""
    torch.manual_seed(seed)
    A, D = 2 * n, 3 * n + 2
    actor = _new(A, D, outputs if outputs is not None else (4 if n % 3 else 3))
    with torch.no_grad():
        actor.w3.mul_(50.0); actor.g1.uniform_(0.5, 1.5); actor.h1.uniform_(-0.3, 0.3); actor.g2.uniform_(0.5, 1.5); actor.h2.uniform_(-0.3, 0.3)
    return actor


def _uniform_obs(n, seed, E=None, scale=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    E = dense_games(n) if E is None else E
    return (torch.rand((E, 2 * n, 3 * n + 2), generator=g) * 2 - 1) * scale


def fresh(n, seed=0, outputs=None):
    obs = _uniform_obs(n, seed)
    obs[::7] = -1.0                                             # dead observers see all -1
    return _fresh_actor(n, 10 + n + seed, outputs), obs


def shipped(n=2, seed=0, play_rows=None):
    """The reference's shipped checkpoints (fixture g12; 2v2 networks).  Observations: the 96 recorded rows tiled over a third of the
    games, uniform rows for the rest; play_rows ([k, A, D], rows a rollout of these networks met: GPU callers) replace the last k."""
    from deep_rl_battlespace_amd.rollout import reference_checkpoint_actor
    assert n == 2
    z = np.load(os.path.join(GOLDEN, "g12_evaluation.npz"))
    actor = reference_checkpoint_actor(z, n, device="cpu")
    rec = torch.stack([torch.from_numpy(z[f"plane{i % n}/x"]) for i in range(2 * n)], 1)         # [96, A, D]
    obs = _uniform_obs(n, seed)
    k = obs.shape[0] // 3
    obs[:k] = rec.repeat((k + 95) // 96, 1, 1)[:k]
    if play_rows is not None:
        rows = play_rows.detach().cpu().float()[:obs.shape[0] // 3]
        obs[obs.shape[0] - rows.shape[0]:] = rows
    return actor, obs.contiguous()


def trained_like(n, seed=0, outputs=None):
    """Weights at the scale of the shipped checkpoints (|W2| up to 10.9, gains up to 5) where no checkpoint exists: the fresh
    initialisation with W1 and W2 * 8, LayerNorm gains ~ N(0, sd 2) -- negative and near-zero gains occur --, biases * 20."""
    actor = _fresh_actor(n, 40 + n + seed, outputs)
    g = torch.Generator().manual_seed(2000 + n + seed)
    with torch.no_grad():
        actor.w1.mul_(8.0); actor.w2.mul_(8.0)
        actor.g1.copy_(2.0 * torch.randn(actor.g1.shape, generator=g)); actor.g2.copy_(2.0 * torch.randn(actor.g2.shape, generator=g))
        for k in ("b1", "b2", "b3"):
            getattr(actor, k).mul_(20.0)
    obs = _uniform_obs(n, seed)
    obs[::7] = -1.0
    return actor, obs


def flat_rows(n, seed=0):
    """Layer 1 (weights AND bias) scaled by 1e-3: the variance of a row's 64 pre-activations is far below the LayerNorm's eps = 1e-5, so
    rsqrtf(var + eps) ~ rsqrtf(eps) carries the row.  (The bias is scaled with W1: left at +-1/8 it alone would put the variance at 5e-3.)"""
    actor, obs = fresh(n, seed)
    with torch.no_grad():
        actor.w1.mul_(1e-3); actor.b1.mul_(1e-3)
    return actor, obs


def dead_half(n, seed=0):
    """Every second game all -1, as dead observers see it."""
    actor, obs = fresh(n, seed)
    obs[::2] = -1.0
    return actor, obs


TILE_EDGES = (31, 32, 63, 64, 255, 256)                       # last / first row of a 32-row tile, of a wave, of a 256-row workgroup
EDGE_VALUES = (7.5, -7.5, 3.25, -0.5, 8.0, -8.0)


def wide_obs(n, seed=0):
    """Observations in +-8 (a learner feeding unnormalised rows); one game at each tile boundary carries a distinct constant row."""
    actor = _fresh_actor(n, 10 + n + seed)
    obs = _uniform_obs(n, seed, scale=8.0)
    for e, v in zip(TILE_EDGES, EDGE_VALUES):
        obs[e] = v
    return actor, obs


CLASSES = {"fresh": fresh, "shipped": shipped, "trained_like": trained_like, "flat_rows": flat_rows, "dead_half": dead_half, "wide_obs": wide_obs}
COMBOS = [(c, n) for c, sizes in CLASS_SIZES.items() for n in sizes]


def localisation_case(layer, launch, n=4, E=1000, seed=0):
    """One launch of the localisation test: A = 2n agents, agent a isolating hidden neuron j = launch * A + a of `layer` (1 or 2).
    LayerNorm gains 1 and biases 0; b1, b2, b3 random and non-zero; layer 1: W2 zero but for row j, so the output depends on the input
    through h1[j] alone -- one accumulator register of one lane half -- as layer 2 of b2 + h1[j] * W2[j]; layer 2: W3 zero but for row
    j, the output h2[j] * W3[j] + b3 a direct read of that register.  b1 (b2) re-centre the neuron's pre-activation so that it is active
    on a good share of the rows whatever its weights: the condition (>= a quarter) is checked on the reference by the CPU tests.
    Returns (actor, obs, neurons, active): active[a] = the share of rows with h[j] > 0, from the float64 reference."""
    A, D = 2 * n, 3 * n + 2
    torch.manual_seed(7000 + 100 * layer + launch + seed)
    actor = _new(A, D, 4)
    g = torch.Generator().manual_seed(7100 + 100 * layer + launch + seed)
    obs = torch.rand((E, A, D), generator=g) * 2 - 1
    neurons = [launch * A + a for a in range(A)]
    with torch.no_grad():
        actor.w3.mul_(50.0); actor.b3.mul_(50.0); actor.b1.mul_(0.25)
        if layer == 1:
            keep = torch.zeros_like(actor.w2)
            for a, j in enumerate(neurons):
                keep[a, j] = 1.0
            actor.w2.mul_(keep)
        else:
            keep = torch.zeros_like(actor.w3)
            for a, j in enumerate(neurons):
                keep[a, j] = 1.0
            actor.w3.copy_(keep * torch.sign(actor.w3) * (0.05 + actor.w3.abs() * (2.0 / 3.0)))   # the one row: every entry in 0.05 .. 0.15
            # the pre-activation of neuron j of layer 2 = b2[j] + h1 . W2[:, j]: a column with a one-sided sum would sit below the
            # row mean on nearly every row; b2 takes the column's mean over the rows out (float64 reference, rounded once)
            a64 = to_float64(actor)
            x = obs.double().transpose(0, 1)
            h = torch.relu(a64._ln(torch.baddbmm(a64.b1, x, a64.w1), a64.g1, a64.h1))
            pre = torch.bmm(h, a64.w2)
            actor.b2.copy_((actor.b2.double() * 0.25 - pre.mean(1, keepdim=True) + pre.mean((1, 2), keepdim=True)).float())
        a64 = to_float64(actor)
        x = obs.double().transpose(0, 1)
        h = torch.relu(a64._ln(torch.baddbmm(a64.b1, x, a64.w1), a64.g1, a64.h1))
        if layer == 2:
            h = torch.relu(a64._ln(torch.baddbmm(a64.b2, h, a64.w2), a64.g2, a64.h2))
        active = [float((h[a, :, j] > 0).double().mean()) for a, j in enumerate(neurons)]
    return actor, obs, neurons, active


# ------------------------------------------------------------------------------------------------ errors, bounds, budgets
def stats(err):
    return float(np.max(err)), float(np.mean(err))


@functools.lru_cache(maxsize=None)
def reference_errors(cls, n, seed=0):
    """(y64, e_t, e_m2, e_m3) of an input class on the CPU: the float64 head sums, torch float32's |error| against them, the two- and
    three-term split models' |error| against them.  Cached: the three precision modes of one (class, n) share it."""
    actor, obs = CLASSES[cls](n, seed)
    return errors_of(actor, obs)


def errors_of(actor, obs):
    y = head_sums64(actor, obs)
    return y, np.abs(head_sums32(actor, obs) - y), np.abs(split_model64(actor, obs, 2) - y), np.abs(split_model64(actor, obs, 3) - y)


def bounds(mode, e_t, e_m2, e_m3):
    """(max bound, mean bound) of a precision mode's head sums.
    f32: mean(e_k) <= 2 mean(e_t), max(e_k) <= 4 max(e_t).  Split modes: mean(e_k) <= 2 (mean(e_m) + mean(e_t)), max(e_k) <= 4 (max(e_m) +
    max(e_t)) with e_m the split model of the mode's term count.  yardstick_util.FACTORS says where 2 and 4 come from."""
    fm, fx = F32_FACTORS
    if mode == "f32":
        return fx * e_t.max(), fm * e_t.mean()
    e_m = e_m2 if TERMS[mode] == 2 else e_m3
    return fx * (e_m.max() + e_t.max()), fm * (e_m.mean() + e_t.mean())


def score_budget(y64, B):
    """|score - tanh(y64)| <= sech^2(y64) * B + 4 * 2^-24: the head-sum bound through tanh's slope, plus tanhf's own few ulps of a
    value below 1.  On a saturated output this says no more than that tanh saturates; the body's error shows where |y64| is small."""
    return B / np.cosh(y64) ** 2 + 4 * ULP1


def ulps32(got, want64):
    """|got - want| in float32 spacings at |want|."""
    w32 = np.abs(want64).astype(np.float32)
    return np.abs(got - want64) / np.maximum(np.spacing(w32).astype(np.float64), 2.0 ** -149)


def kernel_outputs(actor, obs, n, mode):
    """The stand-alone kernel on the GPU: (scores [E, A, na], head sums [E, A, na]) as float64 arrays.  actor / obs live on the CPU or the
    GPU.  The head sums are read through as_critics, one launch per head column; every launch must write the same score rows."""
    from deep_rl_battlespace_amd.rollout import FusedActor
    actor = actor.to("cuda")
    obs = obs.to("cuda").contiguous()
    E, A = obs.shape[:2]
    fa = FusedActor(actor, n, precision=mode)
    sums, first = [], None
    for c in as_critics(actor):
        scores = torch.full((E, A, 4), 7.0, device="cuda")
        out = torch.full((E, A), 7.0, device="cuda")
        fa.forward_into(obs, scores, seq=1, value=dict(weights=c.pack(), out=out))
        torch.cuda.synchronize()
        assert first is None or torch.equal(first, scores)
        first = scores
        sums.append(out)
    na = actor.n_actions
    assert na == 4 or bool((first[..., na:] == 0).all())
    return first[..., :na].double().cpu().numpy(), torch.stack(sums, -1).double().cpu().numpy()
