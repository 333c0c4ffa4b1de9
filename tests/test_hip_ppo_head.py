"""The PPO loss head on the MI355X (bsx_ppo_head, learner.ppo_head): both gradient tensors, log_std's gradient and the statistics against
the float64 restatement of the contract at a small multiple of what torch float32 autograd itself loses on the same inputs
(tests/ppo_head_util.py: the kinks of the loss left out by construction), teams from 1 to 16 a side; ragged row counts between guard slabs; masked-out elements
holding NaN and infinities; the same bits on every call and from a captured graph of a whole minibatch; ties of the arg-max; refusals."""
import numpy as np
import pytest
import torch

import ppo_head_util as P
from guard_util import Buffers

pytestmark = pytest.mark.gpu

RAGGED = (1, 31, 33, 63, 65, 255, 257)
RAGGED_CASES = [(r, n) for n in (1, 3) for r in RAGGED] + [(r, n) for n in (11, 16) for r in (1, 33, 65)]      # (rows, n)
KW = dict(clip=P.CLIP, c_v=P.C_V, c_e=P.C_E)


def _call(inp, kind, vold=True, guarded=False, fill=7.0):
    """learner.ppo_head on (guarded) device buffers whose outputs start at `fill`: (outputs as device tensors, damaged buffers)."""
    from deep_rl_battlespace_amd.learner import ppo_head, ppo_head_workspace_bytes
    rows, A = inp["adv"].shape
    B = Buffers(guarded)
    dev = {}
    for k, v in inp.items():
        dev[k] = B(k, tuple(v.shape), v.dtype)
        dev[k].copy_(v)
    out = (B("g_pi", (rows, A, 4), torch.float32, init=fill), B("g_v", (rows, A, 4), torch.float32, init=fill),
           B("g_log_std", (A, 3), torch.float32, init=fill), B("stats", (8,), torch.float64, init=fill))
    ws = B("workspace", (ppo_head_workspace_bytes(rows, A) // 8,), torch.int64, init=-1)
    extra = dict(temperature=P.TAU) if kind == "categorical" else dict(log_std=dev["log_std"])
    if vold:
        extra.update(v_old=dev["v_old"], vclip=P.VCLIP)
    res = ppo_head(kind, dev["y"], dev["v"], dev["rec"], dev["logp_old"], dev["adv"], dev["ret"], dev["mask"], out=out, workspace=ws, **KW, **extra)
    torch.cuda.synchronize()
    assert res.g_pi is out[0] and res.g_v is out[1] and res.stats is out[3] and (res.g_log_std is out[2]) == (kind == "gaussian")
    return res, B.stray()


def _numpy(res):
    return dict(g_pi=res.g_pi.double().cpu().numpy(), g_v=res.g_v.double().cpu().numpy(), stats=res.stats.cpu().numpy(),
                g_log_std=res.g_log_std.double().cpu().numpy() if res.g_log_std is not None else None)


def _same_bits(a, b):
    return all(x is None and y is None or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("vold", [True, False], ids=["vclip", "plain"])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "R%d-n%d" % s)
def test_gradients_and_statistics_stay_within_the_float32_yardstick_of_the_float64_contract(shape, kind, vold):
    inp, ref, yard, e_stats, e_ls = P.case(kind, *shape, vold)
    res, _ = _call(inp, kind, vold)
    P.check(_numpy(res), ref, yard, e_stats, e_ls, kind, f"HEAD {kind} R={shape[0]} n={shape[1]} {'vclip' if vold else 'plain'}")


@pytest.mark.parametrize("kind", P.KINDS)
def test_workgroups_that_take_more_than_one_tile_keep_the_bounds_and_their_guards(kind):
    """Up to 2 048 tiles the head pass has a workgroup per tile; beyond, every workgroup walks J > 1 consecutive tiles and adds its
    statistics and log_std terms over them.  The ladder is not run at this size: the step is the one it ends on at (1000, 1), and the
    yardstick's own error is that of the given row order alone (no permutations: a tighter bound, not a wider one)."""
    inp, ref, yard, e_stats, e_ls = P.case(kind, *P.LARGE, True, step=P.LARGE_STEP[kind], perms=0)
    res, stray = _call(inp, kind, True, guarded=True)
    assert not stray, stray
    P.check(_numpy(res), ref, yard, e_stats, e_ls, kind, f"LARGE {kind} R={P.LARGE[0]} n={P.LARGE[1]}")


# ---------------------------------------------------------------------------------------------------- 2. ragged sizes, guards
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("rows,n", RAGGED_CASES)
def test_ragged_row_counts_keep_their_guards_overwrite_every_output_and_keep_the_float64_bound(rows, n, kind):
    inp, ref, yard, e_stats, e_ls = P.case(kind, *P.RAGGED_SHAPES[n], True, cut=rows)
    assert inp["adv"].shape == (rows, 2 * n)
    fills = []
    for fill in (7.0, -3.0):                                           # an output float that keeps BOTH fills was not written
        res, stray = _call(inp, kind, True, guarded=True, fill=fill)
        assert not stray, stray
        fills.append([t.clone() for t in res if t is not None])
    assert _same_bits(*fills)
    P.check(_numpy(res), ref, yard, e_stats, e_ls, kind, f"RAGGED {kind} rows={rows} n={n}")


# ---------------------------------------------------------------------------------------------------- 2b. inputs off a 16-byte boundary
def _placed(t, offset, fill):
    """A device copy of `t` that starts `offset` elements into a 16-byte aligned slab holding `fill` around it."""
    slab = torch.full((t.numel() + 32,), fill, dtype=t.dtype, device="cuda")
    assert slab.data_ptr() % 16 == 0
    view = slab[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() == slab.data_ptr() + offset * t.element_size() and view.is_contiguous()
    return view


def _count_regime(offset, M):
    """Which parts of bsx_ppo_count_kernel's split see a mask of M bytes that starts `offset` bytes past a 16-byte boundary: the bytes
    before the first boundary (head, cut to M), whole 16-byte groups (body), the rest (tail) -- its pointer arithmetic restated."""
    head = (16 - offset % 16) % 16
    if head > M:
        return "cut head"                                                # M < head: every byte is a head byte, no boundary is reached
    groups = (M - head) // 16
    tail = M - head - 16 * groups
    return "+".join(name for name, there in (("head", head), ("body", groups), ("tail", tail)) if there)


UNALIGNED_ROWS = {1: (1, 3, 7, 9), 3: (1, 3)}                            # n -> rows with M = A rows in {2, 6, 14, 18}
assert sorted({2 * n * r for n, rs in UNALIGNED_ROWS.items() for r in rs}) == [2, 6, 14, 18]


@pytest.mark.parametrize("vold", [True, False], ids=["vclip", "plain"])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("shape", [(257, 1), (97, 3)], ids=lambda s: "R%d-n%d" % s)
def test_records_off_a_sixteen_byte_boundary_give_the_bits_of_fresh_copies(shape, kind, vold):
    """A learner's minibatch hands the head views of a rollout's records: the float32 [R][A] arrays at any 4-byte offset, the mask at any
    byte (the header says so).  The mask at every byte offset 0 .. 15 and the floats at every float offset 0 .. 3 of an aligned slab,
    at the full shape and at M = A R = 2, 6, 14, 18 mask bytes (the count pass's head alone, head and tail, and fewer bytes than its
    head): every output has the bits of the call on freshly allocated copies, and N is the host's count."""
    from deep_rl_battlespace_amd.learner import ppo_head
    n = shape[1]
    full = P.build(kind, *shape, 0.1)
    seen = set()
    for rows in (shape[0],) + UNALIGNED_ROWS[n]:
        inp = P.head(full, rows)
        M = rows * 2 * n
        dev = {k: v.contiguous().to("cuda") for k, v in inp.items()}
        extra = dict(temperature=P.TAU) if kind == "categorical" else dict(log_std=dev["log_std"])

        def call(t):
            kw = dict(extra, v_old=t["v_old"], vclip=P.VCLIP) if vold else extra
            return ppo_head(kind, dev["y"], t["v"], dev["rec"], t["logp_old"], t["adv"], t["ret"], t["mask"], **KW, **kw)
        want = call(dev)
        count = int((inp["mask"] != 0).sum())
        assert float(want.stats[0]) == count
        for offset in range(16):
            at = {k: _placed(inp[k].contiguous(), offset % 4, float("nan")) for k in ("v", "logp_old", "adv", "ret", "v_old")}
            at["mask"] = _placed(inp["mask"].contiguous(), offset, 1)                 # set bytes around it: a byte counted beyond M shows in N
            assert at["mask"].data_ptr() % 16 == offset and all(at[k].data_ptr() % 16 == 4 * (offset % 4) for k in ("v", "adv"))
            got = call(at)
            torch.cuda.synchronize()
            assert _same_bits(got, want), (rows, offset)
            assert float(got.stats[0]) == count, (rows, offset)
            if rows != shape[0]:
                seen.add((_count_regime(offset, M), M))
    print(kind, shape, sorted(seen))
    # by hand: 2 bytes at offset 3 end before the boundary, at 14 on it, at 15 beyond it; 18 bytes at 14 are head and one whole group
    want = ({("cut head", 2), ("head", 2), ("head+tail", 2), ("tail", 2), ("head", 14), ("head+tail", 14), ("body+tail", 18), ("head+body", 18),
             ("head+body+tail", 18)} if n == 1 else {("cut head", 6), ("head", 6), ("head+tail", 6), ("tail", 6), ("head+body", 18), ("head+tail", 18)})
    assert seen >= want, sorted(want - seen)


# ---------------------------------------------------------------------------------------------------- 3. the mask
@pytest.mark.parametrize("kind", P.KINDS)
def test_masked_out_elements_write_plus_zero_and_reach_nothing_whatever_they_hold(kind):
    for shape in ((257, 3), (97, 13)):                                  # 13 a side: 234 of a workgroup's 256 threads at work
        _masked_out_elements(kind, shape)


def _masked_out_elements(kind, shape):
    inp, _, _ = P.inputs(kind, *shape)
    off = inp["mask"] == 0
    assert 100 < int(off.sum()) < off.numel() - 100
    bad = {k: v.clone() for k, v in inp.items()}
    for i, k in enumerate(("y", "v", "rec", "logp_old", "adv", "ret", "v_old")):
        bad[k][off] = (float("nan"), float("inf"), -float("inf"))[i % 3]
    clean, _ = _call(inp, kind)
    dirty, _ = _call(bad, kind)
    assert _same_bits(clean, dirty)
    for g in (dirty.g_pi, dirty.g_v):
        assert bool((g.view(torch.int32)[off.to("cuda")] == 0).all())           # +0: not -0, not small
        assert bool(torch.isfinite(g).all())
    assert bool((dirty.g_v[..., 1:].view(torch.int32) == 0).all()) and (kind == "categorical" or bool((dirty.g_pi[..., 3].view(torch.int32) == 0).all()))
    assert bool(torch.isfinite(dirty.stats).all()) and float(dirty.stats[0]) == float((~off).sum())
    # no masked row at all, NaN everywhere: every output is 0
    bad["mask"] = torch.zeros_like(bad["mask"])
    for k in ("y", "v", "rec", "logp_old", "adv", "ret", "v_old"):
        bad[k][:] = float("nan")
    none, _ = _call(bad, kind)
    for t in none:
        assert t is None or bool((t.view(torch.int32) == 0).all())


# ---------------------------------------------------------------------------------------------------- 4. determinism, graphs
@pytest.mark.parametrize("kind", P.KINDS)
def test_the_same_inputs_give_the_same_bits_on_every_call(kind):
    inp, _, _ = P.inputs(kind, 1000, 1)
    a, _ = _call(inp, kind)
    b, _ = _call(inp, kind, fill=-1.0)
    assert _same_bits(a, b)
    wide, _, _ = P.inputs(kind, 512, 4)
    assert _same_bits(_call(wide, kind, False)[0], _call(wide, kind, False, fill=-1.0)[0])
    widest, _, _ = P.inputs(kind, 200, 16)                              # 25 workgroups; two parts per log_std column, partial rows of 104
    assert _same_bits(_call(widest, kind)[0], _call(widest, kind, fill=-1.0)[0])


@pytest.mark.parametrize("kind", P.KINDS)
def test_a_captured_minibatch_replays_to_the_bits_of_the_eager_one(kind):
    """pack -> forward -> head -> both backward calls (PPOLearner.minibatch_grads), enqueued on the capturing stream."""
    import ppo_learner_util as L
    from deep_rl_battlespace_amd.learner import PPOLearner
    ro = L.small_rollout(kind)
    learner = PPOLearner(ro, clip=P.CLIP, c_v=P.C_V, c_e=P.C_E, vclip=P.VCLIP, epochs=1, minibatches=1)
    L.nudge(ro.actor, 0.1)                                              # off the policy that played: ratios leave 1
    eager = [[t.clone() for t in learner.minibatch_grads(0, ro.T) if t is not None] for _ in range(2)]
    torch.cuda.synchronize()
    assert _same_bits(*eager)
    assert float(eager[0][-1][0]) > 500 and bool(torch.isfinite(eager[0][0]).all()) and float(eager[0][0].abs().max()) > 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        learner.minibatch_grads(0, ro.T)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = [t for t in learner.minibatch_grads(0, ro.T) if t is not None]
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, eager[0])


# ---------------------------------------------------------------------------------------------------- 5. the arg-max
def test_ties_in_rec_take_the_first_maximum_as_the_step_kernel_does():
    inp = {k: v.clone() for k, v in P.build("categorical", 64, 1, 0.1).items()}
    inp["mask"][:] = 1
    inp["rec"][:, 0] = torch.tensor([0.5, 2.0, 2.0, -1.0])
    inp["rec"][:, 1] = torch.tensor([1.0, 1.0, 1.0, 1.0])
    res, _ = _call(inp, "categorical")
    first = P.reference(inp, "categorical")["g_pi"]
    scale = np.abs(first).max()
    assert np.abs(_numpy(res)["g_pi"] - first).max() <= 1e-5 * scale
    last = dict(inp, rec=inp["rec"].clone())
    last["rec"][:, 0, 2] += 1e-3                                        # what taking the LAST maximum would have played
    last["rec"][:, 1, 3] += 1e-3
    assert np.abs(P.reference(last, "categorical")["g_pi"] - first).max() > 1e-2 * scale


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_ppo_head_refuses_what_it_documents():
    from deep_rl_battlespace_amd.learner import ppo_head
    inp = {k: v.to("cuda") for k, v in P.build("gaussian", 9, 1, 0.1).items()}
    args = lambda **o: [o.get(k, inp[k]) for k in ("y", "v", "rec", "logp_old", "adv", "ret", "mask")]      # noqa: E731
    gauss = dict(KW, log_std=inp["log_std"])
    assert ppo_head("gaussian", *args(), **gauss).g_log_std.shape == (2, 3)
    assert ppo_head(0, *args(), **KW, temperature=0.5).g_log_std is None
    with pytest.raises(ValueError, match="kind"):
        ppo_head("beta", *args(), **KW)
    with pytest.raises(ValueError, match="GPU"):
        ppo_head("categorical", *args(y=inp["y"].cpu()), **KW)
    with pytest.raises(ValueError, match="y must"):
        ppo_head("categorical", *args(y=inp["y"][..., :3]), **KW)
    with pytest.raises(ValueError, match="even A"):
        ppo_head("categorical", *args(y=inp["y"][:, :1]), **KW)
    for name in ("v", "rec", "logp_old", "adv", "ret", "mask"):
        with pytest.raises(ValueError, match=name + " must have shape"):
            ppo_head("categorical", *args(**{name: inp[name][:8]}), **KW)
        with pytest.raises(TypeError, match=name + " must be"):
            ppo_head("categorical", *args(**{name: inp[name].to(torch.float64)}), **KW)
        with pytest.raises(ValueError, match=name + " is on"):
            ppo_head("categorical", *args(**{name: inp[name].cpu()}), **KW)
    with pytest.raises(ValueError, match="adv must be contiguous"):
        ppo_head("categorical", *args(adv=torch.zeros((2, 9), device="cuda").t()), **KW)
    with pytest.raises(TypeError, match="ret must be a torch.Tensor"):
        ppo_head("categorical", *args(ret=None), **KW)
    for bad in (dict(clip=0.0), dict(clip=1.0), dict(clip=float("nan")), dict(c_v=-1.0), dict(c_e=float("inf")), dict(temperature=0.0),
                dict(clip="a")):
        with pytest.raises(ValueError, match=next(iter(bad))):
            ppo_head("categorical", *args(), **dict(KW, **bad))
    with pytest.raises(ValueError, match="go together"):
        ppo_head("categorical", *args(), **KW, v_old=inp["v_old"])
    with pytest.raises(ValueError, match="go together"):
        ppo_head("categorical", *args(), **KW, vclip=0.2)
    with pytest.raises(ValueError, match="vclip"):
        ppo_head("categorical", *args(), **KW, v_old=inp["v_old"], vclip=0.0)
    with pytest.raises(ValueError, match="v_old must have shape"):
        ppo_head("categorical", *args(), **KW, v_old=inp["v_old"][:8], vclip=0.2)
    with pytest.raises(ValueError, match="needs log_std"):
        ppo_head("gaussian", *args(), **KW)
    with pytest.raises(ValueError, match="log_std must have shape"):
        ppo_head("gaussian", *args(), **KW, log_std=inp["log_std"][:, :2])
    with pytest.raises(ValueError, match="belongs to"):
        ppo_head("categorical", *args(), **gauss)
    with pytest.raises(ValueError, match="workspace"):
        ppo_head("categorical", *args(), **KW, workspace=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out g_v must have shape"):
        ppo_head("categorical", *args(), **KW, out=(torch.zeros_like(inp["y"]), torch.zeros_like(inp["v"]), None,
                                                     torch.zeros(8, dtype=torch.float64, device="cuda")))
    with pytest.raises(TypeError, match="out stats must be"):
        ppo_head("categorical", *args(), **KW, out=(torch.zeros_like(inp["y"]), torch.zeros_like(inp["y"]), None, torch.zeros(8, device="cuda")))
