"""The float64 restatement of the PPO loss head's contract (tests/ppo_head_util.py) against torch float64 autograd of the loss as a user
writes it, and the conditions the GPU tests' inputs must meet: the kink filter's 1 % cap, the step ladder;
and the C entry point's refusals, which happen before any launch.  No GPU."""
import numpy as np
import pytest
import torch

import ppo_head_util as P


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("vold", [True, False], ids=["vclip", "plain"])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "R%d-n%d" % s)
def test_the_restatement_is_float64_autograd_of_the_loss_a_user_writes(shape, kind, vold):
    inp, _, _ = P.inputs(kind, *shape)
    ref = P.reference(inp, kind, vold)
    t64 = P.torch_loss(inp, kind, torch.float64, vold)
    for k in ("g_pi", "g_v") + (("g_log_std",) if kind == "gaussian" else ()):
        assert _rel(ref[k], t64[k]) <= 1e-12, (k, _rel(ref[k], t64[k]))
    assert ref["g_log_std"] is None or kind == "gaussian"
    assert ref["stats"][0] == t64["stats"][0] == float((inp["mask"] != 0).sum()) and ref["stats"][7] == 0.0
    for i in range(1, 7):
        assert abs(ref["stats"][i] - t64["stats"][i]) <= 1e-12 * max(abs(t64["stats"][i]), 1e-300), (i, ref["stats"][i], t64["stats"][i])
    # the columns no network output feeds: +0
    assert not ref["g_v"][..., 1:].any() and (kind == "categorical" or not ref["g_pi"][..., 3].any())
    # value clipping is at work in these inputs, and leaves when v_old is not given
    plain = P.reference(inp, kind, False)
    assert vold or np.array_equal(ref["g_v"], plain["g_v"])
    assert not np.array_equal(P.reference(inp, kind, True)["g_v"], plain["g_v"])


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "R%d-n%d" % s)
def test_the_filter_removes_at_most_one_percent_and_the_ladder_finds_clipped_and_unclipped_rows(shape, kind):
    inp, step, masked = P.inputs(kind, *shape)
    kept, outside, clipped = P.ladder_figures(inp, kind)
    print(kind, shape, "step", step, "masked", masked, "kept", kept, f"removed {100 * (masked - kept) / masked:.2f} %; outside the interval", outside,
          f"({100 * outside / kept:.1f} %), clipped", clipped)
    assert masked - kept <= P.FILTER_CAP * masked
    assert 0.05 * kept <= outside <= 0.6 * kept
    assert clipped >= 20 and outside - clipped >= 20
    # the step was chosen as the smallest one: every smaller step of the ladder misses the 5 % .. 60 % window
    for s in P.LADDER[:P.LADDER.index(step)]:
        k, o, _ = P.ladder_figures(P.kink_filter(P.build(kind, *shape, s), kind), kind)
        assert not 0.05 * k <= o <= 0.6 * k
    # every row near a kink is out: the ratio and the value difference keep their distance on the kept rows
    ref = P.reference(inp, kind)
    on = inp["mask"].numpy() != 0
    assert np.abs(ref["ratio"][on] - (1 - P.CLIP)).min() >= P.KINK and np.abs(ref["ratio"][on] - (1 + P.CLIP)).min() >= P.KINK
    assert np.abs(ref["vdiff"][on] - P.VCLIP).min() >= P.KINK


@pytest.mark.parametrize("kind", P.KINDS)
def test_the_large_case_meets_the_same_conditions_at_its_fixed_step(kind):
    inp, step, masked = P.inputs(kind, *P.LARGE, P.LARGE_STEP[kind])
    assert step == P.inputs(kind, *P.SHAPES[0])[1]                                # the step the ladder ends on at (1000, 1)
    kept, outside, clipped = P.ladder_figures(inp, kind)
    print(kind, P.LARGE, "step", step, "masked", masked, "kept", kept, "outside", outside, "clipped", clipped)
    assert masked - kept <= P.FILTER_CAP * masked and 0.05 * kept <= outside <= 0.6 * kept and clipped >= 20 and outside - clipped >= 20
    assert inp["adv"].numel() > 2048 * 256                                         # more tiles than workgroups


@pytest.mark.parametrize("kind", P.KINDS)
def test_masked_out_rows_with_nan_inputs_leave_the_restatement_unchanged(kind):
    for shape in ((257, 3), (97, 13)):
        _masked_out_rows(kind, shape)


def _masked_out_rows(kind, shape):
    inp, _, _ = P.inputs(kind, *shape)
    ref = P.reference(inp, kind)
    off = inp["mask"] == 0
    assert int(off.sum()) > 100
    bad = {k: v.clone() for k, v in inp.items()}
    for i, k in enumerate(("y", "v", "rec", "logp_old", "adv", "ret", "v_old")):
        bad[k][off] = (float("nan"), float("inf"), -float("inf"))[i % 3]
    got = P.reference(bad, kind)
    for k in ("g_pi", "g_v", "stats") + (("g_log_std",) if kind == "gaussian" else ()):
        assert np.array_equal(got[k], ref[k]), k
    assert not np.signbit(got["g_pi"][off.numpy()]).any() and not got["g_pi"][off.numpy()].any()
    # no masked row at all: every output is 0
    none = dict(inp, mask=torch.zeros_like(inp["mask"]))
    z = P.reference(none, kind)
    assert not z["g_pi"].any() and not z["g_v"].any() and not z["stats"].any() and (z["g_log_std"] is None or not z["g_log_std"].any())


def test_ties_in_rec_take_the_first_maximum():
    inp = {k: v.clone() for k, v in P.head(P.build("categorical", 8, 1, 0.1), 8).items()}
    inp["mask"][:] = 1
    inp["rec"][:, 0] = torch.tensor([0.5, 2.0, 2.0, -1.0])
    inp["rec"][:, 1] = torch.tensor([1.0, 1.0, 1.0, 1.0])
    ref = P.reference(inp, "categorical")
    t64 = P.torch_loss(inp, "categorical", torch.float64)
    assert _rel(ref["g_pi"], t64["g_pi"]) <= 1e-12
    moved = dict(inp, rec=inp["rec"].clone())
    moved["rec"][:, 0, 2] = 2.5                                         # now the third column wins: another action, another gradient
    assert not np.array_equal(P.reference(moved, "categorical")["g_pi"], ref["g_pi"])


def test_the_c_entry_point_refuses_what_the_header_documents_before_any_launch():
    """Fake addresses only: every call is refused before anything reaches HIP, in the documented order (calls that break an argument
    rule and an alignment rule at once pin it)."""
    import ctypes
    from deep_rl_battlespace_amd import _lib as L
    lib = L.load()
    A16, A4, A1 = 4096, 4096 + 4, 4096 + 1
    ARG, ALIGN = -1, -2
    fields = [f for f, _ in L.BsxPpoIo._fields_]

    def call(R=100, A=2, kind=0, tau=0.7, clip=0.2, vclip=0.2, c_v=0.5, c_e=0.01, ws=A16, stats=A16, io=True, **ptr):
        st = L.BsxPpoIo(**{f: ptr.get(f, None if f == "v_old" else A16) for f in fields})
        return lib.bsx_ppo_head(ctypes.byref(st) if io else None, R, A, kind, tau, clip, vclip, c_v, c_e, ws, stats, None)

    nan, inf = float("nan"), float("inf")
    arg = [dict(io=False), dict(ws=None), dict(stats=None)] + [{f: None} for f in fields if f not in ("v_old", "log_std", "g_log_std")]
    arg += [dict(kind=2), dict(kind=-1), dict(clip=0.0), dict(clip=1.0), dict(clip=nan), dict(c_v=-0.5), dict(c_v=nan), dict(c_e=-1.0),
            dict(c_e=inf), dict(tau=0.0), dict(tau=nan), dict(tau=inf), dict(v_old=A16, vclip=0.0), dict(v_old=A16, vclip=nan),
            dict(R=0), dict(R=(1 << 30) + 1), dict(A=0), dict(A=3), dict(A=34), dict(kind=1, log_std=None), dict(kind=1, g_log_std=None)]
    for kw in arg:
        assert call(**kw) == ARG, kw
    align = [{f: A4} for f in ("y", "rec", "g_pi", "g_v")] + [{f: A1} for f in ("v", "logp_old", "adv", "ret", "v_old")]
    align += [dict(kind=1, log_std=A1), dict(kind=1, g_log_std=A1), dict(ws=A4), dict(stats=A4)]
    for kw in align:
        assert call(**kw) == ALIGN, kw
    # what is not read is not judged: a temperature with kind 1, vclip without v_old, log_std with kind 0; mask at any byte
    for kw in (dict(kind=1, tau=0.0), dict(vclip=nan), dict(log_std=None, g_log_std=None), dict(log_std=A1)):
        assert call(y=A4, **kw) == ALIGN, kw
    # the order: argument rules before alignment rules
    for kw in (dict(y=A4, kind=2), dict(y=A4, clip=0.0), dict(ws=A4, R=0), dict(stats=A4, A=3), dict(g_v=A4, kind=1, log_std=None),
               dict(v=A1, rec=None)):
        assert call(**kw) == ARG, kw
    nb = ctypes.c_size_t()
    assert lib.bsx_ppo_head_workspace_bytes(1000, 2, ctypes.byref(nb)) == 0 and nb.value >= 2048 + 8 * 14 and nb.value % 8 == 0
    small = nb.value
    assert lib.bsx_ppo_head_workspace_bytes(2097152, 2, ctypes.byref(nb)) == 0 and small < nb.value < 1 << 20
    assert lib.bsx_ppo_head_workspace_bytes(1 << 30, 32, ctypes.byref(nb)) == 0 and nb.value < 1 << 24     # bounded: more tiles per workgroup
    for R_, A_ in ((0, 2), ((1 << 30) + 1, 2), (10, 0), (10, 3), (10, 34)):
        assert lib.bsx_ppo_head_workspace_bytes(R_, A_, ctypes.byref(nb)) == ARG
    assert lib.bsx_ppo_head_workspace_bytes(10, 2, None) == ARG
