"""The free-width optimiser step with Polyak targets without a GPU: both entry points are declared, exported and bound, the workspace
follows its formula, every refusal of bsx_adam_step_mlp fires on fake addresses before any launch and in the documented order, the two
older entries refuse what they refused, the float64 restatement's Polyak line is torch's float64 lerp, and the binding names the argument it
refuses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_mlp_util as MU
import adam_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, ALIGN = -1, -2
A16, A8, A4, A1 = 4096, 4096 + 8, 4096 + 4, 4096 + 1


def _L():
    from deep_rl_battlespace_amd import _lib
    return _lib


def test_both_entries_are_declared_exported_and_bound_and_the_abi_version_stays():
    L = _L()
    hdr = open(os.path.join(ROOT, "include", "battlespace_hip.h")).read()
    lib = L.load()
    for name in ("bsx_adam_step_mlp_workspace_bytes", "bsx_adam_step_mlp"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M) and name in L.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define BSX_ABI_VERSION (\d+)", hdr).group(1) == "14" and lib.bsx_abi_version() == 14 == L.ABI_VERSION
    for struct in ("BsxAdamTarget", "BsxAdamTargets"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        fields = re.findall(r"(\w+)(?:\[\d+\])?\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f for f, _ in getattr(L, struct)._fields_], struct
    assert ctypes.sizeof(L.BsxAdamTarget) == 11 * 8 and ctypes.sizeof(L.BsxAdamTargets) == 22 * 8
    # the entries that stay: the signatures they had; the new one takes A, D, group and the targets
    assert len(L.SIGNATURES["bsx_adam_step"][1]) == 5 and len(L.SIGNATURES["bsx_adam_step_shared"][1]) == 6
    assert L.SIGNATURES["bsx_adam_step_mlp"][1] == [ctypes.POINTER(L.BsxAdamIo), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.POINTER(L.BsxAdamTargets), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    import deep_rl_battlespace_amd as bsx
    from deep_rl_battlespace_amd import learner
    assert bsx.mlp_adam_step is learner.mlp_adam_step and bsx.mlp_adam_step_workspace_bytes is learner.mlp_adam_step_workspace_bytes
    assert "mlp_adam_step" in bsx.__all__ and "mlp_adam_step_workspace_bytes" in bsx.__all__
    assert learner.HYPER[5] == "tau" and learner.HYPER[:5] == ("lr", "beta1", "beta2", "eps", "max_grad_norm")


def test_the_workspace_is_eight_scalars_and_one_partial_per_row_and_for_log_std():
    from deep_rl_battlespace_amd import learner
    lib, nb, old = _L().load(), ctypes.c_size_t(), ctypes.c_size_t()
    for A in (1, 2, 3, 5, 31, 32):
        for nets in (1, 2):
            assert lib.bsx_adam_step_mlp_workspace_bytes(A, nets, ctypes.byref(nb)) == 0
            assert nb.value == 8 * (8 + nets * A + 1) == learner.mlp_adam_step_workspace_bytes(A, nets)
            if A % 2 == 0:                                                       # the older entry returns what it returned
                assert lib.bsx_adam_step_workspace_bytes(A // 2, nets, ctypes.byref(old)) == 0 and old.value == nb.value
    for A, nets in ((0, 1), (33, 1), (-1, 2), (4, 0), (4, 3)):
        assert lib.bsx_adam_step_mlp_workspace_bytes(A, nets, ctypes.byref(nb)) == ARG, (A, nets)
    assert lib.bsx_adam_step_mlp_workspace_bytes(4, 1, None) == ARG
    for n, nets in ((0, 1), (17, 2), (1, 0), (1, 3)):
        assert lib.bsx_adam_step_workspace_bytes(n, nets, ctypes.byref(nb)) == ARG
    assert lib.bsx_adam_step_workspace_bytes(1, 1, None) == ARG


NET_PTRS, IO_PTRS, LS = ("grad", "m", "v", "blob"), ("hyper", "step"), ("log_std", "g_log_std", "m_ls", "v_ls")


def _io(nets=2, na=(4, 1), net1=None, p=None, **kw):
    L = _L()
    st = L.BsxAdamIo()
    st.nets = nets
    for i in range(2):
        for q in range(10):
            st.net[i].p[q] = A16
        for f in NET_PTRS:
            setattr(st.net[i], f, A16)
        st.net[i].n_actions = na[i]
    for f in IO_PTRS:
        setattr(st, f, kw.get(f, A16))
    for f in LS:
        setattr(st, f, kw.get(f))
    for f, x in kw.items():
        if f in NET_PTRS:
            setattr(st.net[0], f, x)
    for f, x in (net1 or {}).items():
        setattr(st.net[1], f, x)
    for q, x in (p or {}).items():
        st.net[0].p[q] = x
    return st


def _targets(spec):
    """spec: per network None (no target), or a dict {q or "blob": address} over a whole target at A16."""
    L = _L()
    tg = L.BsxAdamTargets()
    for i, over in enumerate(spec):
        if over is None:
            continue
        for q in range(10):
            tg.net[i].p[q] = over.get(q, A16)
        tg.net[i].blob = over.get("blob", A16)
    return tg


def _mlp(A=4, D=24, group=1, ws=A16, stats=A16, io=True, targets=None, **kw):
    lib = _L().load()
    st = _io(**kw)
    tg = _targets(targets) if targets is not None else None
    return lib.bsx_adam_step_mlp(ctypes.byref(st) if io else None, A, D, group, ctypes.byref(tg) if tg is not None else None, ws, stats, None)


def test_the_free_width_entry_refuses_what_the_header_documents_before_any_launch():
    """Fake addresses only: every call here is refused before anything reaches HIP, argument rules before alignment rules."""
    all_ls = {f: A16 for f in LS}
    whole = [{}, {}]
    arg = [dict(io=False), dict(ws=None), dict(stats=None), dict(hyper=None), dict(step=None),
           dict(A=0), dict(A=33), dict(A=-2), dict(D=0), dict(D=65), dict(D=-1), dict(nets=0), dict(nets=3),
           dict(group=0), dict(group=-1), dict(group=3), dict(group=8), dict(A=6, group=4), dict(A=3, group=2), dict(A=5, group=10),
           dict(na=(2, 1)), dict(na=(0, 1)), dict(na=(4, 5)), dict(p={0: None}), dict(p={9: None})]
    arg += [{f: None} for f in NET_PTRS] + [dict(net1={f: None}) for f in NET_PTRS]
    arg += [{f: A16} for f in LS] + [{g: A16 for g in LS if g != f} for f in LS]
    # a partly filled target, of either network: a parameter or the blob missing, or one pointer alone
    arg += [dict(targets=[{q: None}, None]) for q in (0, 4, 9)] + [dict(targets=[{"blob": None}, {}]), dict(targets=[{}, {7: None}])]
    arg += [dict(targets=[None, dict({q: None for q in range(10)})]), dict(targets=[dict({q: None for q in range(1, 10)}, blob=None), None])]
    for kw in arg:
        assert _mlp(**kw) == ARG, kw
    align = [{f: A4} for f in NET_PTRS] + [{f: A8} for f in NET_PTRS] + [dict(net1={f: A4}) for f in NET_PTRS]
    align += [dict(p={0: A1}), dict(p={9: A1}), dict(hyper=A1), dict(step=A4), dict(ws=A4), dict(stats=A4)]
    align += [dict(all_ls, **{f: A1}) for f in LS]
    align += [dict(targets=[{"blob": A4}, None]), dict(targets=[{"blob": A8}, {}]), dict(targets=[None, {"blob": A4}]),
              dict(targets=[{0: A1}, {}]), dict(targets=[{}, {9: A1}])]
    for kw in align:
        assert _mlp(**kw) == ALIGN, kw
    # what is not read is not judged: the second network and its target in a single-net call; target parameters need four bytes only;
    # every (A, D, group) of the contract's edges passes the argument rules (the misaligned grad is what refuses these)
    for kw in (dict(nets=1, net1=dict(grad=None)), dict(nets=1, targets=[{}, {3: None}]), dict(nets=1, targets=[None, {"blob": A1}]),
               dict(targets=[{8: A4}, None]), dict(targets=[None, None]), dict(targets=whole),
               dict(A=1, D=1), dict(A=32, D=64), dict(A=3, D=9, group=3), dict(A=6, group=2), dict(A=6, group=3), dict(A=32, group=32), dict(A=5, D=51, group=5)):
        assert _mlp(grad=A4, **kw) == ALIGN, kw
    # the order: argument rules before alignment rules, a partly filled target among them
    for kw in (dict(grad=A4, A=0), dict(ws=A4, D=65), dict(stats=A4, group=3), dict(blob=A4, targets=[{2: None}, None]),
               dict(targets=[{"blob": A4}, {"blob": None}]), dict(step=A4, log_std=A16), dict(targets=[{"blob": A4}, None], D=0)):
        assert _mlp(**kw) == ARG, kw


def test_the_two_older_entries_still_refuse_what_they_refused():
    lib = _L().load()

    def step(n=2, ws=A16, stats=A16, io=True, **kw):
        st = _io(**kw)
        return lib.bsx_adam_step(ctypes.byref(st) if io else None, n, ws, stats, None)

    def shared(n=2, group=1, ws=A16, stats=A16, io=True, **kw):
        st = _io(**kw)
        return lib.bsx_adam_step_shared(ctypes.byref(st) if io else None, n, group, ws, stats, None)
    for kw in (dict(io=False), dict(ws=None), dict(stats=None), dict(hyper=None), dict(step=None), dict(n=0), dict(n=17), dict(nets=3),
               dict(na=(2, 1)), dict(p={9: None}), dict(grad=None), dict(log_std=A16), dict(grad=A4, n=0), dict(blob=A4, na=(4, 2))):
        assert step(**kw) == ARG and shared(**kw) == ARG, kw
    for kw in (dict(grad=A4), dict(blob=A8), dict(p={0: A1}), dict(step=A4), dict(ws=A4), dict(stats=A4), dict(hyper=A1)):
        assert step(**kw) == ALIGN and shared(**kw) == ALIGN, kw
    # the tied entry's own group rule: 1, a divisor of n that is >= 2, or 2n -- narrower than the free-width entry's "divides A"
    for n, group in ((2, 0), (2, -1), (2, 3), (3, 2), (4, 8 + 1), (6, 4), (3, 12)):
        assert shared(n=n, group=group) == ARG and shared(n=n, group=group, grad=A4) == ARG, (n, group)
    for n, group in ((2, 1), (2, 2), (2, 4), (6, 3), (6, 12), (3, 6), (16, 32)):
        assert shared(n=n, group=group, grad=A4) == ALIGN, (n, group)
    assert shared(n=3, group=2, grad=A4) == ARG and _mlp(A=6, D=11, group=2, grad=A4) == ALIGN       # 2 divides A = 6 but not n = 3


def test_the_polyak_line_of_the_restatement_is_torch_lerp_in_float64():
    """Three steps over a 3-agent network and a log_std without a target: parameters, moments and the norm against torch's float64
    clip_grad_norm_ + Adam as in test_adam_step_cpu.py, the targets against both torch.lerp(t, p, tau) and t.mul(1 - tau).add(p, alpha=tau)
    in float64 (1e-12 relative: the two torch forms differ from each other by that much)."""
    gen = torch.Generator().manual_seed(5)
    A, D, na, tau = 3, 9, 1, MU.TAU
    shapes = [(A, D, 64)] + [(A, 1, 64)] * 3 + [(A, 64, 64)] + [(A, 1, 64)] * 3 + [(A, 64, na), (A, 1, na), (A, 3)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64) * 0.1) for s in shapes]
    t_lerp = [torch.randn(s, generator=gen, dtype=torch.float64) * 0.1 for s in shapes[:-1]] + [None]
    t_mad = [None if x is None else x.clone() for x in t_lerp]
    hp = U.hyper32(lr=0.01, max_grad_norm=20.0)
    opt = torch.optim.Adam(params, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    P = [p.detach().numpy().copy() for p in params]
    M, V, t = [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P], 0
    T = [None if x is None else x.numpy().copy() for x in t_lerp]
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())     # noqa: E731
    for step in range(3):
        row = U.random_rows(A, D, na, gen).double().numpy()
        grads = U.row_to_tensors(row, na) + [torch.randn((A, 3), generator=gen, dtype=torch.float64).numpy()]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        norm_t = float(torch.nn.utils.clip_grad_norm_(params, hp["max_grad_norm"]))
        opt.step()
        with torch.no_grad():
            for i, p in enumerate(params):
                if t_lerp[i] is not None:
                    t_lerp[i] = torch.lerp(t_lerp[i], p.detach(), tau)
                    t_mad[i].mul_(1.0 - tau).add_(p.detach(), alpha=tau)
        P, M, V, T, t, norm, coef = MU.reference_step(P, grads, M, V, T, t, hp, tau)
        assert abs(norm - norm_t) <= 1e-12 * norm_t and coef < 1.0 and t == step + 1
        for i, p in enumerate(params):
            assert rel(P[i], p.detach().numpy()) <= 1e-12 and rel(M[i], opt.state[p]["exp_avg"].numpy()) <= 1e-12, (step, i)
            if T[i] is None:
                assert t_lerp[i] is None
                continue
            assert rel(T[i], t_lerp[i].numpy()) <= 1e-12 and rel(T[i], t_mad[i].numpy()) <= 1e-12, (step, i)
    assert T[-1] is None                                                        # log_std has no target
    # the edges of the rule: tau = 1 is the parameter, tau = 0 the target, exactly
    assert all(np.array_equal(a, b) for a, b in zip(MU.polyak(T[:-1], P[:-1], 1.0), P[:-1]))
    assert all(np.array_equal(a, b) for a, b in zip(MU.polyak(T[:-1], P[:-1], 0.0), T[:-1]))


def test_the_binding_names_the_argument_it_refuses():
    """mlp_adam_step's own checks that need no device: what adam_step refuses by name, the targets' pairing, shapes and kinds, and tau."""
    from deep_rl_battlespace_amd import learner
    from deep_rl_battlespace_amd.rollout import StackedActor
    net, tgt = StackedActor(3, 9, 1), StackedActor(3, 9, 1)
    st = learner.AdamState(net)
    assert all(StackedActor(1, D, 1).pack().shape == (1, MU.blob_floats(D)) for D in (1, 9, 50, 51, 64))
    row, blob, tblob = torch.zeros_like(st.m), torch.zeros(3, MU.blob_floats(9)), torch.zeros(3, MU.blob_floats(9))
    hyper, step = learner.adam_hyper(device="cpu", tau=0.005), torch.zeros(1, dtype=torch.int64)
    assert hyper.tolist()[5] == float(np.float32(0.005)) and hyper.tolist()[6:] == [0.0, 0.0]
    assert torch.equal(learner.adam_hyper(device="cpu"), torch.tensor([3e-4, 0.9, 0.999, 1e-8, 0, 0, 0, 0], dtype=torch.float32))   # the default: as it was
    assert learner.adam_hyper(device="cpu", tau=1).tolist()[5] == 1.0 and learner.adam_hyper(device="cpu", tau=0).tolist()[5] == 0.0
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="tau"):
            learner.adam_hyper(device="cpu", tau=bad)

    def call(nets=(net,), rows=(row,), states=(st,), blobs=(blob,), **kw):
        return learner.mlp_adam_step(list(nets), list(rows), list(states), list(blobs), hyper, step, **kw)
    with pytest.raises(TypeError, match="nets"):
        learner.mlp_adam_step(net, [row], [st], [blob], hyper, step)
    with pytest.raises(ValueError, match="one or two networks"):
        call(nets=(net, net))
    with pytest.raises(TypeError, match=r"nets\[0\]"):
        call(nets=(row,))
    with pytest.raises(ValueError, match="targets and target_blobs go together"):
        call(targets=[tgt])
    with pytest.raises(ValueError, match="targets and target_blobs go together"):
        call(target_blobs=[tblob])
    with pytest.raises(TypeError, match="targets must be a list"):
        call(targets=tgt, target_blobs=[tblob])
    with pytest.raises(ValueError, match="target_blobs must have one entry"):
        call(targets=[tgt], target_blobs=[tblob, tblob])
    with pytest.raises(ValueError, match=r"targets\[0\] and target_blobs\[0\] go together"):
        call(targets=[tgt], target_blobs=[None])
    with pytest.raises(ValueError, match=r"targets\[0\] and target_blobs\[0\] go together"):
        call(targets=[None], target_blobs=[tblob])
    with pytest.raises(TypeError, match=r"targets\[0\] must be a StackedActor"):
        call(targets=[row], target_blobs=[tblob])
    with pytest.raises(ValueError, match=r"targets\[0\] is nets\[0\] itself"):
        call(targets=[net], target_blobs=[tblob])
    for other in (StackedActor(3, 9, 3), StackedActor(3, 8, 1), StackedActor(4, 9, 1)):     # another n_actions, obs_len, agent count
        with pytest.raises(ValueError, match=r"targets\[0\] must have the \(agents, obs_len, n_actions\) = \(3, 9, 1\)"):
            call(targets=[other], target_blobs=[tblob])
    with pytest.raises(ValueError, match=r"target_blobs\[0\] must have shape"):
        call(targets=[tgt], target_blobs=[tblob[:, 1:]])
    with pytest.raises(TypeError, match=r"target_blobs\[0\] must be a torch.Tensor"):
        call(targets=[tgt], target_blobs=[[0.0]])
    # everything about the targets holds: the call gets as far as adam_step's does without a GPU, under its own name
    with pytest.raises(ValueError, match="mlp_adam_step runs on the GPU"):
        call(targets=[tgt], target_blobs=[tblob])
    with pytest.raises(ValueError, match="adam_step runs on the GPU"):
        learner.adam_step([StackedActor(2, 5, 4)], [row], [st], [blob], hyper, step)
