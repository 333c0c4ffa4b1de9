"""The fused optimiser step without a GPU: the float64 restatement the GPU tests measure against (tests/adam_util.py) is pinned to
torch's own clip_grad_norm_ + Adam in float64, the row layout and the pad mask to learner.split_grad, the integer restatement of the blob's
bfloat16 split to CPU StackedActor.pack() at weights that force every rounding case, and the C entry points' refusals are host-only."""
import ctypes

import numpy as np
import pytest
import torch

import adam_util as U


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_the_float64_restatement_is_torch_clip_grad_norm_and_adam_in_float64():
    """Five steps over the ten tensors of a 2-agent network and a log_std, fresh gradients each; the gradients of steps 2 and 4 are a
    tenth of the others, so that max_grad_norm bites on steps 1, 3, 5 and not on 2, 4."""
    gen = torch.Generator().manual_seed(3)
    A, D, na = 2, 5, 3
    shapes = [(A, D, 64)] + [(A, 1, 64)] * 3 + [(A, 64, 64)] + [(A, 1, 64)] * 3 + [(A, 64, na), (A, 1, na), (A, 3)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64) * 0.1) for s in shapes]
    hp = U.hyper32(lr=3e-4, max_grad_norm=20.0)
    opt = torch.optim.Adam(params, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    P = [p.detach().numpy().copy() for p in params]
    M, V, t = [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P], 0
    coefs = []
    for step in range(5):
        scale = 0.1 if step in (1, 3) else 1.0
        row = U.random_rows(A, D, na, gen, scale).double().numpy()
        grads = U.row_to_tensors(row, na) + [scale * torch.randn((A, 3), generator=gen, dtype=torch.float64).numpy()]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        norm_t = float(torch.nn.utils.clip_grad_norm_(params, hp["max_grad_norm"]))
        opt.step()
        P, M, V, t, norm, coef = U.reference_step(P, grads, M, V, t, hp)
        coefs.append(coef)
        assert abs(norm - norm_t) <= 1e-12 * norm_t
        for i, p in enumerate(params):
            st = opt.state[p]
            assert _rel(P[i], p.detach().numpy()) <= 1e-12, (step, i)
            assert _rel(M[i], st["exp_avg"].numpy()) <= 1e-12 and _rel(V[i], st["exp_avg_sq"].numpy()) <= 1e-12, (step, i)
        assert t == step + 1 == int(opt.state[params[0]]["step"])
    assert [c < 1.0 for c in coefs] == [True, False, True, False, True], coefs
    # max_grad_norm = 0 is "no clipping": the coefficient is exactly 1
    assert U.reference_step(P, grads, M, V, t, U.hyper32())[5] == 1.0


def test_the_row_layout_matches_split_grad_and_round_trips():
    from deep_rl_battlespace_amd import learner
    gen = torch.Generator().manual_seed(5)
    for A, D, na in ((2, 5, 4), (6, 11, 3), (4, 8, 1)):
        assert U.grad_floats(D) == learner.grad_floats(D)
        row = U.random_rows(A, D, na, gen)
        mine, theirs = U.row_to_tensors(row, na), learner.split_grad(row, na)
        assert all(torch.equal(a, b) for a, b in zip(mine, theirs))
        back = U.tensors_to_row([t.numpy() for t in mine])
        assert np.array_equal(back, row.double().numpy())                      # the pad columns were +0 and come back as 0
        tail = row[:, -(64 * 4 + 4):].view(A, 65, 4)
        assert bool((tail[:, :, na:] == 0).all()) and bool((tail[:, :, :na] != 0).all())
        assert learner.blob_floats(D) == 64 * (D + D % 2) + 10884


def test_the_pad_mask_marks_exactly_the_row_elements_no_parameter_stands_behind():
    """Against row_to_tensors (itself pinned to learner.split_grad above): the elements of a row that reach one of the ten tensors are
    the unmasked ones, in order; random_rows holds +0 exactly where the mask is set."""
    gen = torch.Generator().manual_seed(7)
    for A, D, na in ((2, 5, 4), (6, 11, 3), (4, 8, 1)):
        G = U.grad_floats(D)
        mask = U.pad_mask(D, na)
        assert mask.shape == (G,) and mask.dtype == np.bool_ and int(mask.sum()) == 65 * (4 - na)
        assert not mask[:G - 260].any()
        assert np.array_equal(mask[G - 260:].reshape(65, 4), np.broadcast_to(np.arange(4) >= na, (65, 4)))
        row = np.arange(A * G, dtype=np.float64).reshape(A, G)
        kept = np.concatenate([t.reshape(A, -1) for t in U.row_to_tensors(row, na)], axis=1)
        assert np.array_equal(kept, row[:, ~mask])
        rnd = U.random_rows(A, D, na, gen).numpy()
        assert np.array_equal(rnd == 0, np.broadcast_to(mask, (A, G))) and not np.signbit(rnd[:, mask]).any()


def test_the_integer_restatement_of_the_bf16_split_is_pack_where_rounding_is_decided():
    """w2 = adam_util.w2_edge_weights: ties, one bit either side of them, carries into the exponent, +-0, exponents -60 .. 60.  The W2B
    part of CPU StackedActor.pack() equals adam_util.w2b_words on every element, for a 4-column and a 1-column network, and the three terms sum to
    the weight exactly (3 x 8 significant bits cover float32's 24).  Non-finite weights are a diverged run and are not covered."""
    from deep_rl_battlespace_amd.rollout import StackedActor
    A, D = 4, 8
    w2 = U.w2_edge_weights(A, seed=11)
    bits = w2.view(np.uint32)
    # the set is what it says: every crafted pattern in every agent, both zeros, exponents inside +-60, nothing non-finite
    for a in range(A):
        have = set(bits[a].ravel().tolist())
        assert {0x00000000, 0x80000000} <= have
        for e in U.W2_EDGE_EXPONENTS:
            for up in U.W2_EDGE_UPPER:
                for lo in U.W2_EDGE_LOW:
                    assert {((e + 127) << 23) | (up << 16) | lo, (1 << 31) | ((e + 127) << 23) | (up << 16) | lo} <= have
    expo = ((bits >> 23) & 0xff).astype(np.int64) - 127
    nz = (bits & 0x7fffffff) != 0
    assert expo[nz].min() == -60 and expo[nz].max() == 60 and int((~nz).sum()) == 2 * A
    assert not np.array_equal(bits[0], bits[1])                                 # shuffled per agent
    # the rounding rule on a few patterns by hand: below a tie, ties to even, above a tie, the carry into the exponent, -0
    hand = np.array([0x3f807fff, 0x3f808000, 0x3f818000, 0x3f808001, 0x3fffffff, 0x3fff8000, 0x80000000], dtype=np.uint32)
    assert U.bf16_rne_bits(hand).tolist() == [0x3f80, 0x3f80, 0x3f82, 0x3f81, 0x4000, 0x4000, 0x8000]
    assert np.array_equal(U.bf16_rne_bits(bits), torch.from_numpy(w2.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    h, m, l = U.w2b_split(w2)
    total = sum(U.bf16_bits_to_float(x).astype(np.float64) for x in (h, m, l))
    assert np.array_equal(total, w2.astype(np.float64))
    for x in (h, m, l):                                                           # no term is subnormal or non-finite
        e = (x >> 7) & 0xff
        assert bool(((e != 0xff) & ((e != 0) | ((x & 0x7f) == 0))).all())
    for na in (4, 1):
        net = StackedActor(A, D, na)
        with torch.no_grad():
            net.w2.copy_(torch.from_numpy(w2.copy()))
        blob = net.pack().numpy().view(np.uint32)
        assert blob.shape[1] == 64 * D + 10884 and U.W2B_FLOATS == 6144
        mine = U.w2b_words(w2)
        bad = np.argwhere(blob[:, -U.W2B_FLOATS:] != mine)
        assert bad.size == 0, bad[:4].tolist()


def test_the_c_entry_points_refuse_what_the_header_documents_before_any_launch():
    """Fake addresses only: every call is refused before anything reaches HIP, argument rules before alignment rules."""
    from deep_rl_battlespace_amd import _lib as L
    lib = L.load()
    A16, A8, A4, A1 = 4096, 4096 + 8, 4096 + 4, 4096 + 1
    ARG, ALIGN = -1, -2
    net_ptrs, io_ptrs, ls = ("grad", "m", "v", "blob"), ("hyper", "step"), ("log_std", "g_log_std", "m_ls", "v_ls")

    def call(n=2, nets=2, ws=A16, stats=A16, io=True, na=(4, 1), net1=None, p=None, **kw):
        st = L.BsxAdamIo()
        st.nets = nets
        for i in range(2):
            for q in range(10):
                st.net[i].p[q] = A16
            for f in net_ptrs:
                setattr(st.net[i], f, A16)
            st.net[i].n_actions = na[i]
        for f in io_ptrs:
            setattr(st, f, A16)
        for f in ls:
            setattr(st, f, kw.get(f))
        for f, x in kw.items():
            if f in net_ptrs:
                setattr(st.net[0], f, x)
            elif f in io_ptrs:
                setattr(st, f, x)
        for f, x in (net1 or {}).items():
            setattr(st.net[1], f, x)
        for q, x in (p or {}).items():
            st.net[0].p[q] = x
        return lib.bsx_adam_step(ctypes.byref(st) if io else None, n, ws, stats, None)

    all_ls = {f: A16 for f in ls}
    arg = [dict(io=False), dict(ws=None), dict(stats=None), dict(hyper=None), dict(step=None), dict(n=0), dict(n=17), dict(n=-1),
           dict(nets=0), dict(nets=3), dict(na=(2, 1)), dict(na=(0, 1)), dict(na=(4, 5)), dict(p={0: None}), dict(p={9: None})]
    arg += [{f: None} for f in net_ptrs] + [dict(net1={f: None}) for f in net_ptrs]
    arg += [{f: A16} for f in ls] + [{g: A16 for g in ls if g != f} for f in ls]             # some but not all of the log_std four
    for kw in arg:
        assert call(**kw) == ARG, kw
    align = [{f: A4} for f in net_ptrs] + [{f: A8} for f in net_ptrs] + [dict(net1={f: A4}) for f in net_ptrs]
    align += [dict(p={0: A1}), dict(p={9: A1}), dict(hyper=A1), dict(step=A4), dict(ws=A4), dict(stats=A4)]
    align += [dict(all_ls, **{f: A1}) for f in ls]
    for kw in align:
        assert call(**kw) == ALIGN, kw
    # what is not read is not judged: the second network of a single-net call; parameters need four bytes only
    for kw in (dict(nets=1, net1=dict(grad=None, blob=A1)), dict(nets=1, na=(4, 7)), dict(p={8: A4}), all_ls):
        assert call(grad=A4, **kw) == ALIGN, kw
    # the order: argument rules before alignment rules
    for kw in (dict(grad=A4, n=0), dict(ws=A4, nets=3), dict(stats=A4, m=None), dict(blob=A4, na=(4, 2)), dict(step=A4, log_std=A16)):
        assert call(**kw) == ARG, kw
    nb = ctypes.c_size_t()
    for n, nets in ((1, 1), (1, 2), (16, 2)):
        assert lib.bsx_adam_step_workspace_bytes(n, nets, ctypes.byref(nb)) == 0
        assert nb.value % 8 == 0 and 8 * (2 * n * nets + 1) < nb.value <= 8 * (2 * n * nets + 16)
    for n, nets in ((0, 1), (17, 2), (1, 0), (1, 3)):
        assert lib.bsx_adam_step_workspace_bytes(n, nets, ctypes.byref(nb)) == ARG
    assert lib.bsx_adam_step_workspace_bytes(1, 1, None) == ARG


def test_the_binding_names_the_argument_it_refuses():
    """learner.adam_step's own checks that need no device: container types, the network count, tensors off the GPU; AdamState's shapes."""
    from deep_rl_battlespace_amd import learner
    from deep_rl_battlespace_amd.rollout import StackedActor
    net, critic = StackedActor(2, 5, 4), StackedActor(2, 5, 1)
    st = learner.AdamState(net)
    assert st.m.shape == st.v.shape == (2, learner.grad_floats(5)) and st.m.dtype == torch.float32 and not st.m.any() and not st.v.any()
    ls = torch.zeros(2, 3)
    assert learner.AdamState(ls).m.shape == (2, 3)
    row, blob = torch.zeros_like(st.m), torch.zeros(2, learner.blob_floats(5))
    hyper, step = learner.adam_hyper(device="cpu"), torch.zeros(1, dtype=torch.int64)
    assert hyper.dtype == torch.float32 and hyper.tolist()[4:] == [0.0] * 4 and hyper[0] == np.float32(3e-4)
    with pytest.raises(TypeError, match="nets"):
        learner.adam_step(net, [row], [st], [blob], hyper, step)
    with pytest.raises(ValueError, match="one or two networks"):
        learner.adam_step([net, critic], [row], [st], [blob], hyper, step)
    with pytest.raises(ValueError, match="one or two networks"):
        learner.adam_step([], [], [], [], hyper, step)
    with pytest.raises(TypeError, match=r"nets\[0\]"):
        learner.adam_step([row], [row], [st], [blob], hyper, step)
    with pytest.raises(ValueError, match="GPU"):
        learner.adam_step([net], [row], [st], [blob], hyper, step)
    for kw, name in ((dict(lr=-1.0), "lr"), (dict(betas=(0.9, 1.0)), r"betas\[1\]"), (dict(betas=0.9), "betas"), (dict(eps=float("nan")), "eps"),
                     (dict(max_grad_norm=-1.0), "max_grad_norm")):
        with pytest.raises(ValueError, match=name):
            learner.adam_hyper(device="cpu", **kw)
