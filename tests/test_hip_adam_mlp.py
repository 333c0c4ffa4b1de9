"""The free-width optimiser step with Polyak targets on the GPU (learner.mlp_adam_step, csrc/bsx_adam_step.hip: bsx_adam_step_mlp).

Shapes (tests/adam_mlp_util.py SHAPES): (1, 1, 1) the smallest, an odd D with W1A's pad row; (3, 9, 1) an odd A at the 1v1 critic's width;
(4, 24, 1) the reference's 2v2 critic; (5, 51, 3) the first width beyond the old LDS bound, odd D, pad columns; (2, 64, 4) the widest
row: 8 full strides of 1024 and a ragged ninth; (32, 64, 1) with a second network and log_std: 65 partials, the widest call.

Accuracy: five steps against the float64 restatement with torch's own float32 path as the yardstick, targets included; every blob and
target blob against pack() after every step.  Then the clauses of the contract: the older entries' bits, determinism and guard bytes,
the Polyak edges (tau = 1, tau = 0, a tau changed under a captured call, a network without a target beside one with, the bfloat16 split
of the target's blob), poisoned pad columns, the agent with a zero gradient, tied groups at free width, and one captured DDPG update.

Measured on an MI355X (profiles/adam_step_mlp.json holds every figure): over the 18 (shape, leg) cases the largest mean ratio of the
kernel's error to torch's is 1.05 (parameters), 1.14 (m), 1.05 (v) and 0.90 (targets), the largest maximum ratio 1.21, 1.36, 1.02 and
1.00 -- inside the bars of 2 and 4 everywhere."""
import numpy as np
import pytest
import torch

import adam_case_util as C
import adam_mlp_util as MU
import adam_util as U
import guard_util as GU

pytestmark = pytest.mark.gpu

BARS = dict(env="BSX_ADAM_MLP_RATIOS_OUT", key="shape")        # =<file>: the five-step ratios as JSON lines for tools/measure_adam_mlp.py


def _new(A, D, nas, hp, seed=0, **kw):
    return C.Case(A, D, nas, hp, seed=300 + seed, **kw)


def _case(shape, hp, **kw):
    A, D, na, wide = MU.SHAPES[shape]
    return _new(A, D, (na, 1) if wide else (na,), hp, with_ls=wide, **kw)


def _first_norm(shape, seed):
    """The float64 norm of the first gradients Case.draw gives from a generator seeded with `seed`."""
    A, D, na, wide = MU.SHAPES[shape]
    return C.first_norm(A, D, (na, 1) if wide else (na,), wide, seed)


@pytest.mark.parametrize("leg", list(C.LEGS))
@pytest.mark.parametrize("shape", list(MU.SHAPES))
def test_five_steps_match_the_float64_restatement_as_well_as_torch_does_targets_included(shape, leg):
    """Five steps with fresh gradients each (steps 2 and 4 a tenth of the others: max_grad_norm, half the first step's norm, bites on 1,
    3, 5 only), tau = 0.01, a target on every network.  After EVERY step each blob equals net.pack() and each target blob target.pack()
    bit for bit, and stats holds the exact step, the norm and the clip coefficient within 1e-10 relative of float64 (an N-term float64
    sum of exact squares is off by at most (N - 1) 2^-53, N <= 5.7e5 here) and the float32 lr.  After the five steps, per network and for
    each of parameters, m, v and targets, pooled over the ten tensors: mean |error| against the float64 restatement at most 2x that of
    torch's own float32 clip_grad_norm_ + Adam + target.mul_(1 - tau).add_(p, alpha=tau) on the same inputs, maximum at most 4x."""
    lr, counter = C.LEGS[leg]
    hp = U.hyper32(lr=lr, max_grad_norm=0.5 * _first_norm(shape, 17))
    case = _case(shape, hp)
    yard = C.TorchPath(case, hp, MU.TAU)
    ref = C.start(case)
    t, coefs = 0, []
    gen = torch.Generator().manual_seed(17)
    for s in range(C.STEPS):
        if s in counter:
            t = counter[s]
            case.step.fill_(t)
            yard.set_counter(t)
        rows, g_ls = case.draw(gen, 0.1 if s in (1, 3) else 1.0)
        grads = C.flat_split(case, rows, g_ls)
        stats = case.run(rows, g_ls)
        yard.step(grads)
        t, norm, coef = C.advance(ref, grads, t, hp, MU.TAU)
        coefs.append(coef)
        C.blobs_are_packs(case, (shape, leg, s))
        C.check_stats(case, stats, t, norm, coef, hp)
    assert [c < 1.0 for c in coefs] == [True, False, True, False, True], coefs
    C.meets_the_bars(case, yard, ref, shape, leg, **BARS)


@pytest.mark.parametrize("tied", [False, True], ids=["group1", "group2n"])
@pytest.mark.parametrize("n", [1, 3])
def test_at_an_actors_shape_and_without_targets_the_call_leaves_the_older_entries_bits(n, tied):
    """(A, D) = (2n, 3n + 2), a 4-column policy network, a value network and log_std, group = 1 and the tied group = 2n: two clipped
    steps through learner.adam_step(group=) and through mlp_adam_step(group=) from copies of one state leave every output bit equal."""
    from deep_rl_battlespace_amd import learner
    A, D, group = 2 * n, 3 * n + 2, 2 * n if tied else 1
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    old, new = (_new(A, D, (4, 1), hp, with_ls=True, targets=(False, False), seed=5, group=group) for _ in range(2))
    if tied:
        old.tie()
        new.load(old)
    assert C.same_bits(old.bits(), new.bits()) == []
    gen = torch.Generator().manual_seed(61)
    for s in range(2):
        rows, g_ls = old.draw(gen)
        learner.adam_step(old.nets, rows, old.states, old.blobs, old.hyper, old.step, log_std=old.log_std, g_log_std=g_ls,
                          log_std_state=old.ls_state, stats=old.stats, workspace=old.ws, group=group)
        new.run([r.clone() for r in rows], g_ls.clone())
        a, b = old.bits(), new.bits()
        assert sorted(a) == sorted(b) and C.same_bits(a, b) == [], (s, C.same_bits(a, b))
        assert int(new.step) == s + 1 and float(new.stats[2]) < 1.0
        if tied:
            assert all(learner.is_tied(x, group) for x in new.nets + new.states + [new.log_std, new.ls_state])
    C.blobs_are_packs(new, (n, tied))


@pytest.mark.parametrize("shape", ["a3-d9", "a5-d51-na3", "a2-d64-na4", "a32-d64-two-nets-log-std"])
def test_two_calls_from_copies_of_one_state_give_identical_bits_and_leave_the_guards_alone(shape):
    hp = U.hyper32(lr=0.01, max_grad_norm=5.0)
    alloc = GU.Buffers(True)
    a, b = _case(shape, hp, alloc=alloc), _case(shape, hp)
    gen = torch.Generator().manual_seed(29)
    for _ in range(2):
        rows, g_ls = a.draw(gen)
        a.run(rows, g_ls)
        b.run([r.clone() for r in rows], g_ls.clone() if g_ls is not None else None)
    x, y = a.bits(), b.bits()
    assert sorted(x) == sorted(y) and C.same_bits(x, y) == []
    assert any(k.startswith("target") for k in x) and int(a.step) == 2 and float(a.stats[2]) < 1.0
    assert alloc.stray() == []
    C.blobs_are_packs(a, shape)


@pytest.mark.parametrize("shape", ["a3-d9", "a5-d51-na3"])
def test_tau_one_makes_the_target_the_network_and_tau_zero_keeps_it_and_still_writes_its_blob(shape):
    """Random weights (StackedActor's initialisation holds no -0).  tau = 1: every target parameter equals the new parameter and the
    target's blob the network's, bit for bit.  tau = 0: the target parameters keep their bits and the target blob, pre-filled with a
    non-zero pattern, is pack() of them.  The network's own outputs do not depend on tau."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    one, zero = _case(shape, hp, tau=1.0), _case(shape, hp, tau=0.0)
    before = zero.bits()
    assert bool((zero.target_blobs[0] == -3.5).all())
    rows, g_ls = one.draw(torch.Generator().manual_seed(67))
    one.run(rows, g_ls)
    zero.run([r.clone() for r in rows], g_ls)
    x, y = one.bits(), zero.bits()
    for k in U.PARAMS:
        assert torch.equal(x[f"target0.{k}"], x[f"net0.{k}"]), k
        assert torch.equal(y[f"target0.{k}"], before[f"target0.{k}"]) and not torch.equal(y[f"net0.{k}"], before[f"net0.{k}"]), k
    assert torch.equal(x["target0.blob"], x["net0.blob"])
    assert not torch.equal(y["target0.blob"], before["target0.blob"])
    own = lambda bits: {k: v for k, v in bits.items() if k.startswith(("net", "st"))}     # noqa: E731
    assert C.same_bits(own(x), own(y)) == []
    C.blobs_are_packs(one, (shape, "tau 1"))
    C.blobs_are_packs(zero, (shape, "tau 0"))


def test_a_tau_changed_in_hyper_between_two_replays_of_a_captured_call_is_followed():
    """tau is read on the device at every launch: one captured call replayed at tau = 0.25 and then at tau = 1 leaves the bits of two
    eager calls with those rates from a copy of the state -- and after the second the target is the network."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    cap, eager = _case("a3-d9", hp, tau=0.25, seed=7), _case("a3-d9", hp, tau=0.25, seed=7)
    rows, g_ls = cap.draw(torch.Generator().manual_seed(71))
    kept = [r.clone() for r in rows]
    start = cap.bits()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # one call ahead of the capture, then the state as it was
        cap.run(rows, g_ls)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k, v in cap.tensors().items():
        v.view(start[k].dtype).copy_(start[k])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.run(rows, g_ls)
    for tau in (0.25, 1.0):
        cap.hyper[5] = tau
        eager.hyper[5] = tau
        graph.replay()
        eager.run(kept, g_ls)
        assert C.same_bits(cap.bits(), eager.bits()) == [], tau
    x = cap.bits()
    assert int(cap.step) == 2 and all(torch.equal(x[f"target0.{k}"], x[f"net0.{k}"]) for k in U.PARAMS)
    assert torch.equal(x["target0.blob"], x["net0.blob"])
    C.blobs_are_packs(cap, "captured")


def test_a_network_without_a_target_beside_one_with_is_stepped_as_in_the_call_without_targets():
    """targets = [None, a target]: everything of the first network, of log_std and stats hold the bits of the same call without any
    target (so do the second network's own outputs), and the second network's target and its blob are kept up."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    mixed = _new(4, 24, (3, 1), hp, with_ls=True, targets=(False, True), seed=9)
    plain = _new(4, 24, (3, 1), hp, with_ls=True, targets=(False, False), seed=9)
    plain.load(mixed)
    gen = torch.Generator().manual_seed(73)
    before = mixed.bits()
    for _ in range(2):
        rows, g_ls = mixed.draw(gen)
        mixed.run(rows, g_ls)
        plain.run([r.clone() for r in rows], g_ls.clone())
    x, y = mixed.bits(), plain.bits()
    assert sorted(k for k in x if k not in y) == sorted([f"target1.{k}" for k in U.PARAMS] + ["target1.blob"])
    assert C.same_bits(y, x, common=True) == [] and float(mixed.stats[2]) < 1.0
    assert all(not torch.equal(x[f"target1.{k}"], before[f"target1.{k}"]) for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    C.blobs_are_packs(mixed, "mixed")


def test_the_bf16_split_of_the_target_blob_is_pack_where_rounding_is_decided():
    """The target's w2 = adam_util.w2_edge_weights (ties, one bit either side of a tie, carries into the exponent, +-0, exponents
    -60 .. 60), tau = 0, one clipped step with real gradients: the target's parameters come back equal in value with every bit of every
    non-zero element kept (a -0 is added to a zero and may come back +0: the header says so), every W2B word of the target's blob
    equals the integer restatement adam_util.w2b_words of the target's w2, and the whole blob is pack()."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    case = _new(2, 8, (4, 1), hp, tau=0.0, seed=11)
    w2s = [U.w2_edge_weights(case.A, seed=79 + i) for i in range(2)]
    with torch.no_grad():
        for tgt, w2 in zip(case.targets, w2s):
            tgt.w2.copy_(torch.from_numpy(w2.copy()))
    rows, g_ls = case.draw(torch.Generator().manual_seed(83))
    case.run(rows, g_ls)
    after = case.bits()
    for i, w2 in enumerate(w2s):
        got = after[f"target{i}.w2"].cpu().numpy().view(np.uint32)
        want = w2.view(np.uint32)
        nonzero = (want & 0x7fffffff) != 0
        assert np.array_equal(got[nonzero], want[nonzero]) and not (got[~nonzero] & 0x7fffffff).any() and int((~nonzero).sum()) == 2 * case.A
        words = after[f"target{i}.blob"].cpu().numpy().view(np.uint32)[:, -U.W2B_FLOATS:]
        bad = np.argwhere(words != U.w2b_words(got.view(np.float32)))
        assert bad.size == 0, ("restatement", i, bad[:4].tolist())
    C.blobs_are_packs(case, "bf16 edges")


@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("shape", ["a3-d9", "a5-d51-na3"])
def test_poisoned_pad_columns_are_neither_read_nor_written(shape, poison):
    """n_actions 1 and 3: twins from one seed, B with every pad element of its gradient rows at NaN (or 1e30) and of its moments at 7.25.
    After each of two clipped steps every tensor of B equals A's bit for bit outside the moments' pads -- stats, targets and target
    blobs among them --, B's pads still hold 7.25, A's +0, and every blob is pack() (whose pad columns are +0)."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    a, b = _case(shape, hp, seed=3), _case(shape, hp, seed=3)
    masks = [torch.from_numpy(U.pad_mask(a.D, net.n_actions)).cuda() for net in a.nets]
    assert all(int(m.sum()) for m in masks)
    sentinel = torch.tensor(7.25).view(torch.int32).item()
    for st, mask in zip(b.states, masks):
        st.m[:, mask] = 7.25
        st.v[:, mask] = 7.25
    moments = {f"net{i}.{x}": mask for i, mask in enumerate(masks) for x in "mv"}
    gen = torch.Generator().manual_seed(43)
    for s in range(2):
        rows, g_ls = a.draw(gen)
        poisoned = [r.clone() for r in rows]
        for r, mask in zip(poisoned, masks):
            assert bool((r[:, mask] == 0).all())
            r[:, mask] = poison
        a.run(rows, g_ls)
        b.run(poisoned, g_ls)
        x, y = a.bits(), b.bits()
        assert float(a.stats[2]) < 1.0 and int(a.step) == s + 1
        for k in x:
            if k in moments:
                mask = moments[k]
                assert torch.equal(x[k][:, ~mask], y[k][:, ~mask]), (s, k)
                assert bool((y[k][:, mask] == sentinel).all()) and bool((x[k][:, mask] == 0).all()), (s, k)
            else:
                assert torch.equal(x[k], y[k]), (s, k)
        C.blobs_are_packs(a, (shape, s, "a"))
        C.blobs_are_packs(b, (shape, s, "b"))


@pytest.mark.parametrize("max_grad_norm", [0.0, 1.0])
def test_an_agent_with_a_zero_gradient_and_zero_moments_keeps_every_bit_and_its_target_still_moves(max_grad_norm):
    """Gradient rows of +0 and moments of +0 for agents 1 and 3 of five: their parameters, moments and blob rows stay as they are, with
    clipping on and off, the other agents move -- and the frozen agents' targets still move toward their parameters (tau = 0.5)."""
    case = _case("a5-d51-na3", U.hyper32(lr=0.01, max_grad_norm=max_grad_norm), tau=0.5)
    for net, blob in zip(case.nets, case.blobs):
        blob.copy_(net.pack())
    frozen, others = [1, 3], [0, 2, 4]
    before = case.bits()
    rows, g_ls = case.draw(torch.Generator().manual_seed(31))
    for r in rows:
        r[frozen] = 0.0
    case.run(rows, g_ls)
    after = case.bits()
    assert (float(case.stats[2]) < 1.0) == (max_grad_norm > 0.0)
    for k in before:
        if k in ("step", "stats"):
            continue
        assert not torch.equal(before[k][others], after[k][others]), k
        if k.startswith("net"):
            assert torch.equal(before[k][frozen], after[k][frozen]), k
        elif k.split(".")[1] in ("g1", "h1", "g2", "h2"):            # a gain of 1 and a bias of 0 in network and target alike: the blend is exact
            assert torch.equal(before[k][frozen], after[k][frozen]), k
        else:
            assert not torch.equal(before[k][frozen], after[k][frozen]), k
    half = MU.polyak([before["target0.w2"].view(torch.float32).cpu().numpy()], [before["net0.w2"].view(torch.float32).cpu().numpy()], 0.5)[0]
    got = after["target0.w2"].view(torch.float32).cpu().numpy()
    assert float(np.abs(got[frozen] - half[frozen]).max()) <= 2.0 ** -24 * float(np.abs(half[frozen]).max())
    C.blobs_are_packs(case, max_grad_norm)


@pytest.mark.parametrize("A,D,group", [(3, 9, 3), (6, 24, 2)])
def test_the_tied_call_at_free_width_is_the_untied_call_on_the_groups_sums(A, D, group):
    """The header's statement of the tied step, at an odd A tied as one group and at groups of two out of six: two clipped steps of the
    tied call equal the untied call, from the same state, on rows that hold the group's float32 sum (in agent order) at each leader and
    +0 at the followers -- the leaders' parameters, moments, blob rows, targets and target blob rows, and stats, bit for bit -- and
    what was tied before is tied after, targets and every blob row included (compared member by member here: learner.is_tied speaks of
    share_group's groups of an even A, which neither of these is; the test of the older entries' bits asks it at group = 2n)."""
    from deep_rl_battlespace_amd import learner
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    tied = _new(A, D, (1,), hp, tau=0.25, seed=13, group=group)
    tied.tie()
    untied = _new(A, D, (1,), hp, tau=0.25, seed=13, group=1)
    untied.load(tied)
    leaders = list(range(0, A, group))
    gen = torch.Generator().manual_seed(89)
    for s in range(2):
        rows, _ = tied.draw(gen)
        sums = []
        for r in rows:
            v = r.view(A // group, group, -1)
            acc = v[:, 0].clone()
            for k in range(1, group):
                acc = acc + v[:, k]                                  # float32, in agent order from the leader
            z = torch.zeros_like(v)
            z[:, 0] = acc
            sums.append(z.view(A, -1))
        tied.run(rows, None)
        untied.run(sums, None)
        x, y = tied.bits(), untied.bits()
        assert torch.equal(x["stats"], y["stats"]) and torch.equal(x["step"], y["step"]) and float(tied.stats[2]) < 1.0
        for k in x:
            if k not in ("step", "stats"):
                assert torch.equal(x[k][leaders], y[k][leaders]), (s, k)
        for obj in tied.nets + tied.targets + tied.states:
            assert all(bool((t.detach().view(A // group, group, -1) == t.detach().view(A // group, group, -1)[:, :1]).all())
                       for t in learner._tied_tensors(obj))
        for blob in tied.blobs + tied.target_blobs:
            v = blob.view(A // group, group, -1).view(torch.int32)
            assert bool((v == v[:, :1]).all())
    C.blobs_are_packs(tied, (A, D, group))


def _mlp_forward(blob, x, y4, raw):
    from deep_rl_battlespace_amd import _lib
    R, A, D = x.shape
    _lib.check(_lib.load().bsx_mlp_forward(blob.data_ptr(), x.data_ptr(), y4.data_ptr(), raw.data_ptr() if raw is not None else None, R, A, D,
                                           torch.cuda.current_stream(x.device).cuda_stream), "bsx_mlp_forward")


def test_one_ddpg_update_with_targets_replays_as_one_graph_without_allocating():
    """A 1v1-sized actor (2, 5, 3) and critic (2, 8, 1) on 64 rows: target actor and target critic forwards from the TARGET BLOBS
    (bsx_mlp_forward), the TD target with torch ops on preallocated tensors, mlp_grad on the critic, mlp_adam_step on the critic with its
    target, mlp_grad through the critic for dQ/da and then through the actor, mlp_adam_step on the actor with its target -- captured as
    one torch.cuda.graph.  Three replays leave, bit for bit, the state of three eager runs of the same calls from a copy of the starting
    state; both step counters read 3; torch.cuda.memory_allocated() does not grow across the replays."""
    from deep_rl_battlespace_amd import learner
    R, A, Do, Na, gamma = 64, 2, 5, 3, 0.95
    hp = U.hyper32(lr=1e-3, max_grad_norm=0.5)
    actor, critic = _new(A, Do, (Na,), hp, tau=0.05, seed=17), _new(A, Do + Na, (1,), hp, tau=0.05, seed=19)
    for c in (actor, critic):
        c.blobs[0].copy_(c.nets[0].pack())
        c.target_blobs[0].copy_(c.targets[0].pack())
    gen = torch.Generator().manual_seed(97)
    dev = "cuda"
    obs, nxt = torch.randn((R, A, Do), generator=gen).to(dev), torch.randn((R, A, Do), generator=gen).to(dev)
    act, rew = torch.rand((R, A, Na), generator=gen).mul(2).sub(1).to(dev), torch.randn((R, A), generator=gen).to(dev)
    x_cur, x_next, x_pi = (torch.cat([o, a], dim=2).contiguous() for o, a in ((obs, act), (nxt, torch.zeros_like(act)), (obs, torch.zeros_like(act))))
    y4 = torch.empty((R, A, 4), device=dev)
    q_next, q_cur, td = (torch.empty((R, A), device=dev) for _ in range(3))
    go_q, dqda = torch.empty((R, A, 1), device=dev), torch.empty((R, A, Na), device=dev)
    minus = torch.full((R, A, 1), -1.0 / R, device=dev)

    def update():
        _mlp_forward(actor.target_blobs[0], nxt, y4, None)                                  # 1. a' = target actor(next obs)
        x_next[..., Do:].copy_(y4[..., :Na])
        _mlp_forward(critic.target_blobs[0], x_next, y4, q_next)                            #    Q'(next obs, a')
        torch.add(rew, q_next, alpha=gamma, out=td)                                         # 2. the TD target
        _mlp_forward(critic.blobs[0], x_cur, y4, q_cur)                                     # 3. d/dQ of mean (Q - td)^2, then the critic's row
        torch.sub(q_cur, td, out=go_q[..., 0])
        go_q.mul_(2.0 / R)
        row_c, _ = learner.mlp_grad(critic.nets[0], critic.blobs[0], x_cur, go_q, squash=False, input_grad=False)
        critic.run([row_c], None)                                                           # 4. the critic's step, its target and both blobs
        _mlp_forward(actor.blobs[0], obs, y4, None)                                         # 5. dQ/da at a = actor(obs), through the actor
        x_pi[..., Do:].copy_(y4[..., :Na])
        _, gx = learner.mlp_grad(critic.nets[0], critic.blobs[0], x_pi, minus, squash=False, input_grad=True)
        dqda.copy_(gx[..., Do:])
        row_a, _ = learner.mlp_grad(actor.nets[0], actor.blobs[0], obs, dqda, squash=True, input_grad=False)
        actor.run([row_a], None)                                                            # 6. the actor's step, its target and both blobs

    def state():
        torch.cuda.synchronize()
        out = {f"actor.{k}": v for k, v in actor.bits().items()}
        out.update({f"critic.{k}": v for k, v in critic.bits().items()})
        return out

    def restore(snap):
        for name, c in (("actor", actor), ("critic", critic)):
            for k, v in c.tensors().items():
                v.view(snap[f"{name}.{k}"].dtype).copy_(snap[f"{name}.{k}"])
    start = state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            update()
    torch.cuda.current_stream().wait_stream(side)
    eager = state()
    assert int(actor.step) == 3 == int(critic.step)
    moved = [k for k in start if not torch.equal(start[k], eager[k])]
    assert {"actor.net0.w2", "actor.target0.w2", "actor.target0.blob", "critic.net0.w1", "critic.target0.w1", "critic.target0.blob"} <= set(moved)
    restore(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update()
    captured = state()
    assert [k for k in start if not torch.equal(start[k], captured[k])] == []               # a capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held
    replayed = state()
    assert [k for k in eager if not torch.equal(eager[k], replayed[k])] == []
    assert int(actor.step) == 3 == int(critic.step)
    C.blobs_are_packs(actor, "ddpg actor")
    C.blobs_are_packs(critic, "ddpg critic")
