"""The fused optimiser step on the GPU (learner.adam_step, csrc/bsx_adam_step.hip): the blob it packs against StackedActor.pack() bit for
bit, its arithmetic against the float64 restatement of tests/adam_util.py with torch's own float32 clip_grad_norm_ + Adam as the
yardstick, its statistics, determinism, guard words and the agent whose gradient is zero; then the clauses of the contract one by one:
each partial norm on its own (the 65th among them), poisoned pad columns, the bfloat16 split at weights that force every rounding
case, a counter beyond int32, lr = 0 and the all-zero gradient under clipping.

Shapes, the smallest that reach every layout case: n = 1 (D = 5, odd: W1A has a pad row), n = 2 (D = 8), n = 3 with a 3-column actor and
log_std, n = 16 (A = 32, D = 50), each with a 1-column value network beside the policy network, and one single-network call; n = 16
with log_std (65 partials, the most a call can have: the workspace at its largest, the last partial in its last word); the policy-only
Gaussian step (one network and log_std: the log_std workgroup is block A) at n = 1 and n = 16; a value network alone."""
import numpy as np
import pytest
import torch

import adam_case_util as C
import adam_util as U
import guard_util as GU

pytestmark = pytest.mark.gpu

#        id            n  n_actions log_std value net
CONFIGS = {"n1": (1, 4, False, True), "n2": (2, 4, False, True), "n3-gaussian": (3, 3, True, True), "n16": (16, 4, False, True),
           "n2-single": (2, 4, False, False), "n16-gaussian": (16, 3, True, True), "n1-policy-gaussian": (1, 3, True, False),
           "n16-policy-gaussian": (16, 3, True, False), "n2-value-only": (2, 1, False, False)}
RATIOS = "BSX_ADAM_RATIOS_OUT"        # =<file>: the five-step ratios as JSON lines (how profiles/adam_step.json's accuracy table is made)


def _shape(config):
    n, na, with_ls, with_value = CONFIGS[config]
    return 2 * n, 3 * n + 2, (na, 1) if with_value else (na,), with_ls


def _case(config, hp, seed=0, **kw):
    A, D, nas, with_ls = _shape(config)
    return C.Case(A, D, nas, hp, with_ls=with_ls, seed=100 + seed, entry="adam", **kw)


@pytest.mark.parametrize("leg", list(C.LEGS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_five_steps_match_the_float64_restatement_as_well_as_torch_does_and_every_blob_is_the_pack(config, leg):
    """Five steps with fresh gradients each (steps 2 and 4 a tenth of the others: max_grad_norm, half the first step's norm, bites on
    1, 3, 5 only).  After EVERY step both blobs equal pack() of the parameters bit for bit and stats holds the exact step, the norm and the
    clip coefficient within 1e-10 relative of float64 (an N-term float64 sum of exact squares is off by at most (N - 1) 2^-53, N <=
    5.1e5) and the float32 lr.  After the five steps, per network and for each of parameters, m, v, pooled over the ten tensors: mean
    |error| against the float64 restatement at most 2x that of torch's own float32 clip_grad_norm_ + Adam on the same inputs, maximum at
    most 4x."""
    lr, counter = C.LEGS[leg]
    first = C.first_norm(*_shape(config), seed=17)
    hp = U.hyper32(lr=lr, max_grad_norm=0.5 * first)
    case = _case(config, hp)
    yard = C.TorchPath(case, hp)
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
        t, norm, coef = C.advance(ref, grads, t, hp)
        coefs.append(coef)
        C.blobs_are_packs(case, (config, leg, s))
        C.check_stats(case, stats, t, norm, coef, hp)
    assert [c < 1.0 for c in coefs] == [True, False, True, False, True], coefs
    C.meets_the_bars(case, yard, ref, config, leg, env=RATIOS)


@pytest.mark.parametrize("config", ["n1", "n3-gaussian"])
def test_no_clipping_and_a_bound_that_never_bites_give_the_bits_of_coefficient_one(config):
    gen = torch.Generator().manual_seed(23)
    off, huge = _case(config, U.hyper32()), _case(config, U.hyper32(max_grad_norm=1e30))
    for _ in range(2):
        rows, g_ls = off.draw(gen)
        off.run(rows, g_ls)
        huge.run(rows, g_ls)
        a, b = ({k: v for k, v in c.bits().items() if k != "stats"} for c in (off, huge))
        assert C.same_bits(a, b) == []
        assert float(off.stats[2]) == 1.0 == float(huge.stats[2]) and torch.equal(off.stats, huge.stats)
    # a bound of 1 does bite on these gradients: 1e30 above was a bound that did not, not a switch that is ignored
    clipped = _case(config, U.hyper32(max_grad_norm=1.0))
    gen = torch.Generator().manual_seed(23)
    rows, g_ls = clipped.draw(gen)
    clipped.run(rows, g_ls)
    assert float(clipped.stats[2]) < 1.0


@pytest.mark.parametrize("config", ["n3-gaussian", "n16", "n16-gaussian", "n1-policy-gaussian"])
def test_two_calls_from_copies_of_one_state_give_identical_bits_and_leave_the_guards_alone(config):
    hp = U.hyper32(max_grad_norm=5.0)
    alloc = GU.Buffers(True)
    a, b = _case(config, hp, alloc=alloc), _case(config, hp)
    gen = torch.Generator().manual_seed(29)
    for _ in range(2):
        rows, g_ls = a.draw(gen)
        a.run(rows, g_ls)
        b.run([r.clone() for r in rows], g_ls.clone() if g_ls is not None else None)
    assert C.same_bits(a.bits(), b.bits()) == []
    assert int(a.step) == 2 and float(a.stats[2]) < 1.0
    assert alloc.stray() == []
    C.blobs_are_packs(a, config)


@pytest.mark.parametrize("max_grad_norm", [0.0, 1.0])
def test_an_agent_with_a_zero_gradient_and_zero_moments_keeps_every_bit(max_grad_norm):
    """What a scripted opponent's agents are to the learner: gradient rows of +0, moments +0.  Parameters, moments and the blob row stay
    as they are, with clipping on and off; the other agents move."""
    case = _case("n3-gaussian", U.hyper32(lr=0.01, max_grad_norm=max_grad_norm))
    for net, blob in zip(case.nets, case.blobs):
        blob.copy_(net.pack())
    frozen = [1, 4]
    before = case.bits()
    rows, g_ls = case.draw(torch.Generator().manual_seed(31))
    for r in rows:
        r[frozen] = 0.0
    g_ls[frozen] = 0.0
    case.run(rows, g_ls)
    after = case.bits()
    assert (float(case.stats[2]) < 1.0) == (max_grad_norm > 0.0)
    for k in before:
        if k in ("step", "stats"):
            continue
        assert torch.equal(before[k][frozen], after[k][frozen]), k
        others = [a for a in range(case.A) if a not in frozen]
        assert not torch.equal(before[k][others], after[k][others]), k


def test_the_binding_refuses_wrong_tensors_by_name():
    from deep_rl_battlespace_amd import learner
    case = _case("n3-gaussian", U.hyper32())
    rows, g_ls = case.draw(torch.Generator().manual_seed(37))
    kw = dict(log_std=case.log_std, g_log_std=g_ls, log_std_state=case.ls_state)

    def call(nets=case.nets, rows=rows, states=case.states, blobs=case.blobs, hyper=case.hyper, step=case.step, **over):
        return learner.adam_step(nets, rows, states, blobs, hyper, step, **dict(kw, **over))
    before = case.bits()
    with pytest.raises(TypeError, match=r"grads\[0\]"):
        call(rows=[rows[0].double(), rows[1]])
    with pytest.raises(ValueError, match=r"grads\[1\]"):
        call(rows=[rows[0], rows[1][:, :-1]])
    with pytest.raises(ValueError, match=r"grads\[0\].*contiguous"):
        call(rows=[rows[0].t().contiguous().t(), rows[1]])
    with pytest.raises(ValueError, match=r"grads\[0\] is on"):
        call(rows=[rows[0].cpu(), rows[1]])
    with pytest.raises(ValueError, match=r"blobs\[1\]"):
        call(blobs=[case.blobs[0], case.blobs[1][:, 1:]])
    with pytest.raises(TypeError, match=r"states\[0\]"):
        call(states=[None, case.states[1]])
    with pytest.raises(ValueError, match="all three or none"):
        call(g_log_std=None)
    with pytest.raises(ValueError, match="g_log_std"):
        call(g_log_std=g_ls[:, :2])
    with pytest.raises(ValueError, match="hyper"):
        call(hyper=case.hyper[:5])
    with pytest.raises(TypeError, match="step"):
        call(step=case.step.int())
    with pytest.raises(TypeError, match="step"):
        call(step=3)
    with pytest.raises(ValueError, match="workspace"):
        call(workspace=torch.empty(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError, match="stats"):
        call(stats=torch.empty(4, device="cuda"))
    w2 = case.nets[0].w2
    case.nets[0].w2 = torch.nn.Parameter(w2.detach().transpose(1, 2))
    with pytest.raises(ValueError, match=r"nets\[0\]\.w2.*contiguous"):
        call()
    case.nets[0].w2 = w2
    assert C.same_bits(before, case.bits()) == []                    # nothing was launched by a refused call


def _row_of(case, index):
    """Partial `index` of a call -> (network, agent), or (None, None) for log_std's (the last partial of a Gaussian call)."""
    rows = len(case.nets) * case.A
    assert 0 <= index < rows + (case.log_std is not None)
    return (index // case.A, index % case.A) if index < rows else (None, None)


@pytest.mark.parametrize("config,index", [("n16-gaussian", i) for i in (0, 31, 32, 63, 64)] + [("n1-policy-gaussian", i) for i in (0, 1, 2)])
def test_each_partial_norm_alone_reaches_the_clip_and_only_its_row_moves(config, index):
    """"Every workgroup adds the (at most 65) partials": one call per partial in which only that workgroup's gradient is non-zero (a
    network's row of one agent, or g_log_std for the last index), moments +0, max_grad_norm half that row's float64 norm.  The norm in
    stats is that row's alone (1e-10 relative), the coefficient bites, the row behind the index moves in every tensor and every other
    parameter, moment and blob row keeps its bits (grad = m = v = +0 keeps p, m, v; the blobs start as pack()).  At n = 16 with two
    networks and log_std, index 64 is the one partial a lane adds as its second; at one network and log_std the last index is block A."""
    case = _case(config, U.hyper32(lr=0.01))
    case.blobs_from_pack()
    drawn, drawn_ls = case.draw(torch.Generator().manual_seed(41 + index))
    rows, g_ls = case.zeros()
    net, agent = _row_of(case, index)
    if net is None:
        g_ls.copy_(drawn_ls)
        alone = g_ls
    else:
        rows[net][agent] = drawn[net][agent]
        alone = rows[net][agent]
    norm = float(np.sqrt(float((alone.double() ** 2).sum())))
    assert norm > 0.0
    hp = U.hyper32(lr=0.01, max_grad_norm=0.5 * norm)
    case.set_hyper(hp)
    before = case.bits()
    stats = case.run(rows, g_ls)
    after = case.bits()
    coef = hp["max_grad_norm"] / (norm + 1e-6)
    print(f"adam_step {config} partial {index}: norm {float(stats[1])!r} want {norm!r}, coef {float(stats[2])!r} want {coef!r}")
    C.check_stats(case, stats, 1, norm, coef, hp)
    assert float(stats[2]) < 1.0
    for k in before:
        if k in ("step", "stats"):
            continue
        if net is None and k in ("log_std", "ls.m", "ls.v"):
            assert bool((before[k] != after[k]).any(dim=1).all()), k                  # every agent's log_std moves
        elif net is not None and k.startswith(f"net{net}."):
            others = [a for a in range(case.A) if a != agent]
            assert torch.equal(before[k][others], after[k][others]), k
            assert not torch.equal(before[k][agent], after[k][agent]), k
        else:
            assert torch.equal(before[k], after[k]), k
    C.blobs_are_packs(case, (config, index))


@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("config", ["n3-gaussian", "n2-value-only"])
def test_poisoned_pad_columns_are_neither_read_nor_written(config, poison):
    """"Columns n_actions..3 of w3 / b3 ... are not read" and the same columns of m, v "are not touched": twins from one seed, B with every
    pad element of its gradient rows at NaN (or 1e30) and of its moments at 7.25.  After each of two clipped steps every tensor of B
    equals A's bit for bit outside the moments' pads -- the norm and the coefficient in stats among them --, B's pads still hold 7.25,
    A's +0, and every blob is pack() (whose pad columns are +0)."""
    hp = U.hyper32(lr=0.01, max_grad_norm=1.0)
    a, b = _case(config, hp, seed=3), _case(config, hp, seed=3)
    masks = [torch.from_numpy(U.pad_mask(a.D, net.n_actions)).cuda() for net in a.nets]
    assert any(int(m.sum()) for m in masks)
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
        b.run(poisoned, g_ls.clone() if g_ls is not None else None)
        x, y = a.bits(), b.bits()
        assert float(a.stats[2]) < 1.0 and int(a.step) == s + 1
        for k in x:
            if k in moments:
                mask = moments[k]
                assert torch.equal(x[k][:, ~mask], y[k][:, ~mask]), (s, k)
                assert bool((y[k][:, mask] == sentinel).all()) and bool((x[k][:, mask] == 0).all()), (s, k)
            else:
                assert torch.equal(x[k], y[k]), (s, k, x[k].view(-1)[:4], y[k].view(-1)[:4])
        C.blobs_are_packs(a, (config, s, "a"))
        C.blobs_are_packs(b, (config, s, "b"))


@pytest.mark.parametrize("max_grad_norm", [0.0, 1.0])
@pytest.mark.parametrize("config", ["n1", "n2-single"])
def test_the_bf16_split_of_the_blob_is_pack_where_rounding_is_decided(config, max_grad_norm):
    """"W2B's three bfloat16 terms (round to nearest even, residuals in float32): bit for bit what StackedActor.pack() makes": w2 of
    every network = adam_util.w2_edge_weights (ties, one bit either side of a tie, carries into the exponent, +-0, exponents -60 .. 60: no
    term or residual is subnormal or overflows, so no denormal mode decides).  One call with gradients and moments +0, clipping off and
    on: every parameter keeps its bits, -0 included; the W2B part of each blob equals the integer restatement (pinned to CPU pack() in
    test_adam_step_cpu.py); the whole blob equals pack() of a CPU copy of the network and pack() on the GPU.  Non-finite weights are a
    diverged run and are not covered."""
    from deep_rl_battlespace_amd.rollout import StackedActor
    case = _case(config, U.hyper32(max_grad_norm=max_grad_norm))
    w2s = [U.w2_edge_weights(case.A, seed=47 + i) for i in range(len(case.nets))]
    with torch.no_grad():
        for net, w2 in zip(case.nets, w2s):
            net.w2.copy_(torch.from_numpy(w2.copy()))
    before = case.bits()
    for i, w2 in enumerate(w2s):
        assert np.array_equal(before[f"net{i}.w2"].cpu().numpy().view(np.uint32), w2.view(np.uint32))
    case.run(*case.zeros())
    after = case.bits()
    kept = lambda bits: {k: v for k, v in bits.items() if k not in ("step", "stats") and not k.endswith(".blob")}     # noqa: E731
    assert C.same_bits(kept(before), kept(after)) == []
    assert int(case.step) == 1 and float(case.stats[1]) == 0.0 and float(case.stats[2]) == 1.0
    for i, (net, w2) in enumerate(zip(case.nets, w2s)):
        got = after[f"net{i}.blob"].cpu().numpy().view(np.uint32)
        bad = np.argwhere(got[:, -U.W2B_FLOATS:] != U.w2b_words(w2))
        assert bad.size == 0, ("restatement", i, bad[:4].tolist())
        host = StackedActor(case.A, case.D, net.n_actions)
        with torch.no_grad():
            for k in U.PARAMS:
                getattr(host, k).copy_(getattr(net, k).detach().cpu())
        on_host, on_gpu = host.pack().numpy().view(np.uint32), net.pack().cpu().numpy().view(np.uint32)
        bad = np.argwhere(on_host != on_gpu)
        assert bad.size == 0, ("pack() on the CPU and on the GPU differ", i, bad[:4].tolist())
        bad = np.argwhere(got != on_host)
        assert bad.size == 0, ("pack()", i, bad[:4].tolist())


@pytest.mark.parametrize("t0", [2 ** 31 + 5, 2 ** 40], ids=["2^31+5", "2^40"])
@pytest.mark.parametrize("config", ["n2", "n3-gaussian"])
def test_a_counter_beyond_int32_counts_exactly_and_steps_with_bias_corrections_of_one(config, t0):
    """`step` is an int64 read on the device: set beyond int32 before the first of three steps (the second a tenth of the others, so
    max_grad_norm, half the first norm, bites on 1 and 3), stats[0] and `step` hold the exact count after each, every blob is pack(), and
    the result meets the five-step test's bars.  For t >= 2^24 both bias corrections are exactly 1 in float64 (0.999^t < 2^-53 from about
    t = 36 700 on), so the torch yardstick, whose counter is a float32, runs with it at 2^24, where it stays."""
    first = C.first_norm(*_shape(config), seed=53)
    hp = U.hyper32(max_grad_norm=0.5 * first)
    assert 1.0 - hp["beta1"] ** 2 ** 24 == 1.0 == 1.0 - hp["beta2"] ** 2 ** 24
    case = _case(config, hp)
    yard = C.TorchPath(case, hp, t0=2 ** 24)
    ref = C.start(case)
    case.step.fill_(t0)
    t, coefs = t0, []
    gen = torch.Generator().manual_seed(53)
    for s in range(3):
        rows, g_ls = case.draw(gen, 0.1 if s == 1 else 1.0)
        grads = C.flat_split(case, rows, g_ls)
        stats = case.run(rows, g_ls)
        yard.step(grads)
        t, norm, coef = C.advance(ref, grads, t, hp)
        coefs.append(coef)
        assert t == t0 + s + 1
        C.check_stats(case, stats, t, norm, coef, hp)
        C.blobs_are_packs(case, (config, t0, s))
    assert [c < 1.0 for c in coefs] == [True, False, True], coefs
    assert all(float(yard.opt.state[p]["step"]) == 2 ** 24 for p in yard.flat)
    C.meets_the_bars(case, yard, ref, config, f"counter-{t0}", env=RATIOS)


def test_a_learning_rate_of_zero_moves_the_moments_and_no_parameter():
    """lr = 0, two clipped steps: step_size is 0, so parameters and blobs (pack() before the call) keep every bit while m and v move and
    meet the bars; `step` advances and stats[3] is 0."""
    config = "n3-gaussian"
    hp = U.hyper32(lr=0.0, max_grad_norm=1.0)
    case = _case(config, hp)
    case.blobs_from_pack()
    yard = C.TorchPath(case, hp)
    ref = C.start(case)
    before = case.bits()
    gen, t = torch.Generator().manual_seed(59), 0
    for s in range(2):
        rows, g_ls = case.draw(gen)
        grads = C.flat_split(case, rows, g_ls)
        stats = case.run(rows, g_ls)
        yard.step(grads)
        t, norm, coef = C.advance(ref, grads, t, hp)
        C.check_stats(case, stats, t, norm, coef, hp)
        assert coef < 1.0 and float(stats[3]) == 0.0
    after = case.bits()
    moments = [k for k in before if k.endswith((".m", ".v"))]
    assert len(moments) == 2 * len(case.nets) + 2
    assert sorted(C.same_bits(before, after)) == sorted(moments + ["step", "stats"])
    assert int(case.step) == 2
    C.meets_the_bars(case, yard, ref, config, "lr0", which=("m", "v"), env=RATIOS)


def test_an_all_zero_gradient_under_clipping_has_norm_zero_and_coefficient_exactly_one():
    """Every gradient +0 with max_grad_norm = 1: norm = 0, coef = min(1, 1 / 1e-6) = 1 exactly; moments are +0, so nothing but `step`
    and stats changes (the blobs hold pack() before the call and after it)."""
    case = _case("n3-gaussian", U.hyper32(lr=0.01, max_grad_norm=1.0))
    case.blobs_from_pack()
    before = case.bits()
    stats = case.run(*case.zeros())
    after = case.bits()
    assert stats.tolist() == [1.0, 0.0, 1.0, U.hyper32(lr=0.01)["lr"]]
    assert sorted(C.same_bits(before, after)) == ["stats", "step"] and int(case.step) == 1
    C.blobs_are_packs(case, "all-zero")
