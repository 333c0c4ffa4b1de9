"""Device-resident transition store: the step after the path.

Mirror of the reference's team replay buffer (maddpg/buffer.py:3-70): same constructor arguments, `store_transition`,
`sample`, `is_ready`, same tuple layout out of `sample()` -- but every array is a torch tensor on the env's device, one
call stores the transitions of ALL games at once (each game contributes one row), and a whole `PolicyRollout` (T ticks)
can be appended without a host copy.  The reference keeps float64 numpy arrays on the host and converts a sampled batch
to float32 tensors for the learner (maddpg/team.py:33-37); here rows are float32 from the start.

Ring semantics are the reference's: row index = counter % mem_size, oldest rows overwritten; `sample()` draws
`batch_size` indices uniformly WITH replacement among the filled rows (np.random.choice, buffer.py:51)."""
import torch


class ReplayBuffer:
    def __init__(self, mem_size, batch_size, agent_list, obs_size, critic_dims, n_actions, device="cuda", generator=None):
        self.mem_size, self.batch_size = int(mem_size), int(batch_size)
        self.agent_list, self.n_agents = list(agent_list), len(agent_list)
        if critic_dims != obs_size * self.n_agents:
            raise ValueError("critic_dims must be obs_size * len(agent_list) (main.py:118)")
        self.mem_cntr = 0
        kw = dict(device=device, dtype=torch.float32)
        nA, M = self.n_agents, self.mem_size
        self.actor_states = torch.zeros((M, nA, obs_size), **kw)        # state_mem is the [M, nA*obs] view of this
        self.actor_new_states = torch.zeros((M, nA, obs_size), **kw)
        self.n_actions = int(n_actions)
        self.action_mem = torch.zeros((M, nA, n_actions), **kw)
        self.rew_mem = torch.zeros((M, nA), **kw)
        self.done_mem = torch.zeros((M, nA), device=device, dtype=torch.bool)
        self.generator = generator

    @property
    def state_mem(self):
        return self.actor_states.view(self.mem_size, -1)

    @property
    def new_state_mem(self):
        return self.actor_new_states.view(self.mem_size, -1)

    def _put(self, obs, act, rew, obs_, done):
        """rows: obs [R, nA, obs], act [R, nA, n_actions], rew [R, nA], obs_ [R, nA, obs], done [R, nA]."""
        R = obs.shape[0]
        if R > self.mem_size:                                            # only the newest mem_size rows can survive
            obs, act, rew, obs_, done = (t[-self.mem_size:] for t in (obs, act, rew, obs_, done))
            self.mem_cntr += R - self.mem_size
            R = self.mem_size
        start = self.mem_cntr % self.mem_size
        first = min(R, self.mem_size - start)
        for dst, src in ((self.actor_states, obs), (self.action_mem, act), (self.rew_mem, rew),
                         (self.actor_new_states, obs_), (self.done_mem, done)):
            dst[start:start + first].copy_(src[:first])
            if first < R:
                dst[:R - first].copy_(src[first:])
        self.mem_cntr += R

    def store_transition(self, states, actions, rewards, states_, dones):
        """buffer.py:25-47, batched: every dict value carries a leading game axis E (a plain per-game value, as the
        reference passes, is one row).  Discrete actions given as indices are stored one-hot."""
        def col(d, a, width=None):
            v = torch.as_tensor(d[a], device=self.actor_states.device)
            return v.reshape(-1, width) if width else v.reshape(-1)
        obs = torch.stack([col(states, a, self.actor_states.shape[2]) for a in self.agent_list], 1).float()
        obs_ = torch.stack([col(states_, a, self.actor_states.shape[2]) for a in self.agent_list], 1).float()
        acts = []
        for a in self.agent_list:
            v = torch.as_tensor(actions[a], device=obs.device)
            if not v.is_floating_point():
                v = torch.nn.functional.one_hot(v.reshape(-1).long(), self.action_mem.shape[2])
            acts.append(v.reshape(-1, self.action_mem.shape[2]).float())
        self._put(obs, torch.stack(acts, 1), torch.stack([col(rewards, a) for a in self.agent_list], 1).float(),
                  obs_, torch.stack([col(dones, a) for a in self.agent_list], 1).bool())

    def store_rollout(self, rollout, columns):
        """Append the transitions of a PolicyRollout for the agents in `columns` (env column indices of this team, e.g.
        range(n) for red), tick-major, without a host copy of the data.  Only rows of RUNNING games are transitions
        (`rollout.valid`): a tick on a finished game is the reference's inert call (battle_env.py:303-306) or, with
        auto_reset, the re-spawn -- its row would pair the old game's last observation with the new game's first under
        done=False, and the reference's loop (`while not env.env_done`, main.py:177-181) never stores such a row.
        Returns the number of rows stored (one host sync: the count decides where the ring wraps)."""
        c = torch.as_tensor(list(columns), device=rollout.obs.device)
        T = rollout.T
        keep = rollout.valid.reshape(-1).nonzero().squeeze(1)                      # [R] indices into the T*E rows, tick-major
        flat = lambda x: x.index_select(2, c).reshape(-1, len(c), *x.shape[3:]).index_select(0, keep)   # noqa: E731
        self._put(flat(rollout.obs[:T]), flat(rollout.scores)[..., :self.n_actions], flat(rollout.rew), flat(rollout.obs[1:T + 1]), flat(rollout.done))
        return int(keep.numel())

    def sample(self, idx=None):
        """buffer.py:49-67 -> (actor_states [nA, B, obs], states [B, nA*obs], actions [nA, B, n_actions], rewards [B, nA],
        actor_new_states [nA, B, obs], states_ [B, nA*obs], dones [B, nA]), all on the device.
        idx: optional row indices to return instead of drawing them (parity runs with the reference's np.random.choice draw)."""
        max_mem = min(self.mem_cntr, self.mem_size)
        if idx is None:
            idx = torch.randint(0, max_mem, (self.batch_size,), device=self.actor_states.device, generator=self.generator)
        else:
            idx = torch.as_tensor(idx, device=self.actor_states.device).long()
            if idx.shape != (self.batch_size,) or int(idx.max()) >= max_mem or int(idx.min()) < 0:
                raise ValueError("idx must be batch_size indices into the filled rows")
        o, o_, a = self.actor_states[idx], self.actor_new_states[idx], self.action_mem[idx]
        B = self.batch_size
        return (o.transpose(0, 1), o.reshape(B, -1), a.transpose(0, 1), self.rew_mem[idx],
                o_.transpose(0, 1), o_.reshape(B, -1), self.done_mem[idx])

    def is_ready(self):
        return self.mem_cntr >= self.batch_size


class DeviceReplayBuffer(ReplayBuffer):
    """The same ring with its control on the device too: the counter is a device int64 and storing and sampling are HIP kernels
    (csrc/bsx_replay.hip: bsx_replay_append / bsx_replay_sample) that never wait for the host, so a rollout, its store and a
    learner batch can be one captured HIP graph (`PolicyRollout.capture(then=...)`).  Same memory tensors and layout as
    ReplayBuffer (state_mem / new_state_mem views included), and the same rows, bit for bit, for the same inputs.

        buf = DeviceReplayBuffer(1_000_000, 512, env.possible_red, env.obs_size, env.obs_size * n, 4, device="cuda", seed=0)
        buf.append_rollout(ro, range(n))      # asynchronous; returns the device word holding the number of rows stored
        batch = buf.sample()                  # asynchronous; tensors the NEXT sample() overwrites; buf.last_idx = the rows drawn

    `sample()` draws with Philox4x32-10 keyed by (seed, a draw counter on the device, position in the batch) instead of the torch
    generator; `sample(idx=...)` is the base behaviour (parity runs).  `mem_cntr` and `is_ready()` read the device counter: one
    host synchronisation each, a convenience for host code, not for the collect loop."""

    def __init__(self, mem_size, batch_size, agent_list, obs_size, critic_dims, n_actions, device="cuda", generator=None, seed=0):
        self._counter = torch.zeros(1, dtype=torch.int64, device=device)   # first: the base constructor assigns mem_cntr = 0
        super().__init__(mem_size, batch_size, agent_list, obs_size, critic_dims, n_actions, device=device, generator=generator)
        from . import _lib
        self._lib = _lib
        nA, D, M, B, k = self.n_agents, int(obs_size), self.mem_size, self.batch_size, self.n_actions
        if not (1 <= nA <= _lib.MAX_N and 1 <= D <= 3 * _lib.MAX_N + 2 and k in (3, 4) and 1 <= M < 2 ** 31 and 1 <= B < 2 ** 31):
            raise ValueError("the device ring takes 1..16 agents, observations of 1..50 floats, 3 or 4 actions, mem_size and batch_size "
                             "in [1, 2^31)")
        self.seed = int(seed)
        dev = self.actor_states.device
        self._draws = torch.zeros(1, dtype=torch.int64, device=dev)       # the sampler's sequence word, advanced once per sample()
        self._stored = torch.zeros(1, dtype=torch.int64, device=dev)      # rows kept by the latest append
        # append workspaces are only ever added: a captured graph keeps the address it was recorded with
        self._workspaces = [torch.empty(0, dtype=torch.int64, device=dev)]
        kw = dict(device=dev, dtype=torch.float32)
        self._b_obs, self._b_obs_ = torch.zeros((B, nA, D), **kw), torch.zeros((B, nA, D), **kw)
        self._b_act, self._b_rew = torch.zeros((B, nA, k), **kw), torch.zeros((B, nA), **kw)
        self._b_done = torch.zeros((B, nA), device=dev, dtype=torch.bool)
        self.last_idx = torch.zeros(B, device=dev, dtype=torch.int64)
        self._ring = _lib.BsxReplayRing(self.actor_states.data_ptr(), self.actor_new_states.data_ptr(), self.action_mem.data_ptr(),
                                        self.rew_mem.data_ptr(), self.done_mem.data_ptr(), self._counter.data_ptr(), M, nA, D, k)

    @property
    def mem_cntr(self):
        return int(self._counter.item())

    @mem_cntr.setter
    def mem_cntr(self, value):
        if int(value) < 0:
            raise ValueError("mem_cntr counts the rows ever stored: it cannot be negative")
        self._counter.fill_(int(value))

    def _stream(self):
        return torch.cuda.current_stream(self.actor_states.device).cuda_stream

    def _append(self, src, rows):
        import ctypes
        lib = self._lib.load()
        need = ctypes.c_size_t()
        self._lib.check(lib.bsx_replay_workspace_bytes(rows, ctypes.byref(need)), "bsx_replay_workspace_bytes")
        if self._workspaces[-1].numel() * 8 < need.value:
            self._workspaces.append(torch.empty((need.value + 7) // 8, dtype=torch.int64, device=self.actor_states.device))
        self._lib.check(lib.bsx_replay_append(ctypes.byref(self._ring), ctypes.byref(src), rows, self._workspaces[-1].data_ptr(),
                                              self._stored.data_ptr(), self._stream()), "bsx_replay_append")
        return self._stored

    def _put(self, obs, act, rew, obs_, done):
        """Dense rows (what store_transition builds): obs / obs_ [R, nA, obs], act [R, nA, n_actions], rew [R, nA], done bool [R, nA]."""
        R, nA, D, k = obs.shape[0], self.n_agents, self.actor_states.shape[2], self.n_actions
        if R == 0:
            return
        obs, act, rew, obs_ = (t.to(torch.float32).contiguous() for t in (obs, act, rew, obs_))
        done = done.to(torch.bool).contiguous().view(torch.uint8)
        if obs.shape != (R, nA, D) or obs_.shape != (R, nA, D) or act.shape != (R, nA, k) or rew.shape != (R, nA) or done.shape != (R, nA):
            raise ValueError("rows must be [R, nA, obs], [R, nA, n_actions], [R, nA], [R, nA, obs], [R, nA]")
        src = self._lib.BsxReplaySource(obs.data_ptr(), nA * D, D, obs_.data_ptr(), nA * D, D, act.data_ptr(), nA * k, k,
                                        rew.data_ptr(), nA, 1, done.data_ptr(), nA, 1, None, 0)
        self._append(src, R)

    def append_rollout(self, rollout, columns):
        """store_rollout without the host: the kept rows of a PolicyRollout (running games only, tick-major) go into the ring straight
        from the rollout's tensors.  Asynchronous and capturable.  `columns`: this team's env columns, a contiguous range (as
        instinct.Team._cols are).  Returns the device int64 [1] holding the number of rows stored (overwritten by the next append)."""
        cols = [int(c) for c in columns]
        T, (_, E, A, D) = rollout.T, tuple(rollout.obs.shape)
        c0 = cols[0] if cols else 0
        if len(cols) != self.n_agents or cols != list(range(c0, c0 + len(cols))) or c0 < 0 or c0 + len(cols) > A:
            raise ValueError("columns must be a contiguous range of len(agent_list) env columns")
        if D != self.actor_states.shape[2] or rollout.obs.device != self.actor_states.device:
            raise ValueError("the rollout's observations do not fit this ring")
        src = self._lib.BsxReplaySource(rollout.obs.data_ptr() + 4 * c0 * D, A * D, D, rollout.obs[1].data_ptr() + 4 * c0 * D, A * D, D,
                                        rollout.scores.data_ptr() + 16 * c0, A * 4, 4, rollout.rew.data_ptr() + 4 * c0, A, 1,
                                        rollout._done.data_ptr() + c0, A, 1, rollout.env_done.data_ptr(), 1)
        return self._append(src, T * E)

    def store_rollout(self, rollout, columns):
        """append_rollout, then the number of rows stored as a Python int (one host synchronisation): the base's return."""
        return int(self.append_rollout(rollout, columns).item())

    def sample(self, idx=None):
        """The base's tuple, drawn and gathered in one HIP launch (capturable).  Its tensors are views of buffers that the NEXT
        sample() overwrites; `last_idx` holds the indices drawn.  idx: the base behaviour (parity runs)."""
        if idx is not None:
            return super().sample(idx)
        import ctypes
        lib, B = self._lib.load(), self.batch_size
        self._lib.check(lib.bsx_replay_sample(ctypes.byref(self._ring), B, self.seed, 0, self._draws.data_ptr(), self.last_idx.data_ptr(),
                                              self._b_obs.data_ptr(), self._b_obs_.data_ptr(), self._b_act.data_ptr(), self._b_rew.data_ptr(),
                                              self._b_done.data_ptr(), self._stream()), "bsx_replay_sample")
        self._draws.add_(1)                              # fresh indices next call, and on every replay of a captured graph
        o, o_, a = self._b_obs, self._b_obs_, self._b_act
        return (o.transpose(0, 1), o.reshape(B, -1), a.transpose(0, 1), self._b_rew,
                o_.transpose(0, 1), o_.reshape(B, -1), self._b_done)


def prio_levels(M):
    """The int64 levels of the sum tree over M rows (include/battlespace_hip.h, BsxPrioTree) -> [(offset, count), ...] bottom-up, in
    nodes of the one node buffer: level 0 has ceil(M / 64) nodes (each the sum of 64 leaves), every next one ceil(previous / 64), the last
    is the root.  The leaves are a buffer of their own: uint32 [64 * ceil(M / 64)]."""
    M = int(M)
    if not 1 <= M < 2 ** 31:
        raise ValueError("prio_levels: 1 <= M < 2^31 is needed")
    out, off, n = [], 0, -(-M // 64)
    while True:
        out.append((off, n))
        if n == 1:
            return out
        off, n = off + n, -(-n // 64)


class PrioritizedReplayBuffer(DeviceReplayBuffer):
    """DeviceReplayBuffer with proportional prioritised sampling (Schaul et al. 2016) kept wholly on the device
    (csrc/bsx_replay_prio.hip; the contract is written out in include/battlespace_hip.h at BsxPrioTree): a sum tree of fan-out 64 over
    integer priorities that `sample()`, the three store calls and `update_priorities()` keep current, O(B log M) words per call, all of
    it asynchronous, capturable and free of allocation after construction.

        buf = PrioritizedReplayBuffer(1_000_000, 512, env.possible_red, env.obs_size, env.obs_size * n, 4, seed=0, alpha=0.6, beta=0.4)
        buf.append_rollout(ro, range(n))       # the new rows get `max_priority`
        batch = buf.sample()                   # P(row) = p / sum p; buf.weights [B, nA] = (p_min / p) ^ beta, buf.last_idx = the rows
        buf.update_priorities(q, y)            # p = (min(max_i |q - y|, delta_max) + eps) ^ alpha for the rows of last_idx

    A priority is a uint32 fixed-point number of scale 2^16 (65536 = 1.0): 0 = never stored (never drawn), a stored row has 1 .. 2^31,
    and every tree node is the exact int64 sum of its children, so tree and draw are reproducible bit for bit (tests/prio_util.py
    restates them in numpy).  Public state, all on the device:
      priorities    the M leaves, an int32-TYPED view of the uint32 words (torch has no arithmetic on uint32): 2^31 reads as -2^31,
                    `priorities.view(torch.uint32)` or `& 0xFFFFFFFF` in int64 gives the value.  Write it, then call rebuild_tree()
      tree          int64 [nodes]: the levels of prio_levels(M), concatenated bottom-up; the last word is the root, the sum of all
      max_priority  int32-typed [1]: the largest priority an update has written (65536 at first); what a fresh row gets
      prio_hyper    float32 [4]: alpha, beta, eps, delta_max (set_alpha / set_beta fill it: a captured graph reads it at every replay)
      weights       float32 [B, nA]: the latest batch's importance weights, normalised by the batch's largest, one value across a row
    `sample(idx=...)` returns the given rows (the base behaviour) and fills `weights` and `last_idx` for them.  Setting `mem_cntr` is
    refused: the tree would no longer describe the ring."""

    def __init__(self, mem_size, batch_size, agent_list, obs_size, critic_dims, n_actions, device="cuda", generator=None, seed=0,
                 alpha=0.6, beta=0.4, eps=1e-6, delta_max=32.0):
        super().__init__(mem_size, batch_size, agent_list, obs_size, critic_dims, n_actions, device=device, generator=generator, seed=seed)
        hyper = [float(alpha), float(beta), float(eps), float(delta_max)]
        if not (hyper[0] >= 0.0 and hyper[1] >= 0.0 and hyper[2] >= 0.0 and hyper[3] > 0.0):
            raise ValueError("alpha, beta and eps must be >= 0 and delta_max > 0")
        dev, M, B = self.actor_states.device, self.mem_size, self.batch_size
        levels = prio_levels(M)
        self._leaves = torch.zeros(64 * levels[0][1], dtype=torch.int32, device=dev)
        self.priorities = self._leaves[:M]
        self.tree = torch.zeros(levels[-1][0] + 1, dtype=torch.int64, device=dev)
        self.max_priority = torch.full((1,), 65536, dtype=torch.int32, device=dev)
        self.prio_hyper = torch.tensor(hyper, dtype=torch.float32, device=dev)
        self.weights = torch.zeros((B, self.n_agents), dtype=torch.float32, device=dev)
        self._drawn = torch.zeros(B, dtype=torch.int32, device=dev)        # the leaves of the rows drawn: the weights' workspace
        self._tree = self._lib.BsxPrioTree(self._leaves.data_ptr(), self.tree.data_ptr(), self.max_priority.data_ptr(),
                                           self.prio_hyper.data_ptr(), M)
        if dev.type == "cuda":
            self.rebuild_tree()

    mem_cntr = property(DeviceReplayBuffer.mem_cntr.fget)

    @mem_cntr.setter
    def mem_cntr(self, value):
        if "_tree" in self.__dict__:                 # (the base constructor's `mem_cntr = 0` comes before the tree)
            raise ValueError("mem_cntr of a PrioritizedReplayBuffer cannot be set: the priority tree would no longer describe the ring")

    def _prio(self, entry, *args):
        import ctypes
        self._lib.check(getattr(self._lib.load(), entry)(ctypes.byref(self._tree), *args, self._stream()), entry)

    def rebuild_tree(self):
        """Every level of `tree` recomputed from `priorities`: after they have been written directly.  Asynchronous."""
        self._prio("bsx_replay_prio_rebuild")

    def set_alpha(self, alpha):
        """The exponent of the priorities written from now on (a device fill: no host synchronisation; leaves already written stay)."""
        if not float(alpha) >= 0.0:
            raise ValueError("alpha must be >= 0")
        self.prio_hyper[0].fill_(float(alpha))

    def set_beta(self, beta):
        """The exponent of the importance weights from the next sample() on, inside a captured graph too (a device fill)."""
        if not float(beta) >= 0.0:
            raise ValueError("beta must be >= 0")
        self.prio_hyper[1].fill_(float(beta))

    def _append(self, src, rows):
        """The ring's three launches, then bsx_replay_prio_append: the rows just written get max_priority, the tree is repaired."""
        stored = super()._append(src, rows)
        self._prio("bsx_replay_prio_append", self._counter.data_ptr(), stored.data_ptr(), rows)
        return stored

    def sample(self, idx=None):
        """The base's tuple, drawn in proportion to the priorities and gathered in one launch, `weights` in a second; `last_idx` holds the
        rows.  idx: these rows instead (the base's checks and one host synchronisation), with `weights` and `last_idx` filled for them."""
        import ctypes
        B = self.batch_size
        if idx is not None:
            out = ReplayBuffer.sample(self, idx)
            self.last_idx.copy_(torch.as_tensor(idx, device=self.last_idx.device).long())
            self._prio("bsx_replay_prio_weights", self.last_idx.data_ptr(), B, self.n_agents, self.weights.data_ptr(), self._drawn.data_ptr())
            return out
        self._lib.check(self._lib.load().bsx_replay_prio_sample(
            ctypes.byref(self._ring), ctypes.byref(self._tree), B, self.seed, 0, self._draws.data_ptr(), self.last_idx.data_ptr(),
            self._b_obs.data_ptr(), self._b_obs_.data_ptr(), self._b_act.data_ptr(), self._b_rew.data_ptr(), self._b_done.data_ptr(),
            self.weights.data_ptr(), self._drawn.data_ptr(), self._stream()), "bsx_replay_prio_sample")
        self._draws.add_(1)
        o, o_, a = self._b_obs, self._b_obs_, self._b_act
        return (o.transpose(0, 1), o.reshape(B, -1), a.transpose(0, 1), self._b_rew,
                o_.transpose(0, 1), o_.reshape(B, -1), self._b_done)

    def update_priorities(self, q, y, idx=None):
        """New priorities for the rows of idx (int64 [B]; `last_idx` if None) from q and y float32 [B, nA] -- td_head's q and td: per row
        the largest |q - y| of its agents, clipped to delta_max (a NaN counts as delta_max), + eps, to the power alpha; a row named more
        than once keeps the largest; max_priority and the tree follow.  Asynchronous; 5 launches at M = 2^20."""
        B, nA = self.batch_size, self.n_agents
        idx = self.last_idx if idx is None else idx
        for t, name, shape, dtype in ((q, "q", (B, nA), torch.float32), (y, "y", (B, nA), torch.float32), (idx, "idx", (B,), torch.int64)):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() \
                    or t.device != self._leaves.device:
                raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {self._leaves.device}")
        self._prio("bsx_replay_prio_update", idx.data_ptr(), q.data_ptr(), y.data_ptr(), B, nA)


class NStepAppender:
    """n-step returns in front of a device ring (csrc/bsx_replay_nstep.hip; the contract is written out in include/battlespace_hip.h at
    BsxNstepCarry): a rollout's records are folded on the device into rows (obs[t], act[t], sum_j gamma^j rew[t+j], obs[t+m], done) and
    stored through the ring's own append, so a DeviceReplayBuffer or a PrioritizedReplayBuffer, and every learner on it, gain n-step
    targets with no change of their own: give the learner `gamma=app.bootstrap_gamma`.

        app = NStepAppender(buf, n=3, gamma=0.95, T=ro.T, E=env.n_envs)
        stored = app.append_rollout(ro, range(nA))                   # device int64 [1], as buf.append_rollout returns
        learner = DDPGLearner(buf, actor, gamma=app.bootstrap_gamma) # likewise TD3Learner, SACLearner
        app.reset_carry(mask)                                        # after an env.reset(mask=...) of running games

    A window ends early at a game's end (m < n ticks; every agent's done is then set, so that one scalar gamma^n is exact in the heads).
    The last n - 1 ticks of a rollout have windows that run into the next one: they are CARRIED, not stored, and the next call completes
    and stores them first.  Every tick therefore reaches the ring once, in tick order, whatever T cuts the run into; `carry_valid` (uint8
    [E], 0 at first) says whose carried ticks count, so the first call stores T - n + 1 ticks of each running game.  A game that the host
    re-spawns between two calls (`env.reset(mask=...)`) must have its carried ticks dropped: `reset_carry(mask)`; games that end and
    re-spawn inside a rollout (auto_reset) need nothing.  n = 1 stores exactly what `buf.append_rollout` stores.
    Asynchronous, capturable (`PolicyRollout.capture(then=lambda: app.append_rollout(ro, cols))`), nothing is allocated after
    construction.  Two more launches than the plain append (fold, carry) plus the staging traffic: profiles/nstep_append.json."""

    def __init__(self, buf, n, gamma, T, E):
        if not isinstance(buf, DeviceReplayBuffer):
            raise ValueError("NStepAppender needs a DeviceReplayBuffer or a PrioritizedReplayBuffer")
        n, T, E, gamma = int(n), int(T), int(E), float(gamma)
        _lib = buf._lib
        if not (1 <= n <= _lib.NSTEP_MAX and n <= T <= _lib.MAX_T and E >= 1 and T * E < 2 ** 31):
            raise ValueError(f"NStepAppender takes 1 <= n <= {_lib.NSTEP_MAX}, n <= T <= {_lib.MAX_T}, E >= 1 and T * E < 2^31")
        if not 0.0 <= gamma <= 1.0:                      # (a NaN fails both comparisons)
            raise ValueError("gamma must lie in [0, 1]")
        self.buf, self.n_step, self.gamma, self.T, self.E = buf, n, gamma, T, E
        g = torch.ones((), dtype=torch.float32)
        for _ in range(n):                               # g_n of the kernel's chain: float32 products, one rounding each
            g = g * torch.tensor(gamma, dtype=torch.float32)
        self.bootstrap_gamma = float(g)
        nA, D, k, dev = buf.n_agents, buf.actor_states.shape[2], buf.n_actions, buf.actor_states.device
        c = n - 1
        self._c_obs = torch.zeros((c, E, nA, D), dtype=torch.float32, device=dev)
        self._c_act = torch.zeros((c, E, nA, k), dtype=torch.float32, device=dev)
        self._c_rew = torch.zeros((c, E, nA), dtype=torch.float32, device=dev)
        self._c_done = torch.zeros((c, E, nA), dtype=torch.uint8, device=dev)
        self._c_env_done = torch.zeros((c, E), dtype=torch.uint8, device=dev)
        self.carry_valid = torch.zeros(E, dtype=torch.uint8, device=dev)
        need = _lib.query_bytes("bsx_replay_nstep_workspace_bytes", T, E, nA, D, k, n)
        self._staging = torch.empty((need + 3) // 4, dtype=torch.int32, device=dev)
        self._folded = _lib.BsxReplaySource()
        self._bind()
        # the ring's own append workspace for T * E rows, now: nothing is allocated once rollouts are flowing (or being captured)
        need = _lib.query_bytes("bsx_replay_workspace_bytes", T * E)
        if buf._workspaces[-1].numel() * 8 < need:
            buf._workspaces.append(torch.empty((need + 7) // 8, dtype=torch.int64, device=dev))

    def _bind(self):
        """The carry's addresses as the C entry points take them (n = 1: the empty tensors are passed as NULL)."""
        ptr = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
        self._carry = self.buf._lib.BsxNstepCarry(ptr(self._c_obs), ptr(self._c_act), ptr(self._c_rew), ptr(self._c_done), ptr(self._c_env_done),
                                                  self.carry_valid.data_ptr())

    def reset_carry(self, mask=None):
        """Drop the carried ticks of the games in `mask` (bool [E], on the device; None = every game): they are not stored, and the next
        call starts those games' windows at its own first tick.  Asynchronous (a device fill)."""
        if mask is None:
            self.carry_valid.zero_()
            return
        mask = torch.as_tensor(mask, device=self.carry_valid.device)
        if mask.dtype != torch.bool or tuple(mask.shape) != (self.E,):
            raise ValueError("mask must be a bool tensor of shape [E]")
        self.carry_valid.masked_fill_(mask, 0)

    def append(self, obs, act, rew, done, env_done, columns):
        """The fold and the store of one rollout-shaped record: obs float32 [T + 1, E, A, D], act float32 [T, E, A, >= n_actions] (the
        first n_actions of each row are stored), rew float32 [T, E, A], done uint8 / bool [T, E, A] (the agent's flag after tick t),
        env_done uint8 / bool [T + 1, E] (the game's flag BEFORE tick t), all contiguous and on the ring's device; `columns`: this team's
        columns of the A axis, a contiguous range.  Returns the device int64 [1] of rows stored (overwritten by the next append)."""
        import ctypes
        buf, lib, T, E, n = self.buf, self.buf._lib.load(), self.T, self.E, self.n_step
        nA, D, k, dev = buf.n_agents, buf.actor_states.shape[2], buf.n_actions, buf.actor_states.device
        if obs.dim() != 4 or tuple(obs.shape[:2]) != (T + 1, E) or obs.shape[3] != D or obs.device != dev:
            raise ValueError(f"the record's observations must be [T + 1, E, A, D] = [{T + 1}, {E}, A, {D}] on {dev}: this appender was built "
                             f"for that rollout length, game count, observation width and device")
        A = obs.shape[2]
        byte = (torch.uint8, torch.bool)
        for t, name, shape, dtypes in ((obs, "obs", (T + 1, E, A, D), (torch.float32,)), (act, "act", (T, E, A, act.shape[-1]), (torch.float32,)),
                                       (rew, "rew", (T, E, A), (torch.float32,)), (done, "done", (T, E, A), byte),
                                       (env_done, "env_done", (T + 1, E), byte)):
            if tuple(t.shape) != shape or t.dtype not in dtypes or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} must be a contiguous {dtypes[0]} tensor of shape {shape} on {dev}")
        Ka = act.shape[-1]
        cols = [int(c) for c in columns]
        c0 = cols[0] if cols else 0
        if len(cols) != nA or cols != list(range(c0, c0 + len(cols))) or c0 < 0 or c0 + len(cols) > A or Ka < k:
            raise ValueError("columns must be a contiguous range of len(agent_list) columns, act rows at least n_actions wide")
        src = buf._lib.BsxReplaySource(obs.data_ptr() + 4 * c0 * D, A * D, D, None, 0, 0, act.data_ptr() + 4 * Ka * c0, A * Ka, Ka,
                                       rew.data_ptr() + 4 * c0, A, 1, done.data_ptr() + c0, A, 1, env_done.data_ptr(), 1)
        stream = buf._stream()
        buf._lib.check(lib.bsx_replay_nstep_fold(ctypes.byref(src), ctypes.byref(self._carry), T, E, nA, D, k, n, self.gamma,
                                                 self._staging.data_ptr(), ctypes.byref(self._folded), stream), "bsx_replay_nstep_fold")
        stored = buf._append(self._folded, T * E)
        buf._lib.check(lib.bsx_replay_nstep_carry(ctypes.byref(src), ctypes.byref(self._carry), T, E, nA, D, k, n, stream),
                       "bsx_replay_nstep_carry")
        return stored

    def append_rollout(self, rollout, columns):
        """`append` on a PolicyRollout's own tensors, read in place."""
        if rollout.T != self.T:
            raise ValueError(f"this appender was built for rollouts of T = {self.T} ticks")
        return self.append(rollout.obs, rollout.scores, rollout.rew, rollout._done, rollout.env_done, columns)
