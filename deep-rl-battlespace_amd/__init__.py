"""deep-rl-battlespace_amd -- the Battlespace step() path, batched, on MI355X.

Only what the hot path needs lives here:
  csrc/          hand-written HIP kernels for gfx950 + the C ABI of include/battlespace_hip.h
  build.py       hipcc recipe for csrc/ (in-tree libbattlespace_hip.so)
  _lib.py        ctypes binding of the C ABI (fails loudly when the library is missing)
  _args.py       the tensor, number and workspace checks of advantage.py and learner/
  envs/battle_env.py   `parallel_env`: the reference's PettingZoo ParallelEnv surface, batched over n_envs
  spaces.py      Box / Discrete metadata containers (gym is not a dependency)
  sharding.py    one contiguous env range per rank (no collective on the step path)
  instinct/      the reference's scripted opponent, evaluated on device (next row f-2)
  rollout.py     on-device actor + step loop in one HIP graph (next row f-1); csrc/bsx_actor.hip is its MFMA actor
  replay.py      device-resident transition ring, mirror of maddpg/buffer.py (next row f-3), and its prioritised form: a sum tree of
                 integer priorities kept current on the device (csrc/bsx_replay_prio.hip); NStepAppender folds a rollout's records
                 into n-step rows in front of either ring, carried across rollouts (csrc/bsx_replay_nstep.hip)
  advantage.py   GAE advantages / returns / per-agent mask of a rollout on device, for on-policy learners (csrc/bsx_advantage.hip)
  learner/       the on-device learners, one module per kernel family:
    mlp.py       the actor / value MLP as one fused forward and one fused backward for on-device learners (csrc/bsx_actor_grad.hip)
    ppo.py       the PPO loss head between them and the minibatch update over a rollout's records, PPOLearner (csrc/bsx_ppo_head.hip);
                 joint_obs, the input rows of a centralised critic on the team's joint observation, which PPOLearner trains on a
                 PolicyRollout(central_critic=): MAPPO (csrc/bsx_ppo_central.hip)
    adam.py      the fused clip + Adam + pack step that makes a whole update one graph, and its tied form for agents that share one
                 policy per team, and the same step for a network of any width with Polyak target networks kept in the same pass
                 (csrc/bsx_adam_step.hip)
    shuffle.py   a keyed row permutation and the gather of a shuffled minibatch (csrc/bsx_shuffle.hip)
    ddpg.py      the critic join, TD head and action gradient of a DDPG update and DDPGLearner, the MADDPG update of a team from
                 its replay ring as one graph (csrc/bsx_ddpg_head.hip)
    td3.py       what TD3 adds to it: target policy smoothing, the TD head of two critics, and TD3Learner with its delayed actor and
                 target step (csrc/bsx_td3_head.hip)
    sac.py       soft actor-critic on the same ring: the Gaussian policy's reparameterised draw, the soft twin head, the gradients
                 of log_std and of the temperature, and SACLearner (csrc/bsx_sac_head.hip)
    dqn.py       Q-learning for the discrete game on the same ring: the double-Q head, independent or VDN-mixed, and DQNLearner, whose
                 bounded Q network is the very network the rollout plays (csrc/bsx_dqn_head.hip)
    qmix.py      QMIX on the same ring: the monotone mixing head between the Q network and a hypernetwork that is itself a fused MLP, and
                 QMIXLearner -- team values that are no sum of per-plane terms (csrc/bsx_qmix_head.hip)
  render.py      one game's exported state as an RGB image on the host, diagnostic (next row f-4)
There is no CPU fallback: without the HIP library the env cannot be constructed.
"""
from . import advantage, envs, instinct, learner  # noqa: F401
from .advantage import gae  # noqa: F401
from .learner import (TD_STATS, AdamState, DDPGLearner, Minibatch, PPOLearner, adam_step, ddpg_action_grad, ddpg_inputs, ddpg_put_actions, td_head,  # noqa: F401
                      td_head_workspace_bytes, categorical_log_prob, fused_apply, fused_mlp, is_tied, minibatch_gather, mlp_adam_step,  # noqa: F401
                      mlp_adam_step_workspace_bytes, mlp_grad, ppo_head, share_group, shuffle_rows, tie_)
from .learner import TD3_STATS, TD3Learner, td3_head, td3_head_workspace_bytes, td3_smooth_actions  # noqa: F401
from .learner import (SAC_PI_STATS, SAC_STATS, SACLearner, SacHead, SacPolicyGrad, sac_head, sac_head_workspace_bytes, sac_policy_grad,  # noqa: F401
                      sac_policy_grad_workspace_bytes, sac_policy_seed, sac_sample_actions)
from .learner import DQN_STATS, DQNLearner, DqnHead, dqn_head, dqn_head_workspace_bytes  # noqa: F401
from .learner import QMIX_STATS, QMIXLearner, QmixHead, qmix_head, qmix_head_workspace_bytes, qmix_inputs, qmix_members  # noqa: F401
from .learner import joint_obs, joint_width  # noqa: F401
from .envs.battle_env import parallel_env  # noqa: F401
from .replay import NStepAppender, PrioritizedReplayBuffer  # noqa: F401

__all__ = ["AdamState", "DDPGLearner", "Minibatch", "NStepAppender", "PPOLearner", "PrioritizedReplayBuffer", "adam_step", "advantage", "categorical_log_prob", "ddpg_action_grad", "ddpg_inputs", "ddpg_put_actions", "envs", "fused_apply", "fused_mlp", "gae", "instinct", "is_tied", "learner",
           "minibatch_gather", "mlp_adam_step", "mlp_adam_step_workspace_bytes", "mlp_grad", "parallel_env", "ppo_head", "share_group", "shuffle_rows", "TD_STATS",
           "td_head", "td_head_workspace_bytes", "tie_", "TD3Learner", "TD3_STATS", "td3_head", "td3_head_workspace_bytes", "td3_smooth_actions",
           "SACLearner", "SAC_PI_STATS", "SAC_STATS", "SacHead", "SacPolicyGrad", "sac_head", "sac_head_workspace_bytes", "sac_policy_grad",
           "sac_policy_grad_workspace_bytes", "sac_policy_seed", "sac_sample_actions", "DQNLearner", "DQN_STATS", "DqnHead", "dqn_head",
           "dqn_head_workspace_bytes", "QMIXLearner", "QMIX_STATS", "QmixHead", "qmix_head", "qmix_head_workspace_bytes", "qmix_inputs",
           "qmix_members", "joint_obs", "joint_width"]
