"""The learner's side of a PolicyRollout and of a DeviceReplayBuffer, on device: one module per kernel family, each with its own catalogue.

  mlp.py      the actor / value / Q MLP as ONE fused forward and ONE fused backward, its cached buffers and its one check (csrc/bsx_actor_grad.hip)
  adam.py     clip + Adam + pack as two launches: the actors' step, its tied form, the free-width form with Polyak targets (csrc/bsx_adam_step.hip)
  shuffle.py  a keyed row permutation and the gather of a shuffled minibatch (csrc/bsx_shuffle.hip)
  ppo.py      the PPO loss head and PPOLearner, the update of a rollout's two networks (csrc/bsx_ppo_head.hip); joint_obs, the input rows of
              a centralised critic (MAPPO: csrc/bsx_ppo_central.hip), which PPOLearner trains on a PolicyRollout(central_critic=)
  ddpg.py     the critic join, TD head and action gradient, and DDPGLearner, the MADDPG update of a team from its ring (csrc/bsx_ddpg_head.hip)
  td3.py      target policy smoothing, the TD head of two critics, the second critic TD3Learner and SACLearner share, and TD3Learner: twin critics,
              a delayed actor and target step (csrc/bsx_td3_head.hip)
  sac.py      the Gaussian policy's reparameterised draw, the soft twin head, the policy's seeds and gradients, and SACLearner (csrc/bsx_sac_head.hip)
  dqn.py      Q-learning for the discrete game: the double-Q head, independent or VDN-mixed, and DQNLearner, whose Q network is the network
              the rollout plays (csrc/bsx_dqn_head.hip)
  qmix.py     QMIX for the discrete game: the monotone mixing head between the Q network and a hypernetwork the fused MLP kernels already take,
              and QMIXLearner (csrc/bsx_qmix_head.hip)
              (both learn from what a PolicyRollout(epsilon=...) plays: annealed epsilon-greedy is the rollout's, rollout.EpsilonSchedule)
  _common.py  what more than one of them uses: the hyper-parameter ranges, the stream, the capture of an update as one graph

A PPO minibatch:  [minibatch_gather] -> bsx_actor_forward with the value head -> ppo_head -> bsx_mlp_grad of the actor, of the critic -> adam_step.
  central critic: [minibatch_gather] -> bsx_actor_forward, no value head -> joint_obs -> bsx_mlp_forward of the critic (raw = v) -> ppo_head ->
                  bsx_mlp_grad of the actor on obs, of the critic on the joined rows -> adam_step of the actor, mlp_adam_step of the critic.
A DDPG update:    buffer.sample -> ddpg_inputs -> target actor, ddpg_put_actions -> target critic, critic -> td_head -> bsx_mlp_grad, mlp_adam_step of the
                  critic -> actor, ddpg_put_actions -> bsx_mlp_grad of the critic for grad_x, ddpg_action_grad -> bsx_mlp_grad, mlp_adam_step of the actor.
A TD3 update:     as DDPG's, with td3_smooth_actions in place of the first ddpg_put_actions, both target critics and both critics -> td3_head ->
                  bsx_mlp_grad of each critic, ONE mlp_adam_step of both; the actor's half, and every Polyak target, once per policy_delay updates.
A SAC update:     as TD3's without its delay, the CURRENT actor and sac_sample_actions in place of the target actor and td3_smooth_actions (a' ~ pi
                  with logp'), both target critics and both critics -> sac_head -> bsx_mlp_grad of each critic, ONE mlp_adam_step of both with their
                  targets -> actor, sac_sample_actions (a ~ pi with logp, z) -> both stepped critics, sac_policy_seed -> bsx_mlp_grad of each critic
                  for grad_x -> sac_policy_grad (g_a4, g_log_std, log_alpha's step) -> bsx_mlp_grad, mlp_adam_step of the actor with log_std.
A DQN update:     buffer.sample -> the online network on obs, [on obs_next: double Q], the target network on obs_next -> dqn_head (the replayed
                  and the greedy next action by the step kernel's argmax4, independent or VDN) -> bsx_mlp_grad(squash) -> ONE mlp_adam_step with
                  the Polyak target.  Q_i(o, a) = q_scale * tanh row: what the learner calls greedy is what a published rollout plays.
A QMIX update:    buffer.sample -> the three forwards of a DQN update -> qmix_inputs -> the mixer on x_cur, the target mixer on x_next (their tanh
                  rows are the mix's weights) -> qmix_head (Q_tot = the monotone mix of the replayed actions' values, its double-Q target, g4 and
                  gh) -> bsx_mlp_grad(squash) of the Q network, of the mixer -> mlp_adam_step of each with its Polyak target.
n-step targets:   the off-policy updates are unchanged on a ring filled through replay.NStepAppender (rows whose reward is the folded
                  n-step sum and whose obs_next lies up to n ticks on): the learner wants gamma=app.bootstrap_gamma, the appender's gamma^n.
                  SAC's target then carries the entropy term at the bootstrap state only.
"""
from . import adam, ddpg, mlp
from .adam import (ADAM_STATS, HYPER, AdamState, adam_hyper, adam_step, adam_step_workspace_bytes, is_tied, mlp_adam_step,  # noqa: F401
                   mlp_adam_step_workspace_bytes, share_group, tie_)
from .ddpg import MAX_OBS, TD_STATS, DDPGLearner, TdHead, ddpg_action_grad, ddpg_inputs, ddpg_put_actions, td_head, td_head_workspace_bytes  # noqa: F401
from .mlp import H, PARAMS, blob_floats, categorical_log_prob, fused_apply, fused_grad, fused_mlp, grad_floats, mlp_grad, split_grad  # noqa: F401
from .ppo import KINDS, STATS, PPOLearner, PpoHead, joint_obs, joint_width, ppo_head, ppo_head_workspace_bytes  # noqa: F401
from .td3 import TD3_STATS, TD3Learner, Td3Head, td3_head, td3_head_workspace_bytes, td3_smooth_actions  # noqa: F401
from .sac import (SAC_PI_STATS, SAC_STATS, SACLearner, SacHead, SacPolicyGrad, sac_head, sac_head_workspace_bytes, sac_policy_grad,  # noqa: F401
                  sac_policy_grad_workspace_bytes, sac_policy_seed, sac_sample_actions)
from .dqn import DQN_STATS, DQNLearner, DqnHead, dqn_head, dqn_head_workspace_bytes  # noqa: F401
from .qmix import QMIX_STATS, QMIXLearner, QmixHead, qmix_head, qmix_head_workspace_bytes, qmix_inputs, qmix_members  # noqa: F401
from .shuffle import GATHER_ROWS, Minibatch, minibatch_gather, shuffle_rows  # noqa: F401

_Buffers, _buffers, _actor_forward, _mlp_forward, _mlp_grad, _tied_tensors, _critic_width = (  # used by tests/ and tools/
    mlp._Buffers, mlp._buffers, mlp._actor_forward, mlp._mlp_forward, mlp._mlp_grad, adam._tied_tensors, ddpg._critic_width)
