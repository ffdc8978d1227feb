"""train.py -- same three lines of logic as the reference (legged_gym/scripts/train.py:40-43).

    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --num_envs 4096
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --recurrent --rnn_hidden_size 256     (an LSTM policy: DESIGN.md 4.10)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --symmetry both --symmetry_coef 1.0   (mirrored minibatches + mirror loss: DESIGN.md 4.11)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --rnd --rnd_weight 0.1                 (an intrinsic reward by random network distillation: DESIGN.md 4.12)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --state_dependent_std --noise_std_type log   (the actor emits sigma per state: DESIGN.md 4.13)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --smooth both --smooth_sigma 0.05           (action-smoothness regularisation, CAPS: DESIGN.md 4.14)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --estimator --estimator_targets lin_vel,base_height   (a concurrent state estimator: DESIGN.md 4.15)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --value_norm popart                    (value normalisation, running or PopArt: DESIGN.md 4.16)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --grad_penalty_coef 0.002              (a Lipschitz gradient penalty on the policy: DESIGN.md 4.17)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --layer_norm                           (Linear -> LayerNorm -> ELU hidden layers: DESIGN.md 4.18)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --reward_groups "track=cmd_diff_lin_vel_x,cmd_diff_lin_vel_y,cmd_diff_ang_vel_yaw;rest=*"   (a critic per reward group: DESIGN.md 4.19)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --cenet --cenet_latent_dim 16 --obs_history 5   (DreamWaQ's context-aided estimator: DESIGN.md 4.21)
    python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --constraints "torque:0.05..0.25,dof_pos:0.25,action_rate:0.25@1.5,upright:1.0@0.7"   (constraints as terminations: DESIGN.md 4.22)
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless
"""
import os

import torch
import torch.distributed as dist

from wiki_grx_gym_amd.envs import *  # noqa: F401,F403  (registers the tasks)
from wiki_grx_gym_amd.utils import get_args, task_registry


def train(args):
    env_cfg = None
    if getattr(args, "reward_groups", None) is not None:   # the group rewards are sums over the step kernel's per-term reward tables
        env_cfg, _ = task_registry.get_cfgs(args.task)
        env_cfg.env.publish_reward_terms = True
    env, env_cfg = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    ppo_runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args)
    ppo_runner.learn(num_learning_iterations=train_cfg.runner.max_iterations, init_at_random_ep_len=True)


if __name__ == "__main__":
    args = get_args()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
        dist.init_process_group("nccl" if args.sim_device_type == "cuda" else "gloo")
    train(args)
