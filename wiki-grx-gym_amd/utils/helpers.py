"""CLI flags, seeding, checkpoint lookup, policy export -- the surface of the reference's
legged_gym/utils/helpers.py (get_args HP:159-185 incl. the gymutil flags GU:298-370, set_seed
HP:70-80, get_load_path HP:108-130, update_cfg_from_args HP:133-156, export_policy_as_jit HP:188-201)
without any isaacgym import."""
import argparse
import copy
import os
import random

import numpy as np
import torch

from ..envs.config import class_to_dict  # noqa: F401  (re-exported like the reference)


def set_seed(seed):
    if seed == -1:
        seed = np.random.randint(0, 10000)
    print("Setting seed: {}".format(seed))
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def parse_device_str(device_str):
    """gymutil.parse_device_str: 'cuda:1' -> ('cuda', 1); 'cpu' -> ('cpu', 0)"""
    parts = device_str.split(":")
    kind = parts[0].lower()
    if kind not in ("cpu", "cuda", "gpu"):
        raise ValueError(f'Invalid device string "{device_str}"')
    return ("cuda" if kind == "gpu" else kind), (int(parts[1]) if len(parts) > 1 else 0)


def get_args(argv=None):
    p = argparse.ArgumentParser(description="RL Policy")
    p.add_argument("--task", type=str, default="GR1T1", help="Registered task name (GR1T1, GR1T2)")
    p.add_argument("--resume", action="store_true", default=False, help="Resume training from a checkpoint")
    p.add_argument("--experiment_name", type=str, help="Name of the experiment to run or load. Overrides config file if provided.")
    p.add_argument("--run_name", type=str, help="Name of the run. Overrides config file if provided.")
    p.add_argument("--load_run", type=str, help="Name of the run to load when resume=True. If -1: will load the last run.")
    p.add_argument("--checkpoint", type=int, help="Saved model checkpoint number. If -1: will load the last checkpoint.")
    p.add_argument("--headless", action="store_true", default=False, help="Force display off at all times")
    p.add_argument("--horovod", action="store_true", default=False, help="(unused in the reference too, HP:169)")
    p.add_argument("--rl_device", type=str, default="cuda:0", help="Device used by the RL algorithm")
    p.add_argument("--num_envs", type=int, help="Number of environments to create. Overrides config file if provided.")
    p.add_argument("--seed", type=int, help="Random seed. Overrides config file if provided.")
    p.add_argument("--max_iterations", type=int, help="Maximum number of training iterations.")
    # gymutil.parse_arguments flags (GU:305-315)
    p.add_argument("--sim_device", type=str, default="cuda:0", help="Physics Device in PyTorch-like syntax")
    p.add_argument("--pipeline", type=str, default="gpu", help="Tensor API pipeline (cpu/gpu)")
    p.add_argument("--graphics_device_id", type=int, default=0)
    p.add_argument("--num_threads", type=int, default=0, help="accepted for compatibility (PhysX CPU threads)")
    p.add_argument("--subscenes", type=int, default=0, help="accepted for compatibility")
    p.add_argument("--slices", type=int)
    p.add_argument("--terrain", type=str, choices=["plane", "heightfield", "trimesh"], help="override cfg.terrain.mesh_type")
    p.add_argument("--precision", type=str, choices=["fp32", "bf16"],
                   help="PPO's hidden-layer matrix products: fp32 (default) or bf16 operands with fp32 accumulation (HIP only)")
    p.add_argument("--exact_resume", action="store_true", default=False,
                   help="Every checkpoint also saves the whole training state (train_state_<it>.pt); with --resume, continue from it bit for bit")
    p.add_argument("--empirical_normalization", action="store_true", default=False,
                   help="Normalise actor and critic observations with their running mean / variance (saved in the checkpoint; play needs the same flag)")
    p.add_argument("--obs_history", type=int, default=1,
                   help="The policy sees the last N observation frames, oldest first (1: off; saved in the checkpoint; play needs the same value)")
    p.add_argument("--critic_obs_history", type=int, default=1,
                   help="The critic sees the last N privileged observation frames (1: off; needs an env with privileged observations)")
    p.add_argument("--privileged_actor", action="store_true", default=False,
                   help="The actor reads the critic's input (privileged observations, --critic_obs_history): a teacher for --distill_from")
    p.add_argument("--distill_from", type=str,
                   help="Path of a PPO checkpoint: distil its actor into a student on the actor's observations (--obs_history) instead of running PPO")
    p.add_argument("--distill_loss", type=str, choices=["mse", "huber"], help="Behaviour loss of --distill_from (default mse)")
    p.add_argument("--distill_noise_std", type=float, help="Fixed action noise of the student's rollout under --distill_from (default 0.1)")
    p.add_argument("--student_recurrent", action="store_true", default=False,
                   help="With --distill_from: the student is an LSTM (--rnn_hidden_size) in front of its MLP, trained by truncated BPTT; "
                        "play the checkpoint with --recurrent --rnn_hidden_size H")
    p.add_argument("--distill_gradient_length", type=int,
                   help="Steps per truncated-BPTT window of --student_recurrent (default 15; 0: the whole rollout in one window)")
    p.add_argument("--recurrent", action="store_true", default=False,
                   help="A recurrent policy: an LSTM in front of the actor's and the critic's MLP (saved in the checkpoint; play needs the same flag)")
    p.add_argument("--rnn_hidden_size", type=int, default=256, help="Hidden size of --recurrent's LSTMs: a multiple of 32 in 32..1024")
    p.add_argument("--symmetry", type=str, choices=["augment", "loss", "both"],
                   help="Left-right symmetry in PPO's update: mirrored minibatches (augment), a mirror loss (loss) or both; nothing is saved")
    p.add_argument("--symmetry_coef", type=float, default=1.0, help="Weight of --symmetry's mirror loss (loss / both; default 1.0)")
    p.add_argument("--smooth", type=str, choices=["temporal", "spatial", "both"],
                   help="Action-smoothness regularisation (CAPS) in PPO's update: the mean action at s_t close to the one at s_t+1 (temporal), "
                        "to the one at s_t + sigma * noise (spatial), or both; nothing is saved")
    p.add_argument("--smooth_temporal_coef", type=float, default=0.1, help="Weight of --smooth's temporal term (default 0.1, not tuned)")
    p.add_argument("--smooth_spatial_coef", type=float, default=0.1, help="Weight of --smooth's spatial term (default 0.1, not tuned)")
    p.add_argument("--smooth_sigma", type=float, default=0.05,
                   help="Standard deviation of --smooth's perturbation of the actor's (stacked, normalised) input (default 0.05, not tuned)")
    p.add_argument("--grad_penalty_coef", type=float,
                   help="Lipschitz gradient penalty (Chen et al., 2024) in PPO's update: this weight times the batch mean of "
                        "||d log pi(a|s) / d s||^2 joins the loss (a float > 0; the paper uses 0.002, not tuned here); nothing is saved")
    p.add_argument("--value_norm", type=str, choices=["running", "popart"],
                   help="Value normalisation: the critic learns returns normalised by their running mean / std (running), and its output "
                        "layer is rescaled when the statistics move, so that its predictions are preserved (popart); saved in the checkpoint, "
                        "--resume needs the same value")
    p.add_argument("--rnd", action="store_true", default=False,
                   help="Random network distillation: an intrinsic reward (predictor error against a fixed random network) added to the env's")
    p.add_argument("--rnd_weight", type=float, default=0.1, help="Weight of --rnd's intrinsic reward (default 0.1, not tuned)")
    p.add_argument("--rnd_weight_schedule", type=str, choices=["constant", "linear", "step"], default="constant",
                   help="--rnd_weight over the PPO iterations: constant, linear (--rnd_final_weight from --rnd_start_it to --rnd_end_it) or "
                        "step (--rnd_final_weight from --rnd_at_it on)")
    p.add_argument("--rnd_final_weight", type=float, help="The weight a linear / step schedule ends at (default: --rnd_weight)")
    p.add_argument("--rnd_start_it", type=int, default=0, help="First iteration of a linear schedule's ramp")
    p.add_argument("--rnd_end_it", type=int, default=0, help="Last iteration of a linear schedule's ramp")
    p.add_argument("--rnd_at_it", type=int, default=0, help="Iteration at which a step schedule switches")
    p.add_argument("--rnd_state", type=str, choices=["privileged", "obs"], default="privileged",
                   help="The frame --rnd's networks read: the env's privileged frame (no observation noise) or the actor's raw frame")
    p.add_argument("--rnd_num_outputs", type=int, default=32, help="Width of --rnd's embedding (1..256)")
    p.add_argument("--rnd_learning_rate", type=float, default=1e-3, help="Learning rate of --rnd's predictor (fixed)")
    p.add_argument("--estimator", action="store_true", default=False,
                   help="A concurrently trained state estimator: a small network regresses privileged quantities from the actor's input and "
                        "its output is appended to that input (saved in the checkpoint; play needs the same flag, targets and hidden dims)")
    p.add_argument("--estimator_targets", type=str, default="lin_vel",
                   help="What --estimator regresses: a comma-separated subset of lin_vel (3 columns), base_height (1), feet_contact (2), "
                        "feet_height (2) (default lin_vel, not tuned)")
    p.add_argument("--estimator_hidden_dims", type=int, nargs="+", default=[128, 64],
                   help="Hidden layers of --estimator's network: 1 to 3 widths of 1..256 (default 128 64, not tuned)")
    p.add_argument("--estimator_learning_rate", type=float, default=1e-3, help="Learning rate of --estimator's network (fixed; default 1e-3, not tuned)")
    p.add_argument("--estimator_num_epochs", type=int, default=1,
                   help="Passes of --estimator's regression over a rollout, in PPO's num_mini_batches minibatches (default 1, not tuned)")
    p.add_argument("--cenet", action="store_true", default=False,
                   help="A context-aided estimator network (DreamWaQ's CENet): an encoder regresses privileged quantities from the actor's input "
                        "AND emits a stochastic latent from which a decoder predicts the next frame; [estimate | latent] is appended to the "
                        "actor's input (saved in the checkpoint; play needs the same flag, targets, latent and hidden dims)")
    p.add_argument("--cenet_targets", type=str, default="lin_vel",
                   help="What --cenet's encoder regresses: --estimator_targets' names (default lin_vel, not tuned)")
    p.add_argument("--cenet_latent_dim", type=int, default=16, help="Width of --cenet's latent z: 1..64 (default 16, not tuned)")
    p.add_argument("--cenet_beta", type=float, default=1.0, help="Weight of --cenet's KL term (default 1.0, not tuned)")
    p.add_argument("--cenet_encoder_dims", type=int, nargs="+", default=[128, 64],
                   help="Hidden layers of --cenet's encoder: 1 to 3 widths of 1..1024 (default 128 64, not tuned)")
    p.add_argument("--cenet_decoder_dims", type=int, nargs="+", default=[64, 128],
                   help="Hidden layers of --cenet's decoder: 1 to 3 widths of 1..1024 (default 64 128, not tuned)")
    p.add_argument("--cenet_learning_rate", type=float, default=1e-3, help="Learning rate of --cenet's networks (fixed; default 1e-3, not tuned)")
    p.add_argument("--cenet_num_epochs", type=int, default=1,
                   help="Passes of --cenet's update over a rollout, in PPO's num_mini_batches minibatches (default 1, not tuned)")
    p.add_argument("--noise_std_type", type=str, choices=["scalar", "log"],
                   help="The action noise's parameter: std itself (scalar, default) or log_std with sigma = exp(log_std), which cannot reach "
                        "zero (saved in the checkpoint; play needs the same value)")
    p.add_argument("--state_dependent_std", action="store_true", default=False,
                   help="The actor emits its own sigma per state: its output layer is [mean | s], sigma = s (scalar) or exp(s) (log; "
                        "recommended).  Saved in the checkpoint; play needs the same flag")
    p.add_argument("--layer_norm", action="store_true", default=False,
                   help="Layer normalisation in the actor's and the critic's hidden layers: Linear -> LayerNorm -> ELU (needs the elu "
                        "activation).  Saved in the checkpoint; --resume and play need the same flag")
    p.add_argument("--reward_groups", type=str,
                   help="Multi-critic PPO: `name=term,term,...;name=...` splits the task's active reward terms into 1..8 groups (`*` in one "
                        "group: every term not named elsewhere); the critic gets a value head per group, GAE and the advantage "
                        "normalisation run per group.  Saved in the checkpoint; --resume needs the same spec")
    p.add_argument("--reward_group_weights", type=str,
                   help="Weights `w1,...,wK` of --reward_groups' normalised group advantages in their sum (default all 1.0, not tuned)")
    p.add_argument("--constraints", type=str,
                   help="Constraints as terminations (CaT): `family:p[@L],...` with the families torque, dof_vel, dof_pos, action_rate@L, "
                        "upright@L; p is the family's maximum termination probability, one number in [0, 1] or `p_lo..p_hi` ramped over "
                        "--constraint_ramp_its iterations.  A violation scales the reward and the discount inside GAE.  Saved in the "
                        "checkpoint; --resume needs the same spec")
    p.add_argument("--constraint_tau", type=float, default=0.95,
                   help="Decay of --constraints' running column maxima, in [0, 1) (default 0.95, the paper's)")
    p.add_argument("--constraint_ramp_its", type=int, default=1000,
                   help="Iterations over which --constraints' `p_lo..p_hi` probabilities ramp, >= 1 (default 1000, not tuned)")
    p.add_argument("--constraint_reward_clip", type=str, choices=["zero", "none"], default="zero",
                   help="Under --constraints the stored reward is (1 - delta) max(r, 0) (zero, default: ending early never pays) or "
                        "(1 - delta) r (none)")
    p.add_argument("--action_dist", type=str, choices=["gaussian", "beta"],
                   help="The policy's action distribution: a Gaussian (default) or a Beta on the env's action box "
                        "(normalization.clip_actions_min / clip_actions_max), which cannot sample outside it.  Saved in the checkpoint; "
                        "--resume and play need the same value")
    p.add_argument("--action_bounds", type=float, nargs=2, metavar=("LO", "HI"),
                   help="The action box of --action_dist beta for a task whose config has only the scalar clip_actions (the same for every joint)")
    args = p.parse_args(argv)
    if args.obs_history < 1 or args.critic_obs_history < 1:
        raise ValueError(f"--obs_history and --critic_obs_history must be >= 1, got {args.obs_history} and {args.critic_obs_history}")
    args.sim_device_type, args.compute_device_id = parse_device_str(args.sim_device)
    args.use_gpu_pipeline = args.pipeline.lower() in ("gpu", "cuda")
    args.use_gpu = args.sim_device_type == "cuda"
    args.physics_engine = "SIM_HIP"          # the reference passes gymapi.SIM_PHYSX
    args.sim_device_id = args.compute_device_id
    args.sim_device = args.sim_device_type + (f":{args.sim_device_id}" if args.sim_device_type == "cuda" else "")
    if "LOCAL_RANK" in os.environ and args.sim_device_type == "cuda":   # torchrun: one process per GPU
        lr = int(os.environ["LOCAL_RANK"])
        args.sim_device = args.rl_device = f"cuda:{lr}"
        args.sim_device_id = lr
    return args


def update_cfg_from_args(env_cfg, cfg_train, args):
    if env_cfg is not None:
        if args.num_envs is not None:
            env_cfg.env.num_envs = args.num_envs
        if getattr(args, "terrain", None):
            env_cfg.terrain.mesh_type = args.terrain
    if cfg_train is not None:
        if args.seed is not None:
            cfg_train.seed = args.seed
        if args.max_iterations is not None:
            cfg_train.runner.max_iterations = args.max_iterations
        if args.resume:
            cfg_train.runner.resume = args.resume
        for name in ("experiment_name", "run_name", "load_run", "checkpoint"):
            if getattr(args, name) is not None:
                setattr(cfg_train.runner, name, getattr(args, name))
        if getattr(args, "precision", None) is not None:   # (only when given: the algorithm config has no such key otherwise)
            cfg_train.algorithm.precision = args.precision
        if getattr(args, "exact_resume", False):   # (likewise: the runner config has no such key otherwise)
            cfg_train.runner.exact_resume = True
        if getattr(args, "empirical_normalization", False):   # (likewise)
            cfg_train.runner.empirical_normalization = True
        if getattr(args, "obs_history", 1) != 1:   # (likewise)
            cfg_train.runner.obs_history_length = int(args.obs_history)
        if getattr(args, "critic_obs_history", 1) != 1:   # (likewise)
            cfg_train.runner.critic_obs_history_length = int(args.critic_obs_history)
        if getattr(args, "privileged_actor", False):   # (likewise)
            cfg_train.runner.privileged_actor = True
        if getattr(args, "distill_from", None) is not None:   # (likewise)
            cfg_train.runner.distill_from = args.distill_from
        if getattr(args, "distill_loss", None) is not None:   # (likewise)
            cfg_train.runner.distill_loss = args.distill_loss
        if getattr(args, "distill_noise_std", None) is not None:   # (likewise)
            cfg_train.runner.distill_noise_std = float(args.distill_noise_std)
        if getattr(args, "student_recurrent", False):   # (likewise; --rnn_hidden_size travels with it as with --recurrent)
            cfg_train.runner.student_recurrent = True
            cfg_train.runner.student_rnn_hidden_size = int(getattr(args, "rnn_hidden_size", 256))
        if getattr(args, "distill_gradient_length", None) is not None:   # (likewise; refused by the runner without --student_recurrent)
            cfg_train.runner.distill_gradient_length = int(args.distill_gradient_length)
        if getattr(args, "symmetry", None) is not None:   # (likewise: the algorithm config has no such keys otherwise)
            cfg_train.algorithm.symmetry = args.symmetry
            cfg_train.algorithm.symmetry_coef = float(getattr(args, "symmetry_coef", 1.0))
        if getattr(args, "smooth", None) is not None:   # (likewise; the --smooth_* values travel only with --smooth)
            a = cfg_train.algorithm
            a.smooth = args.smooth
            a.smooth_temporal_coef = float(getattr(args, "smooth_temporal_coef", 0.1))
            a.smooth_spatial_coef = float(getattr(args, "smooth_spatial_coef", 0.1))
            a.smooth_sigma = float(getattr(args, "smooth_sigma", 0.05))
        if getattr(args, "grad_penalty_coef", None) is not None:   # (likewise)
            cfg_train.algorithm.grad_penalty_coef = float(args.grad_penalty_coef)
        if getattr(args, "value_norm", None) is not None:   # (likewise)
            cfg_train.algorithm.value_norm = args.value_norm
        if getattr(args, "rnd", False):   # (likewise; the --rnd_* values travel only with --rnd)
            a = cfg_train.algorithm
            a.rnd = True
            a.rnd_weight, a.rnd_weight_schedule = float(getattr(args, "rnd_weight", 0.1)), getattr(args, "rnd_weight_schedule", "constant")
            fw = getattr(args, "rnd_final_weight", None)
            a.rnd_final_weight = None if fw is None else float(fw)
            a.rnd_start_it, a.rnd_end_it, a.rnd_at_it = (int(getattr(args, k, 0)) for k in ("rnd_start_it", "rnd_end_it", "rnd_at_it"))
            a.rnd_state, a.rnd_num_outputs = getattr(args, "rnd_state", "privileged"), int(getattr(args, "rnd_num_outputs", 32))
            a.rnd_learning_rate = float(getattr(args, "rnd_learning_rate", 1e-3))
        if getattr(args, "estimator", False):   # (likewise; the --estimator_* values travel only with --estimator)
            r = cfg_train.runner
            r.estimator = True
            r.estimator_targets = getattr(args, "estimator_targets", "lin_vel")
            r.estimator_hidden_dims = [int(h) for h in getattr(args, "estimator_hidden_dims", [128, 64])]
            r.estimator_learning_rate = float(getattr(args, "estimator_learning_rate", 1e-3))
            r.estimator_num_epochs = int(getattr(args, "estimator_num_epochs", 1))
        if getattr(args, "cenet", False):   # (likewise; the --cenet_* values travel only with --cenet)
            r = cfg_train.runner
            r.cenet = True
            r.cenet_targets = getattr(args, "cenet_targets", "lin_vel")
            r.cenet_latent_dim = int(getattr(args, "cenet_latent_dim", 16))
            r.cenet_beta = float(getattr(args, "cenet_beta", 1.0))
            r.cenet_encoder_dims = [int(h) for h in getattr(args, "cenet_encoder_dims", [128, 64])]
            r.cenet_decoder_dims = [int(h) for h in getattr(args, "cenet_decoder_dims", [64, 128])]
            r.cenet_learning_rate = float(getattr(args, "cenet_learning_rate", 1e-3))
            r.cenet_num_epochs = int(getattr(args, "cenet_num_epochs", 1))
        if getattr(args, "recurrent", False):   # (likewise: the policy config has no rnn_hidden_size otherwise)
            cfg_train.runner.policy_class_name = "ActorCriticRecurrent"
            cfg_train.policy.rnn_hidden_size = int(getattr(args, "rnn_hidden_size", 256))
        if getattr(args, "noise_std_type", None) is not None:   # (likewise: the policy config has no such keys otherwise)
            cfg_train.policy.noise_std_type = args.noise_std_type
        if getattr(args, "state_dependent_std", False):   # (likewise)
            cfg_train.policy.state_dependent_std = True
        if getattr(args, "layer_norm", False):   # (likewise)
            cfg_train.policy.layer_norm = True
        if getattr(args, "reward_groups", None) is not None:   # (likewise; the weights travel only with --reward_groups)
            cfg_train.algorithm.reward_groups = args.reward_groups
            if getattr(args, "reward_group_weights", None) is not None:
                cfg_train.algorithm.reward_group_weights = args.reward_group_weights
        if getattr(args, "constraints", None) is not None:   # (likewise; the --constraint_* values travel only with --constraints)
            a = cfg_train.algorithm
            a.constraints = args.constraints
            a.constraint_tau = float(getattr(args, "constraint_tau", 0.95))
            a.constraint_ramp_its = int(getattr(args, "constraint_ramp_its", 1000))
            a.constraint_reward_clip = getattr(args, "constraint_reward_clip", "zero")
        if getattr(args, "action_dist", None) is not None:   # (likewise: the policy config has no such keys otherwise)
            cfg_train.policy.action_dist = args.action_dist
        if getattr(args, "action_bounds", None) is not None:   # (likewise)
            cfg_train.policy.action_bounds = [float(args.action_bounds[0]), float(args.action_bounds[1])]
    return env_cfg, cfg_train


def parse_sim_params(args, cfg):
    """HP:83-105 returns a gymapi.SimParams; here a plain namespace with the same field names."""
    sim = dict(cfg.get("sim", {}))
    ns = argparse.Namespace(**{k: v for k, v in sim.items() if not isinstance(v, dict)})
    ns.use_gpu_pipeline = args.use_gpu_pipeline
    ns.physx = argparse.Namespace(**sim.get("physx", {}))
    ns.physx.use_gpu = args.use_gpu
    if getattr(args, "num_threads", 0) > 0:
        ns.physx.num_threads = args.num_threads
    return ns


def get_load_path(root, load_run=-1, checkpoint=-1):
    try:
        runs = sorted(os.listdir(root))
        if "exported" in runs:
            runs.remove("exported")
        last_run = os.path.join(root, runs[-1])
    except Exception:
        raise ValueError("No runs in this directory: " + root)
    load_run = last_run if load_run == -1 else os.path.join(root, load_run)
    if checkpoint == -1:
        models = [f for f in os.listdir(load_run) if "model" in f]
        models.sort(key=lambda m: "{0:0>15}".format(m))
        model = models[-1]
    else:
        model = "model_{}.pt".format(checkpoint)
    return os.path.join(load_run, model)


def export_policy_as_jit(actor_critic, path, normalizer=None, history=1, estimator=None, cenet=None):
    """A recurrent actor_critic (rl.recurrent.ActorCriticRecurrent): the exported module is an nn.LSTM with its state in buffers in front
    of the actor's layers (rl.recurrent.ExportedRecurrentPolicy: one raw frame per call, `reset_memory()` and `reset(dones)` exported).
    `normalizer` (an rl.normalizer.EmpiricalNormalization): the exported module takes RAW observations and normalises them itself.
    `history` > 1 (the runner's obs_history_length): it takes raw SINGLE frames and keeps the last `history` of them itself
    (rl.history.HistoryPolicy: `reset_memory()` and `reset(dones)` are exported methods).
    An actor_critic with `state_dependent_std`: the exported module returns the mean, the first A of the actor's 2A outputs.
    An actor_critic with `action_dist="beta"`: the exported module returns the Beta's mean in action units, lo + span * alpha / (alpha + beta),
    with lo / span as its own buffers (rl.beta.BetaMeanHead).
    `estimator` (the network of an rl.estimator.StateEstimator): behind history and normaliser the module appends the estimate to the
    actor's input itself (rl.estimator.EstimatorPolicy); a consumer still feeds raw single frames.
    `cenet` (an rl.cenet.CENet): likewise with [v_hat | mu] of its encoder, z = mu (rl.cenet.CENetPolicy); the decoder is not exported"""
    os.makedirs(path, exist_ok=True)
    path = os.path.join(path, "policy_jit.pt")
    if getattr(actor_critic, "is_recurrent", False):
        from ..rl.recurrent import ExportedRecurrentPolicy
        torch.jit.script(ExportedRecurrentPolicy(actor_critic, normalizer)).save(path)
        return path
    # (state_dependent_std: the actor's output layer is [mean | s]; the exported module slices, a consumer sees [B, A] as ever)
    inner = actor_critic.inference_actor() if hasattr(actor_critic, "inference_actor") else actor_critic.actor
    model = copy.deepcopy(inner).to("cpu")
    appended = 0
    if estimator is not None:
        from ..rl.estimator import EstimatorPolicy
        model = EstimatorPolicy(model, copy.deepcopy(estimator).to("cpu"))
        appended = estimator.output_size
    if cenet is not None:
        from ..rl.cenet import CENetPolicy
        model = CENetPolicy(model, copy.deepcopy(cenet.encoder).to("cpu"), cenet.num_outputs)
        appended = cenet.num_outputs
    if normalizer is not None:
        from ..rl.normalizer import NormalizedPolicy
        model = NormalizedPolicy(model, copy.deepcopy(normalizer).to("cpu"))
    if history > 1:
        from ..rl.history import HistoryPolicy
        stacked = actor_critic.actor.model[0].in_features - appended
        if stacked % history:
            raise ValueError(f"export_policy_as_jit: the actor takes {stacked} inputs, no multiple of history={history}")
        model = HistoryPolicy(model, stacked // history, history)
    torch.jit.script(model).save(path)
    return path
