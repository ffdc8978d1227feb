"""On-policy runner with the rsl_rl surface (reference: rsl_rl/runners/on_policy_runner.py:16-345):
``OnPolicyRunner(env, train_cfg_dict, log_dir, device)``, ``learn(num_learning_iterations,
init_at_random_ep_len)``, ``save/load`` with the reference's checkpoint dict keys
(``model_state_dict, optimizer_state_dict, iter, infos``), ``get_inference_policy``, the same
TensorBoard scalar names (Episode/*, Loss/*, Perf/*, Train/*, Policy/*).

Differences, all on the host side: the per-step reward/length bookkeeping stays on the device
(the reference does nonzero() + .cpu() every step, on_policy_runner.py:177-179) and is read back
once per iteration; TensorBoard is optional (a JSON-lines scalar log is always written); with
torch.distributed initialised only rank 0 logs and saves."""
import json
import os
import random
import statistics
import time
from collections import deque

import torch
import torch.distributed as dist

from .distillation import Distillation, StudentTeacher, read_teacher
from .history import HistoryPolicy, ObsHistory
from .modules import ActorCriticMLP
from .normalizer import EmpiricalNormalization, NormalizedPolicy, normalize_step
from .ppo import PPO
from .recurrent import ActorCriticRecurrent, RecurrentPolicy
from .storage import RolloutStorage  # noqa: F401

_POLICIES = {"ActorCriticMLP": ActorCriticMLP, "ActorCritic": ActorCriticMLP, "ActorCriticRecurrent": ActorCriticRecurrent}
_ALGORITHMS = {"PPO": PPO, "Distillation": Distillation}


class _ScalarLog:
    """SummaryWriter when tensorboard is importable, always a scalars.jsonl next to it."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self._f = open(os.path.join(log_dir, "scalars.jsonl"), "a")
        try:
            from torch.utils.tensorboard import SummaryWriter
            self._tb = SummaryWriter(log_dir=log_dir, flush_secs=10)
        except Exception:
            self._tb = None

    def add_scalar(self, tag, value, step):
        value = float(value)
        self._f.write(json.dumps({"tag": tag, "value": value, "step": step}) + "\n")
        self._f.flush()
        if self._tb is not None:
            self._tb.add_scalar(tag, value, step)


class OnPolicyRunner:
    def __init__(self, env, train_cfg, log_dir=None, device="cpu"):
        self.cfg, self.algorithm_cfg, self.policy_cfg = train_cfg["runner"], train_cfg["algorithm"], train_cfg["policy"]
        self.device, self.env = device, env
        policy_cls = _POLICIES[self.cfg["policy_class_name"]]
        if dist.is_available() and dist.is_initialized():
            torch.manual_seed(int(train_cfg.get("seed", 1)))      # identical replicas on every rank
        # observation history: the policy sees the last H frames (the critic the last Hc privileged frames), stacked oldest
        # first; everything after the stacking -- normaliser, storage, update -- is the same code on a wider tensor.  Not config keys either
        # (`--obs_history` / `--critic_obs_history` or an assignment to train_cfg.runner sets them); 1 / 1 builds nothing
        self.obs_history_length = int(self.cfg.get("obs_history_length", 1))
        self.critic_obs_history_length = int(self.cfg.get("critic_obs_history_length", 1))
        if self.obs_history_length < 1 or self.critic_obs_history_length < 1:
            raise ValueError(f"obs_history_length and critic_obs_history_length must be >= 1, got {self.obs_history_length} and "
                             f"{self.critic_obs_history_length}")
        if env.num_pri_obs is None and self.critic_obs_history_length != 1:
            raise ValueError(f"critic_obs_history_length={self.critic_obs_history_length}: this env has no privileged observations, the critic gets "
                             "the actor's stacked input (set obs_history_length)")
        # a privileged actor and distillation.  privileged_actor: the actor reads the tensor the critic gets (a teacher that
        # can be trained).  distill_from: a student on the actor stream is regressed on the frozen actor of that checkpoint, whose stream travels
        # in the critic's slot.  Not config keys either (`--privileged_actor` / `--distill_from` or an assignment to train_cfg.runner sets them)
        self.privileged_actor = bool(self.cfg.get("privileged_actor", False))
        self.distill_from = self.cfg.get("distill_from") or None
        self.distillation = None   # the "distillation" entry of a checkpoint of this run
        self._alt_inputs = None    # what builds (actor input, critic-slot input) from one step's raw frames in these two modes
        if self.privileged_actor:
            self._check_privileged_actor(env)
        # a recurrent distillation student: an LSTM in front of the student's MLP, trained by truncated BPTT.  Not config keys
        # either (`--student_recurrent` / `--rnn_hidden_size` / `--distill_gradient_length` or assignments to train_cfg.runner set them)
        self.student_recurrent = bool(self.cfg.get("student_recurrent", False))
        if self.student_recurrent:
            self._check_student_recurrent()
        elif self.cfg.get("distill_gradient_length") is not None:
            raise ValueError("--distill_gradient_length without --student_recurrent: the window of truncated back-propagation through time "
                             "belongs to a recurrent student (pass --student_recurrent with --distill_from)")
        # a recurrent policy: an LSTM in front of the actor's and the critic's MLP.  Not config keys either (`--recurrent` /
        # `--rnn_hidden_size` or assignments to train_cfg.runner.policy_class_name / train_cfg.policy.rnn_hidden_size set them)
        self.recurrent = bool(getattr(policy_cls, "is_recurrent", False))
        # left-right symmetry: mirrored minibatches and / or a mirror loss in PPO's update; the maps are built here from the env.
        # Not config keys either (`--symmetry` / `--symmetry_coef` or assignments to train_cfg.algorithm set them); nothing of it is saved
        self.symmetry = self.algorithm_cfg.get("symmetry") or None
        self._symmetry_maps = None
        if self.symmetry is not None:
            self._check_symmetry()
        # random network distillation: an intrinsic reward added to the rollout's reward rows, its networks trained after
        # PPO's update.  Not config keys either (`--rnd` / `--rnd_*` or assignments to train_cfg.algorithm set them): without `rnd` nothing of
        # rl/rnd.py is constructed.  The algorithm's own keyword arguments are what is left
        rnd_cfg = {k[len("rnd_"):]: v for k, v in self.algorithm_cfg.items() if k.startswith("rnd_")} if self.algorithm_cfg.get("rnd") else None
        self._rnd_requested = rnd_cfg is not None
        self.algorithm_cfg = {k: v for k, v in self.algorithm_cfg.items() if k != "rnd" and not k.startswith("rnd_")}
        self.rnd = None
        if rnd_cfg is not None:
            self._check_rnd(env, rnd_cfg)
        # the action noise's parametrisation: `log` holds log_std, `state_dependent_std` lets the actor emit sigma per state.
        # Not config keys either (`--noise_std_type` / `--state_dependent_std` or assignments to train_cfg.policy set them)
        self.noise_std_type = self.policy_cfg.get("noise_std_type", "scalar")
        self.state_dependent_std = bool(self.policy_cfg.get("state_dependent_std", False))
        self.noise = None   # the "noise" entry of a checkpoint of this run: only when an option is not the default
        if self.noise_std_type != "scalar" or self.state_dependent_std:
            self._check_noise()
            self.noise = {"std_type": self.noise_std_type, "state_dependent": self.state_dependent_std}
        if self.recurrent:
            self._check_recurrent()
        # a Beta action distribution: the policy's support is the env's action box.  Not config keys either (`--action_dist`
        # / `--action_bounds` or assignments to train_cfg.policy set them): with the default `gaussian` nothing of rl/beta.py is imported
        self.action_dist = None   # the "action_dist" entry of a checkpoint of this run: only under the flag
        if self.policy_cfg.get("action_dist", "gaussian") != "gaussian":
            self._check_beta(env)
        else:
            self.policy_cfg = {k: v for k, v in self.policy_cfg.items() if k not in ("action_dist", "action_bounds")}
        # action smoothness: the CAPS regulariser on the actor's mean in PPO's update.  Not config keys either (`--smooth` /
        # `--smooth_*` or assignments to train_cfg.algorithm set them); nothing of it is saved
        self.smooth = self.algorithm_cfg.get("smooth") or None
        if self.smooth is not None:
            self._check_smooth()
        # a concurrent state estimator: a small network regresses privileged columns from the actor's input, its output is
        # appended to that input, and it is trained on the rollout after PPO's update.  Not config keys either (`--estimator` /
        # `--estimator_*` or assignments to train_cfg.runner set them): without `estimator` nothing of rl/estimator.py is constructed
        # value normalisation: the critic learns a normalised value, the statistics follow the rollout's returns.  Not a config
        # key either (`--value_norm` or an assignment to train_cfg.algorithm sets it): without it nothing of rl/value_norm.py is imported.
        # inference_only (scripts/play.py sets it): load() takes the actor from a checkpoint whatever its value_norm entry says
        self.value_norm = self.algorithm_cfg.get("value_norm") or None
        self.inference_only = bool(self.cfg.get("inference_only", False))
        if self.value_norm is not None:
            self._check_value_norm()
        else:
            self.algorithm_cfg = {k: v for k, v in self.algorithm_cfg.items() if k not in ("value_norm", "value_norm_eps")}
        # the Lipschitz gradient penalty: grad_penalty_coef * mean ||d logp / d obs||^2 in PPO's loss.  Not a config key either
        # (`--grad_penalty_coef` or an assignment to train_cfg.algorithm sets it): without it nothing of rl/grad_penalty.py is imported;
        # nothing of it is saved
        self.grad_penalty_coef = self.algorithm_cfg.get("grad_penalty_coef")
        if self.grad_penalty_coef is not None:
            self._check_grad_penalty()
        # layer normalisation in the hidden layers: Linear -> LayerNorm -> ELU in actor and critic.  Not a config key either
        # (`--layer_norm` or an assignment to train_cfg.policy sets it); the estimator's and RND's own networks stay without it
        self.layer_norm = None   # the "layer_norm" entry of a checkpoint of this run: only under the flag
        if bool(self.policy_cfg.get("layer_norm", False)):
            self._check_layer_norm()
            self.layer_norm = {"enabled": True, "eps": float(self.policy_cfg.get("layer_norm_eps", 1e-5))}
        else:
            self.policy_cfg = {k: v for k, v in self.policy_cfg.items() if k not in ("layer_norm", "layer_norm_eps")}
        # multi-critic PPO: a value head, a GAE pass and an advantage normalisation per group of reward terms.  Not config
        # keys either (`--reward_groups` / `--reward_group_weights` or assignments to train_cfg.algorithm set them): without `reward_groups`
        # nothing of rl/multi_critic.py is imported
        self.multi_critic = None   # the "multi_critic" entry of a checkpoint of this run: only under the flag
        if self.algorithm_cfg.get("reward_groups") is not None:   # (an empty spec is refused by the parser, not taken for "no flag")
            self._check_multi_critic(env)
        else:
            self.algorithm_cfg = {k: v for k, v in self.algorithm_cfg.items() if k not in ("reward_groups", "reward_group_weights")}
        # constraints as terminations: constraint violations become termination probabilities that scale the rollout's
        # rewards and the discount inside GAE.  Not config keys either (`--constraints` / `--constraint_*` or assignments to
        # train_cfg.algorithm set them): without `constraints` nothing of rl/constraints.py is imported
        self.constraints = None   # the "constraints" entry of a checkpoint of this run, without the state: only under the flag
        if self.algorithm_cfg.get("constraints") is not None:   # (an empty spec is refused by the parser, not taken for "no flag")
            self._check_constraints()
        else:
            self.algorithm_cfg = {k: v for k, v in self.algorithm_cfg.items() if k != "constraints" and not k.startswith("constraint_")}
        self.estimator = None
        estimator_cfg = self._check_estimator(env) if bool(self.cfg.get("estimator", False)) else None
        # a context-aided estimator network: the estimator's regression plus a stochastic latent that a decoder predicts the
        # next frame from; [v_hat | z] is appended to the actor's input and both networks are trained after PPO's update.  Not config keys
        # either (`--cenet` / `--cenet_*` or assignments to train_cfg.runner set them): without `cenet` nothing of rl/cenet.py is imported
        self.cenet = None
        cenet_cfg = self._check_cenet(env) if bool(self.cfg.get("cenet", False)) else None
        if self.distill_from is not None:
            teacher = self._check_distillation(env, device)
        self.obs_history = self.critic_obs_history = None
        if self.obs_history_length > 1:
            self.obs_history = ObsHistory(env.num_envs, env.num_obs, self.obs_history_length, device)
        if self.critic_obs_history_length > 1:
            self.critic_obs_history = ObsHistory(env.num_envs, env.num_pri_obs, self.critic_obs_history_length, device)
        actor_in = self.obs_history_length * env.num_obs
        critic_in = self.critic_obs_history_length * env.num_pri_obs if env.num_pri_obs is not None else actor_in
        if self.privileged_actor:
            actor_in = critic_in
        if self.distill_from is not None:
            self.teacher_history = ObsHistory(env.num_envs, teacher["frame"], teacher["history"], device) if teacher["history"] > 1 else None
            self.teacher_obs_normalizer = None
            if teacher["norm"] is not None:   # the checkpoint's statistics of that stream, frozen: applied, never updated
                self.teacher_obs_normalizer = EmpiricalNormalization(teacher["width"]).to(device)
                self.teacher_obs_normalizer.load_state_dict(teacher["norm"])
                self.teacher_obs_normalizer.eval()
            student_kw, alg_kw = {}, {}
            student_cls = StudentTeacher
            if self.student_recurrent:   # (nothing of it is imported otherwise)
                from .distillation import StudentTeacherRecurrent as student_cls
                student_kw = {"rnn_hidden_size": self.student_rnn_hidden_size}
                alg_kw = {"gradient_length": self.distill_gradient_length}
            actor_critic = student_cls(actor_in, teacher["width"], env.num_actions, actor_hidden_dims=self.policy_cfg["actor_hidden_dims"],
                                       teacher_hidden_dims=teacher["hidden"], activation=self.policy_cfg.get("activation", "elu"),
                                       noise_std=float(self.cfg.get("distill_noise_std", 0.1)), **student_kw).to(device)
            actor_critic.load_teacher(teacher["state"])
            self.algorithm = _ALGORITHMS["Distillation"](actor_critic=actor_critic, device=device, loss_type=self.cfg.get("distill_loss", "mse"),
                                                         **self.algorithm_cfg, **alg_kw)
            self.distillation = {"teacher_stream": teacher["stream"], "teacher_history": teacher["history"], "teacher_width": teacher["width"],
                                 "loss": self.algorithm.loss_type}
            if self.student_recurrent:
                # save() / load() / get_inference_policy() treat the student as the recurrent actor it is: the checkpoint carries
                # "recurrent", and an ordinary `--recurrent --rnn_hidden_size H` runner loads it (the checks above ran for an MLP policy)
                self.recurrent = True
                self.distillation["student"] = {"recurrent": self.student_rnn_hidden_size, "gradient_length": self.distill_gradient_length}
            self._alt_inputs = self._distill_inputs
        else:
            # (with an estimator the policy acts on [x | est(x)]: E more columns; the normaliser's statistics stay actor_in wide)
            policy_in = actor_in + (len(estimator_cfg["cols"]) if estimator_cfg is not None else 0)
            if cenet_cfg is not None:   # (likewise: [x | v_hat | z], E + Z more columns)
                policy_in = actor_in + len(cenet_cfg["cols"]) + cenet_cfg["latent_dim"]
            actor_critic = policy_cls(policy_in, critic_in, env.num_actions, **self.policy_cfg).to(device)
            extra = {}
            if self.symmetry is not None:   # (a model the joint map refuses, an asymmetric height scan: build_maps' ValueError)
                from .symmetry import build_maps
                self._symmetry_maps = extra["symmetry_maps"] = build_maps(env, device, self.obs_history_length, self.critic_obs_history_length,
                                                                           self.privileged_actor)
            self.algorithm = _ALGORITHMS[self.cfg["algorithm_class_name"]](actor_critic=actor_critic, device=device, **self.algorithm_cfg, **extra)
            if self.privileged_actor:
                self._alt_inputs = self._privileged_inputs
            if self.multi_critic is not None:   # the step kernel's per-term tables, zero-copy views the rollout's store reads every step
                base = env._sim.tensor("BASE_REWARD_TERMS") if self.algorithm.multi_critic.groups.uses_base else None
                self.algorithm.multi_critic.bind_tables(env._sim.tensor("REWARD_TERMS"), base)
            if self.constraints is not None:   # the env's tensors and limits, zero-copy views the rollout's step pass reads every step
                self.algorithm.constraints.bind(env)
            if rnd_cfg is not None:   # (after the policy: its initial parameters are those of a run without the flag)
                from .rnd import RandomNetworkDistillation
                state = rnd_cfg.get("state", "privileged")
                self.rnd = self.algorithm.rnd = RandomNetworkDistillation(
                    env.num_pri_obs if state == "privileged" else env.num_obs, env.num_envs, self.cfg["num_steps_per_env"], device,
                    **rnd_cfg)
            if estimator_cfg is not None:   # (after the policy and RND, as RND after the policy)
                from .estimator import StateEstimator
                self.estimator = StateEstimator(actor_in, env.num_obs, env.num_pri_obs, env.num_envs, self.cfg["num_steps_per_env"], device,
                                                targets=estimator_cfg["targets"], hidden_dims=estimator_cfg["hidden_dims"],
                                                learning_rate=estimator_cfg["learning_rate"], num_epochs=estimator_cfg["num_epochs"])
            if cenet_cfg is not None:   # (after the policy, as the estimator: its initial parameters are those of a run without the flag)
                from .cenet import CENet
                self.cenet = CENet(actor_in, env.num_obs, env.num_obs, env.num_pri_obs, env.num_envs, self.cfg["num_steps_per_env"], device,
                                   **{k: v for k, v in cenet_cfg.items() if k != "cols"})
        self.alg = self.algorithm
        self.num_steps_per_env, self.save_interval = self.cfg["num_steps_per_env"], self.cfg["save_interval"]
        # exact resume: every save() also writes train_state_<it>.pt, the whole training state; not a config key
        # (`--exact_resume` or an assignment to train_cfg.runner sets it)
        self.exact_resume = bool(self.cfg.get("exact_resume", False))
        if self.exact_resume and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("exact_resume: one process only (with more ranks every rank holds its own env shard)")
        if self.exact_resume and self.distill_from is not None:
            raise NotImplementedError("exact_resume: not available for a distillation run (--distill_from)")
        # empirical observation normalisation: running mean / variance of the actor's and -- when the env has privileged
        # observations -- the critic's inputs; what the policy acts on, what the storage keeps and what compute_returns gets are the
        # normalised tensors.  Not a config key either (`--empirical_normalization` or an assignment to train_cfg.runner sets it)
        self.empirical_normalization = bool(self.cfg.get("empirical_normalization", False))
        self.obs_normalizer = self.critic_obs_normalizer = None
        if self.empirical_normalization:
            if not self.privileged_actor:   # (a privileged actor reads the critic's normalised tensor: no actor-side statistics)
                self.obs_normalizer = EmpiricalNormalization(actor_in).to(device)   # (history first, then normalisation: the stacked widths)
            if env.num_pri_obs is not None and self.distill_from is None:   # (a distillation run has no critic)
                self.critic_obs_normalizer = EmpiricalNormalization(critic_in).to(device)
        if self._symmetry_maps is not None and self.empirical_normalization:   # (the storage holds normalised rows: the maps follow the statistics)
            actor_norm = self.obs_normalizer if self.obs_normalizer is not None else self.critic_obs_normalizer   # (privileged actor: the critic's)
            self._symmetry_maps.obs_normalizer = actor_norm
            self._symmetry_maps.critic_obs_normalizer = self.critic_obs_normalizer if self.critic_obs_normalizer is not None else actor_norm
            self._symmetry_maps.refresh()
        self._pending_state = None   # what load_train_state() restored and learn() still has to apply
        self._log_buffers = None     # learn()'s running episode reward / length and the finished episodes' deques
        self._next_iteration = None  # the iteration a save() from inside learn() resumes at
        self.algorithm.init_storage(env.num_envs, self.num_steps_per_env)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            torch.manual_seed(int(train_cfg.get("seed", 1)) + 1000 * dist.get_rank())   # different action noise per shard
        self.env.reset()
        self.log_dir, self.writer = log_dir, None
        self.tot_timesteps, self.tot_time, self.current_learning_iteration = 0, 0.0, 0
        self.is_main = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # Perf/collection time and Perf/learning_time of the last iteration (on_policy_runner.py:235's inputs), also without a log directory;
        # sync_timers: drain the device before each clock is read (bench.py's full_iteration leg: an iteration otherwise ends on the
        # update's .item(), which is a synchronisation too, but the split between the two halves is the host's enqueue time)
        self.last_collection_time = self.last_learn_time = 0.0
        self.sync_timers = False

    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        env, alg = self.env, self.algorithm
        if self.log_dir is not None and self.writer is None and self.is_main:
            self.writer = _ScalarLog(self.log_dir)
        pending, self._pending_state = self._pending_state, None
        if init_at_random_ep_len and pending is None:   # (an exact resume continues the saved episodes)
            env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))
        obs = env.get_observations()
        pri = env.get_privileged_observations()
        critic_obs = pri if pri is not None else obs
        obs, critic_obs = obs.to(self.device), critic_obs.to(self.device)
        if self._alt_inputs is not None:   # (privileged actor, distillation: history and normalisation of both inputs in there)
            obs, critic_obs = self._alt_inputs(obs, critic_obs if pri is not None else None, None)
        elif self.obs_history is not None or self.critic_obs_history is not None:
            # a primed history (an earlier learn() call, an exact resume) already holds the current frames: no frame is pushed twice
            obs, critic_obs = self._stack_history(obs, critic_obs if pri is not None else None, None)
        if self.empirical_normalization and self._alt_inputs is None:
            # the observations learn() starts from, with the statistics as they are: every observation updates the statistics exactly once,
            # after its env.step (a resumed run's first observations went in before the checkpoint; a fresh run's are x / 1.01)
            self.obs_normalizer.train()
            obs_n = self.obs_normalizer.normalize(obs)
            if self.critic_obs_normalizer is not None:
                self.critic_obs_normalizer.train()
                critic_obs = self.critic_obs_normalizer.normalize(critic_obs)
            else:
                critic_obs = obs_n
            obs = obs_n
        if self.estimator is not None:   # the last stage: [x | est(x)]; the frame's targets wait for the row's rollout step
            obs = self.estimator.step(obs, pri.to(self.device), None)
        if self.cenet is not None:   # (likewise): [x | v_hat | z]
            obs = self.cenet.step(obs, pri.to(self.device), None)
        alg.actor_critic.train()
        ep_infos = []
        if pending is None:
            rewbuffer, lenbuffer = deque(maxlen=100), deque(maxlen=100)
            cur_rew = torch.zeros(env.num_envs, dtype=torch.float, device=self.device)
            cur_len = torch.zeros(env.num_envs, dtype=torch.float, device=self.device)
        else:
            rewbuffer, lenbuffer = deque(pending["rewbuffer"], maxlen=100), deque(pending["lenbuffer"], maxlen=100)
            cur_rew, cur_len = pending["cur_rew"].to(self.device), pending["cur_len"].to(self.device)
            # the uninterrupted run captured its graphs at iteration 0, and their warm-up runs drew from the CUDA generator: capture them
            # here, then continue every generator from where the saved run left it
            alg.prepare_graphs(obs, critic_obs)
            self._set_rng_state(pending["rng"])
        self._log_buffers = (cur_rew, cur_len, rewbuffer, lenbuffer)
        done_rew = torch.zeros(self.num_steps_per_env, env.num_envs, dtype=torch.float, device=self.device)
        done_len = torch.zeros(self.num_steps_per_env, env.num_envs, dtype=torch.float, device=self.device)
        tot_iter = self.current_learning_iteration + num_learning_iterations
        for it in range(self.current_learning_iteration, tot_iter):
            start = time.time()
            if self.rnd is not None:
                self.rnd.iteration = it
            if self.constraints is not None:   # this iteration's maximum termination probabilities (a resumed run continues the ramp)
                alg.constraints.set_iteration(it)
            with torch.inference_mode():
                if self.estimator is not None:   # the row this rollout starts with was built from the frames parked last
                    self.estimator.begin_rollout()
                if self.cenet is not None:
                    self.cenet.begin_rollout()
                for t_ in range(self.num_steps_per_env):
                    actions = alg.act(obs, critic_obs)
                    obs, pri, rewards, dones, infos = env.step(actions)
                    if self.rnd is not None:   # the raw frame: before history, normalisation and the privileged actor's re-routing
                        rnd_frame = (pri if self.rnd.state == "privileged" else obs).to(self.device)
                    critic_obs = pri if pri is not None else obs
                    obs, critic_obs, rewards, dones = obs.to(self.device), critic_obs.to(self.device), rewards.to(self.device), dones.to(self.device)
                    if self._alt_inputs is not None:
                        obs, critic_obs = self._alt_inputs(obs, critic_obs if pri is not None else None, dones)
                    elif self.obs_history is not None or self.critic_obs_history is not None:
                        obs, critic_obs = self._stack_history(obs, critic_obs if pri is not None else None, dones)
                    if self.empirical_normalization and self._alt_inputs is None:
                        obs, critic_obs = self._normalize_step(obs, critic_obs if pri is not None else None)
                    if self.estimator is not None:   # this row is acted on at step t_ + 1: its targets are the raw privileged frame of this step
                        obs = self.estimator.step(obs, pri.to(self.device), t_ + 1 if t_ + 1 < self.num_steps_per_env else None)
                    if self.cenet is not None:   # (likewise)
                        obs = self.cenet.step(obs, pri.to(self.device), t_ + 1 if t_ + 1 < self.num_steps_per_env else None)
                    if self.log_dir is not None:
                        if "episode" in infos:
                            ep_infos.append(infos["episode"])
                        # running episode reward / length and the finished episodes' totals: inside process_env_step (one kernel on a
                        # HIP device), read back once per iteration instead of nonzero() + .cpu() per step (on_policy_runner.py:177-179)
                        alg.process_env_step(rewards, dones, infos, log=(cur_rew, cur_len, done_rew[t_], done_len[t_]))
                    else:
                        alg.process_env_step(rewards, dones, infos)
                    if self.rnd is not None:   # into the storage's reward row of this step; the logged episode rewards stay the env's
                        alg.rnd_step(rnd_frame, t_)
                    if self.constraints is not None:   # likewise: delta from the env's tensors as the step left them, the row scaled by 1 - delta
                        alg.constraint_step(t_)
                if self.log_dir is not None:   # one device->host transfer per iteration
                    m = alg.storage.dones.squeeze(-1).bool()
                    rewbuffer.extend(done_rew[m].cpu().tolist())
                    lenbuffer.extend(done_len[m].cpu().tolist())
                if self.sync_timers:
                    torch.cuda.synchronize()
                collection_time = time.time() - start
                start = time.time()
                alg.compute_returns(critic_obs)
            if self.distillation is not None:
                mean_behavior_loss = alg.update()
            else:
                mean_value_loss, mean_surrogate_loss = alg.update()
            if self.rnd is not None:   # the predictor's regression on this rollout, with PPO's epoch and minibatch counts
                mean_rnd_loss = self.rnd.update(alg.num_learning_epochs, alg.num_mini_batches)
                if self.log_dir is not None and self.is_main:
                    mean_intrinsic_reward = self.rnd.intrinsic.mean().item()
            if self.estimator is not None:   # the regression on this rollout: the stored rows' first columns against the stored targets
                mean_estimator_loss = self.estimator.update(alg.storage.observations, alg.num_mini_batches)
            if self.cenet is not None:   # estimation, reconstruction of the successor row's newest frame and KL, on this rollout
                mean_cenet_losses = self.cenet.update(alg.storage.observations, alg.storage.dones, alg.num_mini_batches)
            alg.clear_storage()
            if self.sync_timers:
                torch.cuda.synchronize()
            learn_time = time.time() - start
            self.last_collection_time, self.last_learn_time = collection_time, learn_time
            if self.log_dir is not None and self.is_main:
                self.log(locals())
            if self.log_dir is not None and self.is_main and it % self.save_interval == 0:
                self._next_iteration = it + 1
                self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
            ep_infos.clear()
        self.current_learning_iteration += num_learning_iterations
        if self.log_dir is not None and self.is_main:
            self._next_iteration = self.current_learning_iteration
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))
        self._next_iteration = None

    def _stack_history(self, obs, pri, dones):
        """one env step's raw frames into the histories: (actor input, critic input).  dones None: learn()'s first frames, which fill a
        history that is not primed and leave a primed one as it is"""
        for hist, frame in ((self.obs_history, obs), (self.critic_obs_history, pri)):
            if hist is None or frame is None:
                continue
            if dones is not None:
                stacked = hist.push(frame, dones)
            else:
                stacked = hist.current if hist.primed else hist.fill(frame)
            if hist is self.obs_history:
                obs = stacked
            else:
                pri = stacked
        return obs, (pri if pri is not None else obs)

    @staticmethod
    def _stacked(hist, frame, dones):
        """one history's rows after this frame (dones None: learn()'s first frames, as in _stack_history)"""
        if dones is not None:
            return hist.push(frame, dones)
        return hist.current if hist.primed else hist.fill(frame)

    def _privileged_inputs(self, obs, pri, dones):
        """--privileged_actor: the critic's tensor -- privileged frames, stacked, normalised with the critic's statistics -- is the actor's too"""
        x = pri
        if self.critic_obs_history is not None:
            x = self._stacked(self.critic_obs_history, x, dones)
        if self.empirical_normalization:
            norm = self.critic_obs_normalizer
            if dones is None:   # learn()'s first observations: the statistics as they are
                norm.train()
                x = norm.normalize(x)
            else:
                x, = normalize_step([norm], [x])
        return x, x

    def _distill_inputs(self, obs, pri, dones):
        """--distill_from: (the student's input, the teacher's input).  The student's is the actor stream as ever; the teacher's its own
        stream's raw frames, stacked by the checkpoint's history length and normalised with the checkpoint's frozen statistics"""
        x = pri if self.distillation["teacher_stream"] == "privileged" else obs   # (the raw frames, before the student's stacking)
        if self.teacher_history is not None:
            x = self._stacked(self.teacher_history, x, dones)
        if self.teacher_obs_normalizer is not None:
            x = self.teacher_obs_normalizer.normalize(x)
        if self.obs_history is not None:
            obs = self._stacked(self.obs_history, obs, dones)
        if self.empirical_normalization:
            if dones is None:
                self.obs_normalizer.train()
                obs = self.obs_normalizer.normalize(obs)
            else:
                obs, = normalize_step([self.obs_normalizer], [obs])
        return obs, x

    def _check_privileged_actor(self, env):
        if env.num_pri_obs is None:
            raise ValueError("privileged_actor: this env has no privileged observations for the actor to read")
        if self.obs_history_length != 1:
            raise ValueError(f"privileged_actor with obs_history_length={self.obs_history_length}: the actor reads the critic's tensor, whose "
                             "history is set with --critic_obs_history (train_cfg.runner.critic_obs_history_length)")
        if self.distill_from is not None:
            raise ValueError("privileged_actor and distill_from exclude each other: the student reads the actor's observations")

    def _check_symmetry(self):
        """what --symmetry does not combine with"""
        from .symmetry import MODES
        if self.symmetry not in MODES:
            raise ValueError(f"--symmetry must be one of {MODES}, not {self.symmetry!r}")
        if self.recurrent:
            raise ValueError("--symmetry and --recurrent exclude each other: a mirrored minibatch of a recurrent policy is not implemented")
        if self.distill_from is not None:
            raise ValueError("--symmetry and --distill_from exclude each other: a distillation run has no PPO update to mirror")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--symmetry with a world size above 1 is not implemented: it trains in one process only")

    def _check_smooth(self):
        """what --smooth does not combine with"""
        from .smooth import blocks, check_values
        succ, _ = blocks(self.smooth)
        if self.recurrent:
            raise ValueError("--smooth and --recurrent exclude each other: successor rows of a recurrent policy's minibatch are not implemented")
        if self.symmetry is not None:
            raise ValueError("--smooth and --symmetry exclude each other: both extend the minibatch")
        if self.state_dependent_std:
            raise ValueError("--smooth and --state_dependent_std exclude each other: a smoothness loss on the [mean | s] output is not implemented")
        if self.distill_from is not None:
            raise ValueError("--smooth and --distill_from exclude each other: a distillation run has no PPO loss to add to")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--smooth with --exact_resume: the perturbation's draws are not part of the resumed step order")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--smooth with a world size above 1 is not implemented: it trains in one process only")
        a = self.algorithm_cfg
        check_values(a.get("smooth_temporal_coef", 0.1), a.get("smooth_spatial_coef", 0.1), a.get("smooth_sigma", 0.05), who="runner")
        if succ and int(self.cfg["num_steps_per_env"]) < 2:
            raise ValueError(f"--smooth {self.smooth} with num_steps_per_env={self.cfg['num_steps_per_env']}: a rollout of one step holds no "
                             "successor row (use --smooth spatial or a longer rollout)")

    def _check_grad_penalty(self):
        """what --grad_penalty_coef does not combine with"""
        from .grad_penalty import check_coef
        why = "the penalty's second-order pass covers the plain fp32 MLP actor on one minibatch of stored rows"
        if self.recurrent:
            raise ValueError(f"--grad_penalty_coef and --recurrent exclude each other: {why}")
        if self.symmetry is not None:
            raise ValueError(f"--grad_penalty_coef and --symmetry exclude each other: {why}")
        if self.smooth is not None:
            raise ValueError(f"--grad_penalty_coef and --smooth exclude each other: {why}")
        if self.state_dependent_std:
            raise ValueError(f"--grad_penalty_coef and --state_dependent_std exclude each other: {why}, with one sigma per action")
        if self.distill_from is not None:
            raise ValueError("--grad_penalty_coef and --distill_from exclude each other: a distillation run has no PPO loss to add to")
        if self.algorithm_cfg.get("precision", "fp32") == "bf16":
            raise ValueError(f"--grad_penalty_coef and --precision bf16 exclude each other: {why}")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--grad_penalty_coef with --exact_resume is not implemented: a resumed run with the penalty is not pinned "
                                      "bit for bit")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--grad_penalty_coef with a world size above 1 is not implemented: it trains in one process only")
        check_coef(self.grad_penalty_coef, who="runner")

    def _check_layer_norm(self):
        """what --layer_norm does not combine with"""
        if self.recurrent:
            raise ValueError("--layer_norm and --recurrent exclude each other: the recurrent policy's MLPs have no LayerNorm path")
        if self.algorithm_cfg.get("precision", "fp32") == "bf16":
            raise ValueError("--layer_norm and --precision bf16 exclude each other: the bf16 products cover Linear -> ELU hidden layers only")
        if self.grad_penalty_coef is not None:
            raise ValueError("--layer_norm and --grad_penalty_coef exclude each other: the penalty's second-order pass covers Linear -> ELU "
                             "hidden layers only")
        if self.distill_from is not None:
            raise ValueError("--layer_norm and --distill_from exclude each other: a student with LayerNorm hidden layers is not implemented")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--layer_norm with --exact_resume is not implemented: a resumed run with LayerNorm hidden layers is not "
                                      "pinned bit for bit")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--layer_norm with a world size above 1 is not implemented: it trains in one process only")
        if self.policy_cfg.get("activation", "elu") != "elu":
            raise ValueError(f"--layer_norm needs the elu activation, not {self.policy_cfg.get('activation')!r}: the fused pass is LayerNorm + ELU")

    def _check_multi_critic(self, env):
        """what --reward_groups needs of the env and does not combine with; parses the spec against the env's active terms and hands PPO
        the parsed groups, the weights and a critic with one output per group"""
        from .. import _capi
        from .multi_critic import parse_reward_groups, parse_weights
        why = "the per-group critic, GAE and value loss cover the plain fp32 MLP policy on the plain minibatch"
        if self.recurrent:
            raise ValueError(f"--reward_groups and --recurrent exclude each other: {why}")
        if self.value_norm is not None:
            raise ValueError("--reward_groups and --value_norm exclude each other: return statistics per value head are not implemented")
        if self.symmetry is not None:
            raise ValueError(f"--reward_groups and --symmetry exclude each other: {why}")
        if self.smooth is not None:
            raise ValueError(f"--reward_groups and --smooth exclude each other: {why}")
        if self.grad_penalty_coef is not None:
            raise ValueError(f"--reward_groups and --grad_penalty_coef exclude each other: {why}")
        if self.state_dependent_std:
            raise ValueError("--reward_groups and --state_dependent_std exclude each other: the multi-critic loss takes one sigma per action")
        if self._rnd_requested:
            raise ValueError("--reward_groups and --rnd exclude each other: the intrinsic reward belongs to no group")
        if bool(self.cfg.get("estimator", False)):
            raise ValueError("--reward_groups and --estimator exclude each other: the combination is not pinned")
        if bool(self.cfg.get("cenet", False)):
            raise ValueError("--reward_groups and --cenet exclude each other: the combination is not pinned")
        if self.layer_norm is not None:
            raise ValueError(f"--reward_groups and --layer_norm exclude each other: {why}")
        if self.algorithm_cfg.get("precision", "fp32") == "bf16":
            raise ValueError(f"--reward_groups and --precision bf16 exclude each other: {why}")
        if self.distill_from is not None:
            raise ValueError("--reward_groups and --distill_from exclude each other: a distillation run has no critic to split")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--reward_groups with --exact_resume is not implemented: a resumed multi-critic run is not pinned bit for bit")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--reward_groups with a world size above 1 is not implemented: the advantage statistics are per process")
        if not bool(getattr(env.cfg.env, "publish_reward_terms", True)):
            raise ValueError("--reward_groups needs an env built with env_cfg.env.publish_reward_terms = True (scripts/train.py sets it before "
                             "make_env): the group rewards are sums over the step kernel's per-term reward tables")
        if bool(env.cfg.rewards.only_positive_rewards):
            raise ValueError("--reward_groups and rewards.only_positive_rewards = True exclude each other: with the clip the groups no longer add "
                             "up to the env's reward")
        groups = parse_reward_groups(self.algorithm_cfg["reward_groups"], list(env.reward_scales), _capi.REWARD_TERMS, _capi.BASE_REWARD_TERMS)
        weights = parse_weights(self.algorithm_cfg.get("reward_group_weights"), groups.K)
        self.algorithm_cfg = {**self.algorithm_cfg, "reward_groups": groups, "reward_group_weights": weights}
        self.policy_cfg = {**self.policy_cfg, "num_critic_outputs": groups.K}
        self.multi_critic = groups.entry(weights)

    def _check_constraints(self):
        """what --constraints does not combine with; parses the spec and checks its options, so that PPO gets what it will keep"""
        from .constraints import check_options, parse_constraints
        why = "the combination is not pinned"
        if self.recurrent:
            raise ValueError(f"--constraints and --recurrent exclude each other: {why}")
        if self.value_norm is not None:
            raise ValueError("--constraints and --value_norm exclude each other: both replace compute_returns")
        if self.multi_critic is not None:
            raise ValueError("--constraints and --reward_groups exclude each other: both replace compute_returns")
        if self._rnd_requested:
            raise ValueError("--constraints and --rnd exclude each other: the order of the two edits of the reward row is not pinned")
        if self.distill_from is not None:
            raise ValueError("--constraints and --distill_from exclude each other: a distillation run has no returns to discount")
        if self.action_dist is not None:
            raise ValueError(f"--constraints and --action_dist beta exclude each other: {why}")
        if self.symmetry is not None:
            raise ValueError(f"--constraints and --symmetry exclude each other: {why}")
        if self.smooth is not None:
            raise ValueError(f"--constraints and --smooth exclude each other: {why}")
        if self.grad_penalty_coef is not None:
            raise ValueError(f"--constraints and --grad_penalty_coef exclude each other: {why}")
        if self.state_dependent_std:
            raise ValueError(f"--constraints and --state_dependent_std exclude each other: {why}")
        if self.layer_norm is not None:
            raise ValueError(f"--constraints and --layer_norm exclude each other: {why}")
        if bool(self.cfg.get("estimator", False)):
            raise ValueError(f"--constraints and --estimator exclude each other: {why}")
        if bool(self.cfg.get("cenet", False)):
            raise ValueError(f"--constraints and --cenet exclude each other: {why}")
        if self.algorithm_cfg.get("precision", "fp32") == "bf16":
            raise ValueError(f"--constraints and --precision bf16 exclude each other: {why}")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--constraints with --exact_resume is not implemented: c_max and the previous actions are not part of "
                                      "train_state_<it>.pt")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--constraints with a world size above 1 is not implemented: the column maxima are per process")
        a = self.algorithm_cfg
        spec = parse_constraints(a["constraints"])
        tau, ramp, clip = check_options(a.get("constraint_tau", 0.95), a.get("constraint_ramp_its", 1000), a.get("constraint_reward_clip", "zero"))
        self.algorithm_cfg = {**a, "constraints": spec, "constraint_tau": tau, "constraint_ramp_its": ramp, "constraint_reward_clip": clip}
        self.constraints = {"spec": spec.key(), "tau": tau, "ramp_its": ramp, "reward_clip": clip}

    def _check_value_norm(self):
        """what --value_norm does not combine with"""
        modes = ("running", "popart")   # (rl.value_norm.MODES)
        if self.value_norm not in modes:
            raise ValueError(f"--value_norm must be one of {modes}, not {self.value_norm!r}")
        if self.recurrent:
            raise ValueError("--value_norm and --recurrent exclude each other: denormalising a recurrent critic's rollout and bootstrap values "
                             "is not implemented")
        if self.distill_from is not None:
            raise ValueError("--value_norm and --distill_from exclude each other: a distillation run has no critic whose target could be normalised")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--value_norm with --exact_resume: the return statistics are not part of train_state_<it>.pt")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--value_norm with a world size above 1 is not implemented: the return statistics are per process")

    def _check_rnd(self, env, rnd_cfg):
        """what --rnd does not combine with"""
        from .rnd import STATES
        state = rnd_cfg.get("state", "privileged")
        if state not in STATES:
            raise ValueError(f"--rnd_state must be one of {STATES}, not {state!r}")
        if state == "privileged" and env.num_pri_obs is None:
            raise ValueError("--rnd_state privileged: this env has no privileged observations (pass --rnd_state obs)")
        if self.distill_from is not None:
            raise ValueError("--rnd and --distill_from exclude each other: a distillation run has no reward for an intrinsic one to add to")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--rnd with --exact_resume: RND's state is not part of train_state_<it>.pt")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--rnd with a world size above 1 is not implemented: the return statistics are per process")

    def _check_estimator(self, env):
        """what --estimator does not combine with; returns its options: targets, their columns, hidden_dims, learning_rate, num_epochs"""
        from .estimator import check_hidden_dims, check_layout, parse_targets, target_columns
        if self.recurrent:
            raise ValueError("--estimator and --recurrent exclude each other: the memory is the estimator")
        if self.privileged_actor:
            raise ValueError("--estimator and --privileged_actor exclude each other: the actor already reads the targets")
        if self.distill_from is not None:
            raise ValueError("--estimator and --distill_from exclude each other: a distillation run has no PPO update the estimator trains beside")
        if self.symmetry is not None:
            raise ValueError("--estimator and --symmetry exclude each other: a mirror map of the appended columns is not implemented")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--estimator with --exact_resume: the estimator's state is not part of train_state_<it>.pt")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--estimator with a world size above 1 is not implemented: it trains in one process only")
        check_layout(env)
        targets = parse_targets(self.cfg.get("estimator_targets", "lin_vel"))
        return {"targets": targets, "cols": target_columns(targets, env.num_obs),
                "hidden_dims": check_hidden_dims(self.cfg.get("estimator_hidden_dims", (128, 64))),
                "learning_rate": float(self.cfg.get("estimator_learning_rate", 1e-3)), "num_epochs": int(self.cfg.get("estimator_num_epochs", 1))}

    def _check_cenet(self, env):
        """what --cenet does not combine with; returns CENet's options: targets, their columns, latent_dim, beta, encoder_dims,
        decoder_dims, learning_rate, num_epochs"""
        from .cenet import MAX_TARGETS, check_dims, check_layout, check_values, parse_targets, target_columns
        pinned = "the combination is not pinned"
        if bool(self.cfg.get("estimator", False)):
            raise ValueError("--cenet and --estimator exclude each other: CENet contains the estimator (its v_hat head; pass --cenet_targets)")
        if self.recurrent:
            raise ValueError("--cenet and --recurrent exclude each other: the memory is the estimator")
        if self.privileged_actor:
            raise ValueError("--cenet and --privileged_actor exclude each other: the actor already reads the targets")
        if self.distill_from is not None:
            raise ValueError("--cenet and --distill_from exclude each other: a distillation run has no PPO update CENet trains beside")
        if self.symmetry is not None:
            raise ValueError("--cenet and --symmetry exclude each other: a mirror map of the appended columns is not implemented")
        if self.smooth is not None:
            raise ValueError("--cenet and --smooth exclude each other: the perturbed and successor rows would carry another draw of z")
        if self.grad_penalty_coef is not None:
            raise ValueError(f"--cenet and --grad_penalty_coef exclude each other: {pinned}")
        if self.state_dependent_std:
            raise ValueError(f"--cenet and --state_dependent_std exclude each other: {pinned}")
        if self._rnd_requested:
            raise ValueError(f"--cenet and --rnd exclude each other: {pinned}")
        if self.layer_norm is not None:
            raise ValueError(f"--cenet and --layer_norm exclude each other: {pinned}")
        if self.multi_critic is not None:
            raise ValueError(f"--cenet and --reward_groups exclude each other: {pinned}")
        if self.action_dist is not None:
            raise ValueError(f"--cenet and --action_dist beta exclude each other: {pinned}")
        if self.algorithm_cfg.get("precision", "fp32") == "bf16":
            raise ValueError(f"--cenet and --precision bf16 exclude each other: {pinned}")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--cenet with --exact_resume: CENet's state and its draws are not part of train_state_<it>.pt")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--cenet with a world size above 1 is not implemented: it trains in one process only")
        check_layout(env)
        targets = parse_targets(self.cfg.get("cenet_targets", "lin_vel"))
        cols = target_columns(targets, env.num_obs)
        if len(cols) > MAX_TARGETS:
            raise ValueError(f"--cenet_targets: {len(cols)} columns, at most {MAX_TARGETS}")
        out = {"targets": targets, "cols": cols, "latent_dim": int(self.cfg.get("cenet_latent_dim", 16)), "beta": float(self.cfg.get("cenet_beta", 1.0)),
               "encoder_dims": check_dims(self.cfg.get("cenet_encoder_dims", (128, 64)), "cenet_encoder_dims"),
               "decoder_dims": check_dims(self.cfg.get("cenet_decoder_dims", (64, 128)), "cenet_decoder_dims"),
               "learning_rate": float(self.cfg.get("cenet_learning_rate", 1e-3)), "num_epochs": int(self.cfg.get("cenet_num_epochs", 1))}
        check_values(out["latent_dim"], out["beta"], out["learning_rate"], out["num_epochs"])
        return out

    def _check_noise(self):
        """what --noise_std_type log / --state_dependent_std do not combine with"""
        from .modules import NOISE_STD_TYPES
        if self.noise_std_type not in NOISE_STD_TYPES:
            raise ValueError(f"--noise_std_type must be one of {NOISE_STD_TYPES}, not {self.noise_std_type!r}")
        if self.distill_from is not None:
            which = "--state_dependent_std" if self.state_dependent_std else f"--noise_std_type {self.noise_std_type}"
            raise ValueError(f"{which} and --distill_from exclude each other: the student's action noise is a fixed buffer "
                             "(--distill_noise_std), there is no noise parameter to shape")
        if not self.state_dependent_std:
            return   # (`log` alone composes with everything the default composes with: only the parameter differs)
        if self.recurrent:
            raise ValueError("--state_dependent_std and --recurrent exclude each other: a recurrent policy with a state-dependent sigma is "
                             "not implemented")
        if self.symmetry is not None:
            raise ValueError("--state_dependent_std and --symmetry exclude each other: a mirror map of the [mean | s] output is not implemented")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--state_dependent_std with a world size above 1 is not implemented: it trains in one process only")

    def _check_beta(self, env):
        """what --action_dist beta does not combine with, and the action box: policy_cfg["action_bounds"] becomes (lo, hi) per joint"""
        from .beta import ACTION_DISTS, resolve_bounds
        kind = self.policy_cfg["action_dist"]
        if kind not in ACTION_DISTS:
            raise ValueError(f"--action_dist must be one of {ACTION_DISTS}, not {kind!r}")
        why = "the Beta policy's loss, rollout step and storage cover the plain fp32 MLP policy of a PPO run in one process"
        if self.noise_std_type != "scalar":
            raise ValueError(f"--action_dist beta and --noise_std_type {self.noise_std_type} exclude each other: a Beta policy has no noise parameter")
        if self.state_dependent_std:
            raise ValueError("--action_dist beta and --state_dependent_std exclude each other: a Beta policy has no sigma to emit")
        if self.recurrent:
            raise ValueError(f"--action_dist beta and --recurrent exclude each other: {why}")
        if self.symmetry is not None:
            raise ValueError("--action_dist beta and --symmetry exclude each other: a mirror map of the [p | q] output is not implemented")
        if self.algorithm_cfg.get("smooth"):
            raise ValueError("--action_dist beta and --smooth exclude each other: a smoothness loss on the [p | q] output is not implemented")
        if self.algorithm_cfg.get("grad_penalty_coef") is not None:
            raise ValueError("--action_dist beta and --grad_penalty_coef exclude each other: the penalty differentiates a Gaussian's log-probability")
        if self.algorithm_cfg.get("reward_groups") is not None:
            raise ValueError("--action_dist beta and --reward_groups exclude each other: the multi-critic loss is a Gaussian policy's")
        if self.distill_from is not None:
            raise ValueError("--action_dist beta and --distill_from exclude each other: the student regresses a mean action under a fixed "
                             "Gaussian noise")
        if self._rnd_requested:
            raise ValueError("--action_dist beta and --rnd exclude each other: the combination is not pinned")
        if bool(self.cfg.get("estimator", False)):
            raise ValueError("--action_dist beta and --estimator exclude each other: the combination is not pinned")
        if bool(self.cfg.get("cenet", False)):
            raise ValueError("--action_dist beta and --cenet exclude each other: the combination is not pinned")
        if bool(self.policy_cfg.get("layer_norm", False)):
            raise ValueError("--action_dist beta and --layer_norm exclude each other: the combination is not pinned")
        if self.algorithm_cfg.get("precision", "fp32") != "fp32":
            raise ValueError(f"--action_dist beta and --precision {self.algorithm_cfg['precision']} exclude each other: {why}")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--action_dist beta with --exact_resume is not implemented: the eager rollout step's draws are not pinned "
                                      "against an uninterrupted run")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--action_dist beta with a world size above 1 is not implemented: it trains in one process only")
        if self.policy_cfg.get("fixed_std", False):
            raise ValueError("--action_dist beta and fixed_std exclude each other: a Beta policy has no std parameter to fix")
        if self.policy_cfg.get("actor_output_activation") is not None:
            raise ValueError(f"--action_dist beta and actor_output_activation={self.policy_cfg['actor_output_activation']!r} exclude each other: "
                             "the output layer is [p | q], an activation on it is not defined")
        lo, hi = resolve_bounds(env.cfg.normalization, env.num_actions, self.policy_cfg.get("action_bounds"))
        self.policy_cfg = dict(self.policy_cfg, action_bounds=(lo, hi))
        self.action_dist = {"kind": kind, "lo": lo, "hi": hi}

    def _check_recurrent(self):
        """what a recurrent policy (--recurrent) does not combine with"""
        if self.obs_history_length != 1 or self.critic_obs_history_length != 1:
            raise ValueError(f"--recurrent with --obs_history {self.obs_history_length} --critic_obs_history {self.critic_obs_history_length}: the "
                             "memory replaces the frame stack (drop one of the two options)")
        if self.privileged_actor:
            raise ValueError("--recurrent and --privileged_actor exclude each other: a recurrent teacher is not implemented")
        if self.distill_from is not None:
            raise NotImplementedError("--recurrent with --distill_from: --recurrent builds PPO's recurrent actor-critic, which distillation does "
                                      "not train (a recurrent student is --distill_from with --student_recurrent)")
        if self.algorithm_cfg.get("precision", "fp32") != "fp32":
            raise ValueError(f"--recurrent with --precision {self.algorithm_cfg['precision']}: the recurrent policy runs in fp32")
        if bool(self.cfg.get("exact_resume", False)):
            raise NotImplementedError("--recurrent with --exact_resume: the memories' state is not part of train_state_<it>.pt")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("--recurrent with a world size above 1: a recurrent policy trains in one process only")

    def _check_student_recurrent(self):
        """the refusals of a recurrent distillation student (--student_recurrent); sets student_rnn_hidden_size and distill_gradient_length"""
        if self.distill_from is None:
            raise ValueError("--student_recurrent without --distill_from: the recurrent student is distilled from a teacher's checkpoint "
                             "(PPO's own recurrent policy is --recurrent)")
        if self.obs_history_length != 1:
            raise ValueError(f"--student_recurrent with --obs_history {self.obs_history_length}: the memory replaces the stack, the student "
                             "reads single actor frames (drop one of the two options)")
        from .recurrent import check_rnn
        self.student_rnn_hidden_size = check_rnn("lstm", 1, self.cfg.get("student_rnn_hidden_size", 256))
        L = self.cfg.get("distill_gradient_length", 15)
        if not isinstance(L, int) or isinstance(L, bool) or L < 0:
            raise ValueError(f"--distill_gradient_length must be an integer >= 0 (0: the whole rollout in one window), not {L!r}")
        self.distill_gradient_length = L

    def _check_distillation(self, env, device):
        """the refusals of a distillation run; returns what the checkpoint at distill_from says about its actor (distillation.read_teacher)"""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("distill_from: one process only")
        if self.algorithm_cfg.get("precision", "fp32") != "fp32":
            raise ValueError(f"distill_from: precision={self.algorithm_cfg['precision']!r} is not available, the student trains in fp32")
        if self.critic_obs_history_length != 1:
            raise ValueError(f"distill_from with critic_obs_history_length={self.critic_obs_history_length}: a distillation run has no critic "
                             "(the teacher's history length comes from its checkpoint)")
        loaded = torch.load(self.distill_from, map_location=device, weights_only=False)
        return read_teacher(loaded, self.distill_from, env.num_obs, env.num_pri_obs, env.num_actions)

    def _normalize_step(self, obs, pri):
        """one env step's observations into the statistics (training mode) and back normalised: (actor input, critic input)"""
        if pri is not None and self.critic_obs_normalizer is not None:
            obs, pri = normalize_step([self.obs_normalizer, self.critic_obs_normalizer], [obs, pri])
            return obs, pri
        obs, = normalize_step([self.obs_normalizer], [obs])
        return obs, obs

    def log(self, locs, width=80, pad=35):
        it = locs["it"]
        self.tot_timesteps += self.num_steps_per_env * self.env.num_envs * self.world
        iteration_time = locs["collection_time"] + locs["learn_time"]
        self.tot_time += iteration_time
        w = self.writer
        ep_string = ""
        if locs["ep_infos"]:
            for key in locs["ep_infos"][0]:
                vals = [torch.as_tensor(e[key], dtype=torch.float).reshape(-1).to(self.device) for e in locs["ep_infos"]]
                value = torch.cat(vals).mean().item()
                w.add_scalar("Episode/" + key, value, it)
                ep_string += f"{f'Mean episode {key}:':>{pad}} {value:.4f}\n"
        fps = int(self.num_steps_per_env * self.env.num_envs * self.world / iteration_time)
        alg = self.algorithm
        if self.distillation is not None:
            w.add_scalar("Loss/behavior", locs["mean_behavior_loss"], it)
            w.add_scalar("Loss/learning_rate", alg.learning_rate, it)
        else:
            w.add_scalar("Loss/value_function", locs["mean_value_loss"], it)
            w.add_scalar("Loss/surrogate", locs["mean_surrogate_loss"], it)
            w.add_scalar("Loss/learning_rate", alg.learning_rate, it)
            w.add_scalar("Loss/kl", alg.mean_kl, it)
            if self.symmetry is not None:
                w.add_scalar("Loss/symmetry", alg.mean_symmetry_loss, it)
            if self.smooth is not None:
                w.add_scalar("Loss/smooth_temporal", alg.mean_smooth_temporal, it)
                w.add_scalar("Loss/smooth_spatial", alg.mean_smooth_spatial, it)
            if self.grad_penalty_coef is not None:
                w.add_scalar("Loss/grad_penalty", alg.mean_grad_penalty, it)
            if self.rnd is not None:
                w.add_scalar("Loss/rnd", locs["mean_rnd_loss"], it)
                w.add_scalar("Train/mean_intrinsic_reward", locs["mean_intrinsic_reward"], it)
                w.add_scalar("Train/rnd_weight", self.rnd.weight(it), it)
            if self.estimator is not None:
                w.add_scalar("Loss/estimator", locs["mean_estimator_loss"], it)
            if self.cenet is not None:
                for name, value in zip(("estimation", "reconstruction", "kl"), locs["mean_cenet_losses"]):
                    w.add_scalar("Loss/cenet_" + name, value, it)
            if self.multi_critic is not None:   # (Loss/value_function above is the sum over the heads)
                spread = alg.multi_critic.stats[:, 1].tolist()   # the raw advantages' std per group, before normalisation
                for k, name in enumerate(alg.multi_critic.groups.names):
                    w.add_scalar("Loss/value_function_" + name, alg.multi_critic.mean_head_losses[k], it)
                    w.add_scalar("Train/adv_std_" + name, spread[k], it)
            if self.constraints is not None:   # of the rollout just trained on: one read-back
                for name, value in alg.constraints.scalars().items():
                    w.add_scalar("Constraint/" + name, value, it)
            if self.value_norm is not None:   # (Loss/value_function above is in normalised units then)
                w.add_scalar("Train/value_norm_mean", alg.value_norm.mean.item(), it)
                w.add_scalar("Train/value_norm_std", alg.value_norm.std.item(), it)
        w.add_scalar("Perf/total_fps", fps, it)
        w.add_scalar("Perf/collection time", locs["collection_time"], it)
        w.add_scalar("Perf/learning_time", locs["learn_time"], it)
        if len(locs["rewbuffer"]) > 0:
            mr, ml = statistics.mean(locs["rewbuffer"]), statistics.mean(locs["lenbuffer"])
            w.add_scalar("Train/mean_reward", mr, it)
            w.add_scalar("Train/mean_episode_length", ml, it)
            w.add_scalar("Train/mean_reward/time", mr, self.tot_time)
            w.add_scalar("Train/mean_episode_length/time", ml, self.tot_time)
        if self.state_dependent_std:   # per action, the mean over the rollout just trained on (clear_storage() keeps the rows)
            stds = alg.storage.sigma.detach().flatten(0, 1).mean(0)
        elif self.action_dist is not None:   # the Beta's std in action units (ActorCriticMLP.action_std's formula), over the same rows
            from .beta import std_torch
            stds = std_torch(alg.storage.mu.detach().flatten(0, 1), alg.storage.sigma.detach().flatten(0, 1),
                             alg.actor_critic.action_span).mean(0)
        elif self.distillation is not None:   # (a student's noise is a fixed buffer)
            stds = alg.actor_critic.std.detach()
        else:
            stds = alg.actor_critic.noise_std().detach()
        for i, s in enumerate(stds):
            w.add_scalar(f"Policy/noise_std_{i}", s.item(), it)
        w.add_scalar("Policy/mean_noise_std", stds.mean().item(), it)
        head = f" Learning iteration {it}/{self.current_learning_iteration + locs['num_learning_iterations']} "
        out = f"{'#' * width}\n{head.center(width, ' ')}\n\n"
        out += f"{'Computation:':>{pad}} {fps:.0f} steps/s (collection: {locs['collection_time']:.3f}s, learning {locs['learn_time']:.3f}s)\n"
        if self.distillation is not None:
            out += f"{'Behavior loss:':>{pad}} {locs['mean_behavior_loss']:.6f}\n"
        else:
            out += f"{'Value function loss:':>{pad}} {locs['mean_value_loss']:.4f}\n{'Surrogate loss:':>{pad}} {locs['mean_surrogate_loss']:.4f}\n"
        out += f"{'Mean action noise std:':>{pad}} {stds.mean().item():.2f}\n"
        if len(locs["rewbuffer"]) > 0:
            out += f"{'Mean reward:':>{pad}} {statistics.mean(locs['rewbuffer']):.2f}\n{'Mean episode length:':>{pad}} {statistics.mean(locs['lenbuffer']):.2f}\n"
        out += ep_string + f"{'-' * width}\n{'Total timesteps:':>{pad}} {self.tot_timesteps}\n{'Iteration time:':>{pad}} {iteration_time:.2f}s\n{'Total time:':>{pad}} {self.tot_time:.2f}s\n"
        print(out)

    def save(self, path, infos=None):
        saved = {"model_state_dict": self.algorithm.actor_critic.state_dict(),
                 "optimizer_state_dict": self.algorithm.optimizer.state_dict(),
                 "iter": self.current_learning_iteration, "infos": infos}
        if self.empirical_normalization:   # (rsl_rl 2.x's keys; absent otherwise: the checkpoint keeps exactly the reference's keys)
            actor_norm = self.obs_normalizer if self.obs_normalizer is not None else self.critic_obs_normalizer   # (privileged actor: the critic's)
            saved["obs_norm_state_dict"] = actor_norm.state_dict()
            critic_norm = self.critic_obs_normalizer if self.critic_obs_normalizer is not None else self.obs_normalizer
            saved["critic_obs_norm_state_dict"] = critic_norm.state_dict()
        if self.obs_history_length > 1 or self.critic_obs_history_length > 1 or self.distillation is not None:   # (absent otherwise, as above)
            saved["obs_history"] = {"actor": self.obs_history_length, "critic": self.critic_obs_history_length}
        if self.privileged_actor:   # (absent otherwise)
            saved["privileged_actor"] = True
        if self.distillation is not None:   # (likewise)
            saved["distillation"] = dict(self.distillation)
        if self.recurrent:   # (likewise)
            saved["recurrent"] = {"hidden_size": self.algorithm.actor_critic.rnn_hidden_size}
        if self.noise is not None:   # (likewise)
            saved["noise"] = dict(self.noise)
        if self.action_dist is not None:   # (likewise): the kind and the action box
            saved["action_dist"] = {k: (list(v) if isinstance(v, list) else v) for k, v in self.action_dist.items()}
        if self.rnd is not None:   # (likewise): both networks, RND's normaliser, the discounted-return state, the optimizer, the configuration
            saved["rnd"] = self.rnd.checkpoint()
        if self.estimator is not None:   # (likewise): the network, its optimizer, the targets and hidden layers
            saved["estimator"] = self.estimator.checkpoint()
        if self.cenet is not None:   # (likewise): encoder and decoder, their optimizer, the targets, the latent width and the hidden layers
            saved["cenet"] = self.cenet.checkpoint()
        if self.value_norm is not None:   # (likewise): the mode, eps and the five statistics
            saved["value_norm"] = self.algorithm.value_norm.checkpoint()
        if self.layer_norm is not None:   # (likewise): that the hidden layers are Linear -> LayerNorm -> ELU, and the LayerNorms' eps
            saved["layer_norm"] = dict(self.layer_norm)
        if self.multi_critic is not None:   # (likewise): the groups' names and terms, the weights
            saved["multi_critic"] = {"groups": {n: list(t) for n, t in self.multi_critic["groups"].items()},
                                     "weights": list(self.multi_critic["weights"])}
        if self.constraints is not None:   # (likewise): the spec, tau, the ramp, the clip and the running column maxima
            saved["constraints"] = self.algorithm.constraints.checkpoint()
        torch.save(saved, path)
        if self.exact_resume:
            torch.save(self._train_state(), train_state_path(path))

    def _train_state(self):
        """train_state_<it>.pt: everything besides model_<it>.pt that the run's next iteration depends on"""
        dev = torch.device(self.device)
        cur_rew, cur_len, rewbuffer, lenbuffer = self._log_buffers if self._log_buffers is not None else (None, None, [], [])
        history = {}
        if self.obs_history is not None or self.critic_obs_history is not None:   # (no key otherwise: the file is what it was)
            history = {"obs_history": {"actor": self.obs_history.state_dict() if self.obs_history is not None else None,
                                       "critic": self.critic_obs_history.state_dict() if self.critic_obs_history is not None else None}}
        return {
            **history,
            "format": 1,
            "next_iteration": self._next_iteration if self._next_iteration is not None else self.current_learning_iteration,
            "env": self.env.get_state(),
            "alg": self.algorithm.get_train_state(),
            "rng": {"torch_cpu": torch.get_rng_state(), "torch_cuda": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None,
                    "python": random.getstate()},
            "runner": {"tot_timesteps": self.tot_timesteps, "tot_time": self.tot_time,
                       "cur_rew": cur_rew.cpu() if cur_rew is not None else None, "cur_len": cur_len.cpu() if cur_len is not None else None,
                       "rewbuffer": list(rewbuffer), "lenbuffer": list(lenbuffer)},
        }

    def _set_rng_state(self, rng):
        torch.set_rng_state(rng["torch_cpu"])
        if rng["torch_cuda"] is not None:
            torch.cuda.set_rng_state(rng["torch_cuda"], torch.device(self.device))
        random.setstate(rng["python"])

    def load_train_state(self, model_path):
        """Exact resume from the train_state_<it>.pt next to model_<it>.pt (load(model_path) first): env, learning rate, iteration
        counter and logging state now; the random generators when learn() has captured its graphs.  Raises if the file is missing."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("exact_resume: one process only (with more ranks every rank holds its own env shard)")
        path = train_state_path(model_path)
        if not os.path.exists(path):
            raise FileNotFoundError(f"exact resume: {path} is missing (the run was not saved with exact_resume)")
        state = torch.load(path, map_location="cpu", weights_only=False)
        saved_hist = state.get("obs_history") or {"actor": None, "critic": None}
        for which, hist in (("actor", self.obs_history), ("critic", self.critic_obs_history)):
            if (saved_hist[which] is None) != (hist is None):
                raise ValueError(f"exact resume: {path} {'holds' if hist is None else 'lacks'} the {which}'s observation history, this runner "
                                 f"{'has none' if hist is None else 'needs it'} (--obs_history / --critic_obs_history must match the saved run)")
        for which, hist in (("actor", self.obs_history), ("critic", self.critic_obs_history)):
            if hist is not None:
                hist.load_state_dict(saved_hist[which])   # (raises ValueError on other shapes)
        self.env.set_state(state["env"])
        # the parameters exactly as saved: load() keeps the reference's reset of `std` to set_noise_std (actor_critic_mlp.py:116-134)
        saved = torch.load(model_path, map_location=self.device, weights_only=False)["model_state_dict"]
        torch.nn.Module.load_state_dict(self.algorithm.actor_critic, saved)
        self.algorithm.set_train_state(state["alg"])
        self.current_learning_iteration = state["next_iteration"]
        r = state["runner"]
        self.tot_timesteps, self.tot_time = r["tot_timesteps"], r["tot_time"]
        zeros = torch.zeros(self.env.num_envs, dtype=torch.float)
        self._pending_state = {"rng": state["rng"], "rewbuffer": r["rewbuffer"], "lenbuffer": r["lenbuffer"],
                               "cur_rew": r["cur_rew"] if r["cur_rew"] is not None else zeros, "cur_len": r["cur_len"] if r["cur_len"] is not None else zeros}
        return state

    def load(self, path, load_optimizer=True):
        loaded = torch.load(path, map_location=self.device, weights_only=False)
        if ("obs_norm_state_dict" in loaded) != self.empirical_normalization:
            raise ValueError(f"{path} was saved with empirical_normalization={'obs_norm_state_dict' in loaded}, this runner has "
                             f"empirical_normalization={self.empirical_normalization}: the policy's inputs would not be what it was trained on "
                             "(pass --empirical_normalization, or set train_cfg.runner.empirical_normalization, to match the checkpoint)")
        if bool(loaded.get("privileged_actor", False)) != self.privileged_actor:
            raise ValueError(f"{path} was saved with privileged_actor={bool(loaded.get('privileged_actor', False))}, this runner has "
                             f"privileged_actor={self.privileged_actor}: the policy's inputs would not be what it was trained on "
                             "(pass --privileged_actor, or set train_cfg.runner.privileged_actor, to match the checkpoint)")
        mine = {"hidden_size": self.algorithm.actor_critic.rnn_hidden_size} if self.recurrent else None
        if loaded.get("recurrent") != mine:
            raise ValueError(f"{path} was saved with recurrent={loaded.get('recurrent')}, this runner has recurrent={mine}: the policy would not "
                             "be the one that was trained (pass --recurrent --rnn_hidden_size H, or set train_cfg.runner.policy_class_name / "
                             "train_cfg.policy.rnn_hidden_size, to match the checkpoint)")
        if loaded.get("noise") != self.noise:
            want = loaded.get("noise") or {"std_type": "scalar", "state_dependent": False}
            raise ValueError(f"{path} was saved with noise={loaded.get('noise')}, this runner has noise={self.noise}: the policy would not be "
                             f"the one that was trained (pass --noise_std_type {want['std_type']}"
                             f"{' --state_dependent_std' if want['state_dependent'] else ' without --state_dependent_std'}, or set "
                             "train_cfg.policy.noise_std_type / train_cfg.policy.state_dependent_std, to match the checkpoint)")
        if loaded.get("action_dist") != self.action_dist:   # (before any load_state_dict: its size error would not name the flag)
            theirs = loaded.get("action_dist")
            want = f"--action_dist {theirs['kind']} with the action box lo={theirs['lo']}, hi={theirs['hi']}" if theirs is not None \
                else "--action_dist gaussian, the default"
            raise ValueError(f"{path} was saved with action_dist={theirs}, this runner has action_dist={self.action_dist}: the policy would not be "
                             f"the one that was trained (pass {want}, or set train_cfg.policy.action_dist / action_bounds, to match the "
                             "checkpoint; the flag is --action_dist)")
        if loaded.get("layer_norm") != self.layer_norm:   # (before any load_state_dict: its key error would not name the flag)
            raise ValueError(f"{path} was saved with layer_norm={loaded.get('layer_norm')}, this runner has layer_norm={self.layer_norm}: the "
                             f"networks would not be the ones that were trained (pass {'--layer_norm' if 'layer_norm' in loaded else 'no --layer_norm'}"
                             ", or set train_cfg.policy.layer_norm, to match the checkpoint)")
        mine = dict(self.estimator.config) if self.estimator is not None else None
        theirs = dict(loaded["estimator"]["config"]) if "estimator" in loaded else None
        if theirs != mine:
            want = ("--estimator --estimator_targets " + ",".join(theirs["targets"]) + " --estimator_hidden_dims "
                    + " ".join(str(h) for h in theirs["hidden_dims"])) if theirs is not None else "no --estimator"
            raise ValueError(f"{path} was saved with estimator={theirs}, this runner has estimator={mine}: the policy's inputs would not be "
                             f"what it was trained on (pass {want}, or set train_cfg.runner.estimator / estimator_targets / "
                             "estimator_hidden_dims, to match the checkpoint)")
        mine = dict(self.cenet.config) if self.cenet is not None else None
        theirs = dict(loaded["cenet"]["config"]) if "cenet" in loaded else None
        if theirs != mine:
            want = ("--cenet --cenet_targets " + ",".join(theirs["targets"]) + f" --cenet_latent_dim {theirs['latent_dim']} --cenet_encoder_dims "
                    + " ".join(str(h) for h in theirs["encoder_dims"]) + " --cenet_decoder_dims "
                    + " ".join(str(h) for h in theirs["decoder_dims"])) if theirs is not None else "no --cenet"
            raise ValueError(f"{path} was saved with cenet={theirs}, this runner has cenet={mine}: the policy's inputs would not be what it "
                             f"was trained on (pass {want}, or set train_cfg.runner.cenet / cenet_targets / cenet_latent_dim / "
                             "cenet_encoder_dims / cenet_decoder_dims, to match the checkpoint)")
        if not self.inference_only:   # (play.py and the exported policy use the actor only)
            theirs = loaded["value_norm"]["mode"] if "value_norm" in loaded else None
            if theirs != self.value_norm:
                want = f"--value_norm {theirs}" if theirs is not None else "no --value_norm"
                raise ValueError(f"{path} was saved with value_norm={theirs!r}, this runner has value_norm={self.value_norm!r}: the critic's "
                                 f"output would not be in the units it was trained in (pass {want}, or set train_cfg.algorithm.value_norm, to "
                                 "match the checkpoint)")
            if _groups_key(loaded.get("multi_critic")) != _groups_key(self.multi_critic):   # (before any load_state_dict: its size error would not name the flag)
                theirs = loaded.get("multi_critic")
                want = ("--reward_groups \"" + ";".join(n + "=" + ",".join(t) for n, t in theirs["groups"].items()) + "\" --reward_group_weights "
                        + ",".join(str(x) for x in theirs["weights"])) if theirs is not None else "no --reward_groups"
                raise ValueError(f"{path} was saved with multi_critic={theirs}, this runner has multi_critic={self.multi_critic}: the critic's "
                                 f"heads would not be the ones that were trained (pass {want}, or set train_cfg.algorithm.reward_groups / "
                                 "reward_group_weights, to match the checkpoint)")
            theirs = loaded.get("constraints")
            if (None if theirs is None else theirs["spec"]) != (None if self.constraints is None else self.constraints["spec"]):
                if theirs is not None:
                    from .constraints import ConstraintSpec
                    want = f"--constraints \"{ConstraintSpec(theirs['spec']).text()}\""
                else:
                    want = "no --constraints"
                raise ValueError(f"{path} was saved with constraints={None if theirs is None else theirs['spec']}, this runner has constraints="
                                 f"{None if self.constraints is None else self.constraints['spec']}: the running column maxima would not be "
                                 f"the spec's (pass {want}, or set train_cfg.algorithm.constraints, to match the checkpoint; the flag is "
                                 "--constraints)")
        elif _groups_key(loaded.get("multi_critic")) != _groups_key(self.multi_critic):   # (the actor alone is used: the critic and the optimizer stay what they are)
            mine = self.algorithm.actor_critic.state_dict()
            loaded["model_state_dict"] = {k: (mine[k] if k.startswith("critic.") else v) for k, v in loaded["model_state_dict"].items()}
            load_optimizer = False
        saved_hist = loaded.get("obs_history", {"actor": 1, "critic": 1})   # (a checkpoint without the key: no history)
        if "distillation" in loaded and self.distillation is None:
            return self._load_student(path, loaded, saved_hist)
        if self.distillation is not None:
            self._check_distillation_checkpoint(path, loaded)
        if (saved_hist["actor"], saved_hist["critic"]) != (self.obs_history_length, self.critic_obs_history_length):
            raise ValueError(f"{path} was saved with --obs_history {saved_hist['actor']} --critic_obs_history {saved_hist['critic']}, this runner has "
                             f"--obs_history {self.obs_history_length} --critic_obs_history {self.critic_obs_history_length}: the policy's inputs "
                             "would not be what it was trained on (pass the checkpoint's values, or set train_cfg.runner.obs_history_length / "
                             "critic_obs_history_length)")
        if self.empirical_normalization:
            if self.obs_normalizer is not None:
                self.obs_normalizer.load_state_dict(loaded["obs_norm_state_dict"])
            if self.critic_obs_normalizer is not None:
                self.critic_obs_normalizer.load_state_dict(loaded["critic_obs_norm_state_dict"])
        self.algorithm.actor_critic.load_state_dict(loaded["model_state_dict"])
        self.algorithm.invalidate_graphs()
        if load_optimizer:
            self.algorithm.load_optimizer_state(loaded["optimizer_state_dict"])
        if self.rnd is not None and "rnd" in loaded:
            self.rnd.load_checkpoint(loaded["rnd"], load_optimizer)
        elif self.rnd is not None:
            print(f"{path} holds no rnd entry: random network distillation starts fresh")
        elif "rnd" in loaded:
            print(f"{path} holds an rnd entry, this runner has no --rnd: ignored")
        if self.estimator is not None:
            self.estimator.load_checkpoint(loaded["estimator"], load_optimizer)
        if self.cenet is not None:
            self.cenet.load_checkpoint(loaded["cenet"], load_optimizer)
        if self.constraints is not None and not self.inference_only:   # (c_max; the previous actions restart at zero)
            self.algorithm.constraints.load_checkpoint(loaded["constraints"])
        if self.value_norm is not None and "value_norm" in loaded and loaded["value_norm"]["mode"] == self.value_norm:
            self.algorithm.value_norm.load_checkpoint(loaded["value_norm"])
        self.current_learning_iteration = loaded["iter"]
        return loaded["infos"]

    def _check_distillation_checkpoint(self, path, loaded):
        """a distillation run resumes from a checkpoint of a distillation run with the same teacher only"""
        if "distillation" not in loaded:
            raise ValueError(f"{path} was not saved by a distillation run, this runner has distill_from={self.distill_from!r} "
                             "(drop --distill_from to load a PPO checkpoint)")
        if dict(loaded["distillation"]) != self.distillation:
            raise ValueError(f"{path} was saved with distillation={loaded['distillation']}, this runner has {self.distillation} "
                             "(pass the --distill_from / --distill_loss of the saved run)")
        mine, sd = self.algorithm.actor_critic.state_dict(), loaded["model_state_dict"]
        keys = [k for k in mine if k.startswith("teacher.")]
        if sorted(k for k in sd if k.startswith("teacher.")) != sorted(keys) or \
                any(sd[k].shape != mine[k].shape or not torch.equal(sd[k].to(mine[k].device), mine[k]) for k in keys):
            raise ValueError(f"{path} was distilled from another teacher than {self.distill_from} (its teacher.* tensors differ): "
                             "pass the --distill_from of the saved run")

    def _load_student(self, path, loaded, saved_hist):
        """a distilled checkpoint into an ordinary runner (play.py without --distill_from): the student's actor.*, std, the actor-side
        normaliser and history; the critic stays what it is, the optimizer state is skipped"""
        if saved_hist["actor"] != self.obs_history_length:
            raise ValueError(f"{path} was saved with --obs_history {saved_hist['actor']} --critic_obs_history {saved_hist['critic']}, this runner has "
                             f"--obs_history {self.obs_history_length} --critic_obs_history {self.critic_obs_history_length}: the policy's inputs "
                             "would not be what it was trained on (pass the checkpoint's values, or set train_cfg.runner.obs_history_length / "
                             "critic_obs_history_length)")
        if self.empirical_normalization:
            self.obs_normalizer.load_state_dict(loaded["obs_norm_state_dict"])
        ac, sd = self.algorithm.actor_critic, loaded["model_state_dict"]
        ac.actor.load_state_dict({k[len("actor."):]: v for k, v in sd.items() if k.startswith("actor.")})
        ac.assign_noise_std(sd["std"])
        memory = ""
        if self.recurrent:   # (load()'s "recurrent" check passed: the checkpoint holds a recurrent student of this hidden size)
            ac.memory_a.rnn.load_state_dict({k[len("memory_a.rnn."):]: v for k, v in sd.items() if k.startswith("memory_a.rnn.")})
            memory = ", the actor's memory"
        self.algorithm.invalidate_graphs()
        self.current_learning_iteration = loaded["iter"]
        print(f"{path} is a distilled checkpoint: loaded the student's actor{memory}, std and actor-side normaliser / history; the critic "
              f"{'and its memory are' if self.recurrent else 'is'} left as {'they are' if self.recurrent else 'it is'} and the optimizer state is "
              "skipped")
        return loaded["infos"]

    def _mean_actor(self):
        """the module whose output is the mean action: the actor, or the first A of its 2A outputs under state_dependent_std"""
        ac = self.algorithm.actor_critic
        return ac.inference_actor() if (self.state_dependent_std or self.action_dist is not None) else ac.actor

    def get_inference_policy(self, device=None):
        self.algorithm.actor_critic.eval()
        if device is not None:
            self.algorithm.actor_critic.to(device)
        policy = self.algorithm.actor_critic.act_inference
        if self.recurrent:   # raw frames in: a memory state of its own (policy.reset(dones) after every env.step, policy.reset_memory())
            norm = None
            if self.empirical_normalization:
                norm = self.obs_normalizer
                norm.eval()
                if device is not None:
                    norm.to(device)
            return RecurrentPolicy(self.algorithm.actor_critic, norm)
        if self.privileged_actor:   # raw single PRIVILEGED frames in: the critic's history length and statistics
            inner = self._mean_actor()
            if self.empirical_normalization:
                self.critic_obs_normalizer.eval()
                inner = NormalizedPolicy(inner, self.critic_obs_normalizer)
            return HistoryPolicy(inner, self.env.num_pri_obs, self.critic_obs_history_length).to(device if device is not None else self.device)
        if self.estimator is not None:   # raw SINGLE frames in: history, the statistics as they are now, then [x | est(x)] into the actor
            from .estimator import EstimatorPolicy
            self.estimator.net.eval()
            inner = EstimatorPolicy(self._mean_actor(), self.estimator.net)
            if self.empirical_normalization:
                self.obs_normalizer.eval()
                inner = NormalizedPolicy(inner, self.obs_normalizer)
            if self.obs_history_length > 1:
                inner = HistoryPolicy(inner, self.env.num_obs, self.obs_history_length)
            return inner.to(device if device is not None else self.device)
        if self.cenet is not None:   # raw SINGLE frames in: history, the statistics as they are now, then [x | v_hat | mu] into the actor
            from .cenet import CENetPolicy
            self.cenet.encoder.eval()
            inner = CENetPolicy(self._mean_actor(), self.cenet.encoder, self.cenet.num_outputs)
            if self.empirical_normalization:
                self.obs_normalizer.eval()
                inner = NormalizedPolicy(inner, self.obs_normalizer)
            if self.obs_history_length > 1:
                inner = HistoryPolicy(inner, self.env.num_obs, self.obs_history_length)
            return inner.to(device if device is not None else self.device)
        if self.empirical_normalization:   # raw observations in, as in training: normalised with the statistics as they are
            norm, act = self.obs_normalizer, self.algorithm.actor_critic.act_inference
            norm.eval()
            if device is not None:
                norm.to(device)
            policy = lambda x: act(norm(x))
        if self.obs_history_length > 1:   # raw SINGLE frames in: the policy keeps its own history (policy.reset(dones) after every env.step)
            inner = self._mean_actor()
            if self.empirical_normalization:   # (history first, then the statistics as they are now)
                inner = NormalizedPolicy(inner, self.obs_normalizer)
            policy = HistoryPolicy(inner, self.env.num_obs, self.obs_history_length).to(device if device is not None else self.device)
        return policy


def _groups_key(entry):
    """a checkpoint's "multi_critic" entry as something to compare: the groups IN ORDER (a group's position is its value head), the weights"""
    return None if entry is None else ([(n, list(t)) for n, t in entry["groups"].items()], [float(w) for w in entry["weights"]])


def train_state_path(model_path):
    """train_state_<it>.pt next to model_<it>.pt (no "model" in the name: get_load_path picks the last file containing it)"""
    d, name = os.path.split(model_path)
    return os.path.join(d, "train_state_" + name[len("model_"):] if name.startswith("model_") else "train_state_" + name)
