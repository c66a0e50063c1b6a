"""``torch.ops.ase_hip.*``: PyTorch custom operators over the C ABI of libase_hip.so (include/ase_hip.h).

This is the binding a maintainer of the reference adds to call the HIP kernels from ordinary PyTorch code: the
operators take / return ``torch.Tensor`` (device-resident), allocate their outputs with torch's allocator, launch on torch's
current HIP stream, never synchronise, and raise ``RuntimeError`` on bad shapes / dtypes / devices.  They are registered for
the CUDA (= HIP) dispatch key only: on CPU tensors PyTorch itself raises ``NotImplementedError`` - there is no fallback.

  linear_act(x, w, b, act) -> y                      fused Linear + activation (learning/ase_network_builder.py:255-259), MFMA GEMM;
                                                      differentiable: backward = linear_bwd_data + linear_bwd_weight, so an
                                                      autograd-based agent (the reference's own ``calc_gradients``) trains through it
  linear_bwd_data(dz, w) -> dx                       dz @ w
  linear_bwd_weight(dz, x) -> (gw, gb)               dz^T @ x, column sums of dz
  rms_update_normalize(x, state) -> y                RunningMeanStd.forward in train mode (state f64 [2 D + 1] updated in place)
  rms_normalize(x, state) -> y                       ... in eval mode
  rms_unnormalize(x, state) -> y                     RunningMeanStd(..., unnorm=True) on values
  gae(dones, values, next_values, rewards, gamma, tau) -> (advs, returns)         CommonAgent.discount_values (+ returns)
  masked_norm(returns, values, mask) -> advantages   AMPAgent._calc_advs (torch_ext.normalization_with_masks)
  gather_rows(src, idx) -> out                       AMPDataset._get_item
  disc_reward(logits, scale) / enc_reward(enc, z, scale)                          AMPAgent._calc_disc_rewards / ASEAgent._calc_enc_rewards
  normalize_rows(x) -> y                             torch.nn.functional.normalize(x, dim=-1)
  sample_latents(n, dim, rng_state) -> z             ASEBuilder.Network.sample_latents (Philox stream {seed, offset}, advanced)
  fused_adam_(w, g, m, v, opt_state)                 torch.optim.Adam.step on flat buffers (in place)
  ppo_loss_head(mu, value, actions, old_mu, old_sigma, old_neglogp, advantages, old_values, returns, mask, logstd, ...)
      -> (stats [6], d_mu, d_value)                   CommonAgent._actor_loss / _critic_loss / bound_loss + entropy, clip fraction, kl
                                                      (learning/common_agent.py:456-464,505-534) with the gradient of
                                                      actor_loss + bounds_coef bound_loss w.r.t. mu and of critic_coef critic_loss w.r.t. value
  ppo_loss_head_ls(..., logstd [M, A] | [A], ..., entropy_coef) -> (stats [6], d_mu, d_logstd, d_value)
                                                      the same with a learned log-std (rl_games learn_sigma): d_logstd per row
                                                      (- entropy_coef entropy included)
  disc_loss_gp(logits, grad_demo, disc_coef) -> (stats [4], d_logits)
                                                      AMPAgent._disc_loss' data terms (learning/amp_agent.py:442-459,481-496): BCE halves,
                                                      accuracies, the gradient penalty mean |d logit / d obs|^2, d loss / d logits
  enc_div_loss(enc_pred, enc_z, mu, mu_div, z, z_new, enc_coef, div_coef, div_tar)
      -> (stats [2], d_enc, d_mu, d_mu_div)            ASEAgent._enc_loss + _diversity_loss (learning/ase_agent.py:413-418,445-467)

  humanoid_obs_max(body_pos, body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs) -> obs [n, 15 B - 2]
                                                      compute_humanoid_observations_max (env/tasks/humanoid.py:592-636)
  humanoid_reset(progress_buf, contact_forces, body_pos, termination_heights, contact_body_ids, max_episode_length,
                 enable_early_termination, tar_contact_forces=None, strike_body_ids=None) -> (reset, terminated)
                                                      compute_humanoid_reset, plain and strike form
  task_obs(kind, root_states, ...) -> obs / task_reward(kind, n_envs, ...) -> reward
                                                      the observation / reward functions of humanoid_heading / _location / _reach / _strike
  task_reset(kind, ranges, steps_low, steps_high, enable_rand_heading, progress_buf, change_steps, root_states, tar_a, tar_b,
             tar_speed, tar_states, env_ids, u, steps, rng_state, advance=True) -> ()
                                                      (change_steps, tar_a, tar_b, tar_speed, tar_states, rng_state written in place)
                                                      _reset_task / _update_task of humanoid_heading / _location / _reach and
                                                      HumanoidStrike._reset_target: new targets and change steps in one launch
  proj_launch(root_states, body_pos, body_vel, proj_states, progress_buf, timesteps, slot, env_ids, u, eps, rng_state, advance,
              tar_body, ranges, noise, slot_out, ids_out, draws_out) -> ()
                                                      (proj_states, rng_state and the three exports written in place)
                                                      HumanoidPerturb._update_proj: the schedule test on progress_buf[0], the
                                                      draws and the projectile's root-state row in one launch
                                                      (env/tasks/humanoid_perturb.py:172-213)
  motion_sync(mode, motion_ids, progress_buf, reset_buf, terminate_buf, motion_dt, root_states, dof_pos, dof_vel, body_pos,
              body_rot, body_vel, body_ang_vel, env_ids, ids_out, gts, grs, lrs, lengths, num_frames, clip_dt, length_starts,
              dof_body_ids, dof_offsets) -> ()        (the four buffers, the state tensors and ids_out written in place)
                                                      HumanoidViewMotion._motion_sync + compute_view_motion_reset ('sync') and
                                                      _reset_env_tensors ('reset') in one launch each
                                                      (env/tasks/humanoid_view_motion.py:44-97)
  latent_renew(latents, env_ids, eps, steps, rng_state, advance, progress_buf, reset_steps, steps_add, steps_low, steps_high, z2) -> ()
                                                      (latents, reset_steps, rng_state, z2 written in place)
                                                      ASEAgent._reset_latents + _reset_latent_step_count / _update_latents and
                                                      the step's ase_latents copy (learning/ase_agent.py:310-379) in one launch
  amp_reset(root_states, dof_pos, dof_vel, hist, body_pos, body_rot, body_vel, body_ang_vel, env_ids, kind, motion_ids,
            motion_times, src_rows, clip tensors ..., tab_root_states, tab_dof_pos, tab_dof_vel, dof_body_ids, dof_offsets,
            key_body_ids, local_root_obs, root_height_obs, env_dt) -> ()      (root_states, dof_pos, dof_vel, hist written in place)
                                                      HumanoidAMP._reset_actors + _init_amp_obs, the get-up task's fall episodes
                                                      (env/tasks/humanoid_amp.py:141-246, humanoid_amp_getup.py:109-129)
  amp_reset_due(root_states, dof_pos, dof_vel, hist, body_pos, body_rot, body_vel, body_ang_vel, reset_buf, rng_state,
                progress_buf, terminate_buf, recovery_counter, env_ids_out, kind_out, motion_ids_out, motion_times_out,
                src_rows_out, clip tensors ..., clip_cdf, tab_root_states, tab_dof_pos, tab_dof_vel, dof_body_ids, dof_offsets,
                key_body_ids, state_init, hybrid_init_prob, getup, recovery_episode_prob, recovery_steps, fall_init_prob,
                local_root_obs, root_height_obs, env_dt, advance=True) -> ()
                                                      (state, hist, the three buffers, the counter, rng_state and the plan
                                                      outputs written in place) the same resets for every environment with
                                                      reset_buf != 0: due test, draws (Philox stream {seed, offset}), apply and
                                                      _reset_env_tensors in one launch (humanoid_amp.py:132-201,
                                                      humanoid_amp_getup.py:78-114, humanoid.py:165-167)
  amp_demo_fetch(out, ring_rows, head, n, num_steps, truncate_time, dt, motion_ids, motion_times0, rng_state, clip_cdf,
                 motion_ids_out, motion_times0_out, clip tensors ..., dof_body_ids, dof_offsets, key_body_ids, local_root_obs,
                 root_height_obs, advance=True, head_dev=None) -> ()
                                                      (out, rng_state and the draw outputs written in place) the demo fetch:
                                                      draws (passed in, or the Philox stream {seed, offset}), motion sampler,
                                                      frames and the store into the demo ring in one launch
                                                      (env/tasks/humanoid_amp.py:63-105)
  rollout_store(dones, slot, n_slots, srcs, dsts, rewards, shift, scale, rewards_out, dones_out, next_values, terminate,
                next_values_out, cur_rewards, cur_lengths, meter, max_size, done_ids_out, slot_dev=None) -> ()
                                                      (dsts, the three slotted outputs, the accumulators, the meter and the id
                                                      list written in place) one environment step into experience slot `slot`:
                                                      what play_steps does behind env_step, without dones.nonzero
                                                      (learning/common_agent.py:267-293)
  rollout_head(obs, z, mean, std, xa, xc, zc, zs, obses_out, z_out, slot, slot_dev=None) -> ()
                                                      (the six outputs written in place) the head of one environment step in
                                                      one launch: the obses / latents store into experience slot `slot`, the
                                                      eval-mode normalisation into the actor's and critic's inputs and the
                                                      latents' conversion into the concat block and the style input
                                                      (learning/common_agent.py:253-262)
  word_step(word, add, wrap) -> ()                    (word written in place) word = (word + add) mod wrap on the device: the
                                                      step counter of a recorded rollout step
  hrl_latent(actions) -> z                            F.normalize(torch.clamp(actions, -1, 1), dim=-1): the latent a high-level
                                                      action selects, once per high-level step (learning/hrl_agent.py:89-93,235)
  hrl_llc_action(mu, low, high, act, clip) -> a       the LLC's padded head output -> the environment's action: clamp and
                                                      rl_games rescale_actions (ASEAgent.preprocess_actions, hrl_agent.py:238)
  hrl_accum(rewards, dones, terminate, logit, disc_scale, acc, first, last, llc_steps, rewards_out, disc_out, dones_out,
            terminate_out) -> ()                      (acc and, with last, the four outputs written in place) one inner step's
                                                      task reward, discriminator reward and done / terminate counts folded into
                                                      the running sums; the means and masks at the end (hrl_agent.py:57-73)
  env_pre_step(actions_in, actions, targets, clip_actions, pd_offset, pd_scale, motor_efforts, power_scale, root_states,
               prev_root_pos, recovery_counter) -> () (actions, targets, prev_root_pos, recovery_counter written in place) the
                                                      pre_physics_step chain: action clamp and copy, PD targets or forces, the
                                                      previous root position, the recovery counter (humanoid.py:361-366,479-481)
  env_post_step(body_pos, ..., key_body_ids) -> ()    (progress_buf, obs, reward, reset, terminated, hist written in place)
                                                      Humanoid.post_physics_step + HumanoidAMP.post_physics_step on state read
                                                      in place at its own strides (humanoid.py:368-383, humanoid_amp.py:50-59)
  clip_frames(rotation, root_translation, root_velocity, root_angular_velocity, local_translation, clip_first, clip_num_frames,
              clip_fps, frame_clip, parent_indices, dof_body_ids, dof_offsets) -> (gts, grs, lrs, grvs, gravs, dvs)
                                                      the clip loader: forward kinematics and joint velocities of every frame of
                                                      every clip (MotionLib._load_motions, utils/motion_lib.py:174-236,279-294)
  retarget_fk / retarget_chain / retarget_pose / retarget_hinge / retarget_ground / retarget_finish / retarget_velocity
                                                      the launches of ase_amd.retarget.Retargeter, operands as the backend
                                                      methods of the same names (poselib retarget_to, project_joints, grounding,
                                                      from_skeleton_state); every operand a device tensor

``HipLinear`` is an ``nn.Linear`` whose forward is ``linear_act`` (optionally with a fused ReLU / tanh).
"""
import torch
import torch.nn as nn

from . import lib as L

_ACT = {'none': L.ACT_NONE, 'None': L.ACT_NONE, 'relu': L.ACT_RELU, 'tanh': L.ACT_TANH}
_be = None


def _backend():
    global _be
    if _be is None:
        from .backend import HipBackend
        _be = HipBackend(torch.device('cuda', torch.cuda.current_device()))
    return _be


def _check(cond, msg):
    if not cond:
        raise RuntimeError('ase_hip: ' + msg)


def _P(x, m):
    return (int(x) + m - 1) // m * m


def _padded(x, cols, dtype=None):
    """Contiguous copy of x [R, C] with the row length padded to `cols` (zeros)."""
    dtype = x.dtype if dtype is None else dtype
    if x.shape[1] == cols and x.is_contiguous() and x.dtype == dtype:
        return x
    out = torch.zeros(x.shape[0], cols, dtype=dtype, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def _gemm_dtype(x):
    _check(x.dtype in (torch.bfloat16, torch.float16, torch.float32), f'matrix operands must be bf16, f16 or f32, got {x.dtype}')
    return x.dtype


def _kpad(k, dtype):
    return _P(k, 32 if dtype in (torch.bfloat16, torch.float16) else 16)          # whole 64-byte K steps


# ------------------------------------------------------------------------------------------------ dense layers
@torch.library.custom_op('ase_hip::linear_act', mutates_args=(), device_types='cuda')
def linear_act(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, act: str) -> torch.Tensor:
    _check(x.dim() == 2 and w.dim() == 2 and x.shape[1] == w.shape[1], 'linear_act: x [M, K], w [N, K]')
    _check(act in _ACT, f'linear_act: activation {act!r} (none | relu | tanh)')
    dt = _gemm_dtype(x)
    M, K = x.shape
    N = w.shape[0]
    kp, npad = _kpad(K, dt), _P(N, 64)
    xs, ws = _padded(x, kp), _padded(w.to(dt), kp)
    if npad != N:
        ws = torch.cat([ws, torch.zeros(npad - N, kp, dtype=dt, device=x.device)])
    bs = torch.zeros(npad, dtype=torch.float32, device=x.device)
    bs[:N] = b.float()
    y = torch.empty(M, npad, dtype=dt, device=x.device)
    _backend().gemm_nt(xs, ws, y, M, npad, kp, bias=bs, act=_ACT[act])
    return y[:, :N].contiguous() if npad != N else y


@linear_act.register_fake
def _(x, w, b, act):
    return x.new_empty(x.shape[0], w.shape[0])


@torch.library.custom_op('ase_hip::linear_bwd_data', mutates_args=(), device_types='cuda')
def linear_bwd_data(dz: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    _check(dz.dim() == 2 and w.dim() == 2 and dz.shape[1] == w.shape[0], 'linear_bwd_data: dz [M, N], w [N, K]')
    dt = _gemm_dtype(dz)
    M, N = dz.shape
    K = w.shape[1]
    npad, kout = _kpad(N, dt), _P(K, 64)
    wt = _padded(w.to(dt).t(), npad)                               # [K, N]: the contraction dim contiguous in both operands
    if kout != K:
        wt = torch.cat([wt, torch.zeros(kout - K, npad, dtype=dt, device=dz.device)])
    dx = torch.empty(M, kout, dtype=dt, device=dz.device)
    _backend().gemm_nt(_padded(dz, npad), wt, dx, M, kout, npad)
    return dx[:, :K].contiguous() if kout != K else dx


@linear_bwd_data.register_fake
def _(dz, w):
    return dz.new_empty(dz.shape[0], w.shape[1])


@torch.library.custom_op('ase_hip::linear_bwd_weight', mutates_args=(), device_types='cuda')
def linear_bwd_weight(dz: torch.Tensor, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    _check(dz.dim() == 2 and x.dim() == 2 and dz.shape[0] == x.shape[0], 'linear_bwd_weight: dz [M, N], x [M, K]')
    dt = _gemm_dtype(dz)
    _check(x.dtype == dt, 'linear_bwd_weight: dz and x must have the same dtype')
    M, N = dz.shape
    K = x.shape[1]
    el = 8 if dt in (torch.bfloat16, torch.float16) else 4
    npad, kp = _P(N, el), _P(K, el)
    gw = torch.zeros(N, K, dtype=torch.float32, device=dz.device)
    gb = torch.zeros(N, dtype=torch.float32, device=dz.device)
    _backend().gemm_tn(_padded(dz, npad), _padded(x, kp), gw, M, npad, kp, N, K, K, K, gbias=gb)
    return gw, gb


@linear_bwd_weight.register_fake
def _(dz, x):
    return dz.new_empty(dz.shape[1], x.shape[1], dtype=torch.float32), dz.new_empty(dz.shape[1], dtype=torch.float32)


def _linear_setup(ctx, inputs, output):
    x, w, b, act = inputs
    ctx.act = act
    ctx.save_for_backward(x, w, output)


def _linear_backward(ctx, dy):
    x, w, y = ctx.saved_tensors
    dy = dy.contiguous()
    if ctx.act == 'relu':
        dz = dy * (y > 0).to(dy.dtype)
    elif ctx.act == 'tanh':
        dz = dy * (1 - y.float() * y.float()).to(dy.dtype)
    else:
        dz = dy
    dz = dz.to(x.dtype)
    dx = linear_bwd_data(dz, w) if ctx.needs_input_grad[0] else None
    gw, gb = linear_bwd_weight(dz, x)
    return dx, gw.to(w.dtype), gb, None


linear_act.register_autograd(_linear_backward, setup_context=_linear_setup)


class HipLinear(nn.Linear):
    """nn.Linear (same parameters / state_dict) whose forward is ase_hip::linear_act with a fused activation."""

    def __init__(self, in_features, out_features, activation='none', compute_dtype=torch.bfloat16, **kw):
        super().__init__(in_features, out_features, **kw)
        self.activation, self.compute_dtype = activation, compute_dtype

    def forward(self, x):
        shp = x.shape
        y = linear_act(x.reshape(-1, shp[-1]).to(self.compute_dtype), self.weight, self.bias, self.activation)
        return y.reshape(*shp[:-1], -1).to(x.dtype)


# ------------------------------------------------------------------------------------------------ normaliser
def _rms(x, state, update):
    _check(x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous(), 'rms: x must be a contiguous f32 [M, D] tensor')
    M, D = x.shape
    _check(state.dtype == torch.float64 and state.numel() == 2 * D + 1, 'rms: state must be f64 [2 D + 1] = mean | var | count')
    be = _backend()
    mean = torch.empty(1, D, dtype=torch.float32, device=x.device)
    std = torch.empty(1, D, dtype=torch.float32, device=x.device)
    if update:
        sums = torch.zeros(2 * D, dtype=torch.float64, device=x.device)
        be.rms_moments(x, D, None, (0, 0), M, state, sums)
        be.rms_finalize(state, D, sums, M, 1, mean, std)
    else:
        be.rms_finalize(state, D, None, 0, 0, mean, std)
    y = torch.empty_like(x)
    be.rms_normalize(x, D, None, (0, 0), M, mean[0], std[0], [y])
    return y


@torch.library.custom_op('ase_hip::rms_update_normalize', mutates_args=('state',), device_types='cuda')
def rms_update_normalize(x: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    return _rms(x, state, True)


@rms_update_normalize.register_fake
def _(x, state):
    return torch.empty_like(x)


@torch.library.custom_op('ase_hip::rms_normalize', mutates_args=(), device_types='cuda')
def rms_normalize(x: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    return _rms(x, state, False)


@rms_normalize.register_fake
def _(x, state):
    return torch.empty_like(x)


@torch.library.custom_op('ase_hip::rms_unnormalize', mutates_args=(), device_types='cuda')
def rms_unnormalize(x: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    _check(x.dtype == torch.float32 and x.is_contiguous() and state.dtype == torch.float64 and state.numel() == 3,
           'rms_unnormalize: x f32 contiguous, state f64 [3]')
    y = torch.empty_like(x)
    _backend().rms_unnormalize(state, x, y)
    return y


@rms_unnormalize.register_fake
def _(x, state):
    return torch.empty_like(x)


# ------------------------------------------------------------------------------------------------ rollout tail
@torch.library.custom_op('ase_hip::gae', mutates_args=(), device_types='cuda')
def gae(dones: torch.Tensor, values: torch.Tensor, next_values: torch.Tensor, rewards: torch.Tensor, gamma: float,
        tau: float) -> tuple[torch.Tensor, torch.Tensor]:
    _check(rewards.dim() == 3 and rewards.shape[2] == 1 and values.shape == rewards.shape and next_values.shape == rewards.shape,
           'gae: values / next_values / rewards must be [H, N, 1]')
    H, N = rewards.shape[0], rewards.shape[1]
    advs, rets = torch.empty_like(rewards), torch.empty_like(rewards)
    _backend().gae(dones.to(torch.uint8).contiguous(), values.contiguous(), next_values.contiguous(), rewards.contiguous(),
                   None, None, 1.0, 0.0, 0.0, gamma, tau, advs, rets, H, N)
    return advs, rets


@gae.register_fake
def _(dones, values, next_values, rewards, gamma, tau):
    return torch.empty_like(rewards), torch.empty_like(rewards)


@torch.library.custom_op('ase_hip::masked_norm', mutates_args=(), device_types='cuda')
def masked_norm(returns: torch.Tensor, values: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    n = returns.numel()
    _check(values.numel() == n and mask.numel() == n, 'masked_norm: returns / values / mask must have the same number of rows')
    be = _backend()
    adv = torch.empty(n, 1, dtype=torch.float32, device=returns.device)
    acc3 = torch.zeros(3, dtype=torch.float64, device=returns.device)
    r, v, m = returns.reshape(n, 1).contiguous(), values.reshape(n, 1).contiguous(), mask.reshape(n, 1).float().contiguous()
    be.adv_norm(r, v, m, adv, acc3, n, True, 0)
    be.adv_norm(r, v, m, adv, acc3, n, True, 1)
    return adv.view(-1)


@masked_norm.register_fake
def _(returns, values, mask):
    return returns.new_empty(returns.numel())


@torch.library.custom_op('ase_hip::gather_rows', mutates_args=(), device_types='cuda')
def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _check(src.dim() == 2 and src.dtype == torch.float32 and idx.dtype == torch.int32, 'gather_rows: src f32 [R, D], idx int32 [M]')
    out = torch.empty(idx.numel(), src.shape[1], dtype=torch.float32, device=src.device)
    _backend().gather_rows(src, src.shape[1], idx.contiguous(), (0, 0), idx.numel(), out)
    return out


@gather_rows.register_fake
def _(src, idx):
    return src.new_empty(idx.numel(), src.shape[1])


@torch.library.custom_op('ase_hip::disc_reward', mutates_args=(), device_types='cuda')
def disc_reward(logits: torch.Tensor, scale: float) -> torch.Tensor:
    lg = logits.reshape(-1, 1).float().contiguous()
    r = torch.empty_like(lg)
    _backend().disc_reward(lg, r, lg.shape[0], scale)
    return r.view(logits.shape)


@disc_reward.register_fake
def _(logits, scale):
    return torch.empty_like(logits, dtype=torch.float32)


@torch.library.custom_op('ase_hip::enc_reward', mutates_args=(), device_types='cuda')
def enc_reward(enc: torch.Tensor, z: torch.Tensor, scale: float) -> torch.Tensor:
    _check(enc.shape == z.shape and enc.dim() == 2, 'enc_reward: enc and z must be [n, z_dim]')
    n, D = enc.shape
    r = torch.empty(n, 1, dtype=torch.float32, device=enc.device)
    _backend().enc_reward(enc.float().contiguous(), z.float().contiguous(), r, n, D, scale)
    return r


@enc_reward.register_fake
def _(enc, z, scale):
    return enc.new_empty(enc.shape[0], 1, dtype=torch.float32)


@torch.library.custom_op('ase_hip::normalize_rows', mutates_args=(), device_types='cuda')
def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    _check(x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] <= 128, 'normalize_rows: x f32 [n, d <= 128]')
    xc = x.contiguous()
    y = torch.empty_like(xc)
    _backend().normalize_rows(xc, y, xc.shape[0], xc.shape[1])
    return y


@normalize_rows.register_fake
def _(x):
    return torch.empty_like(x)


@torch.library.custom_op('ase_hip::sample_latents', mutates_args=('rng_state',), device_types='cuda')
def sample_latents(n: int, dim: int, rng_state: torch.Tensor) -> torch.Tensor:
    _check(rng_state.dtype == torch.int64 and rng_state.numel() == 2, 'sample_latents: rng_state int64 [2] = seed | offset')
    z = torch.empty(n, dim, dtype=torch.float32, device=rng_state.device)
    _backend().sample_latents(z, n, dim, rng_state)
    return z


@sample_latents.register_fake
def _(n, dim, rng_state):
    return rng_state.new_empty(n, dim, dtype=torch.float32)


@torch.library.custom_op('ase_hip::fused_adam_', mutates_args=('w', 'm', 'v', 'opt_state'), device_types='cuda')
def fused_adam_(w: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, opt_state: torch.Tensor) -> None:
    """opt_state: f64 [8] = step, lr, beta1, beta2, eps, bias_corr1, bias_corr2, _ (the step is advanced here)."""
    _check(all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == w.numel() for t in (w, g, m, v)),
           'fused_adam_: w / g / m / v must be contiguous f32 buffers of one size')
    _check(opt_state.dtype == torch.float64 and opt_state.numel() == 8, 'fused_adam_: opt_state f64 [8]')
    be = _backend()
    be.begin_step(opt_state, None)
    be.adam(w.view(-1), g.view(-1), m.view(-1), v.view(-1), opt_state)


# ------------------------------------------------------------------------------------------------ loss heads
def _f32c(t, name, cols=None):
    _check(t.dtype == torch.float32 and t.is_cuda, f'{name}: f32 device tensor expected')
    t = t.contiguous()
    _check(cols is None or (t.dim() == 2 and t.shape[1] == cols), f'{name}: expected [rows, {cols}], got {tuple(t.shape)}')
    return t


@torch.library.custom_op('ase_hip::ppo_loss_head', mutates_args=(), device_types='cuda')
def ppo_loss_head(mu: torch.Tensor, value: torch.Tensor, actions: torch.Tensor, old_mu: torch.Tensor, old_sigma: torch.Tensor,
                  old_neglogp: torch.Tensor, advantages: torch.Tensor, old_values: torch.Tensor, returns: torch.Tensor,
                  mask: torch.Tensor, logstd: torch.Tensor, e_clip: float, critic_coef: float, bounds_coef: float,
                  clip_value: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PPO loss head of one minibatch (learning/common_agent.py:505-534,456-464; rl_games neglogp / policy_kl):
    stats = [actor_loss, critic_loss, bound_loss, entropy, clip_fraction, kl] as the reference reports them (mask: an EMPTY tensor ->
    plain means; else the AMP / ASE masked means sum(mask x) / sum(mask) of learning/amp_agent.py:316-324), d_mu = d (actor_loss +
    bounds_coef bound_loss) / d mu, d_value = d (critic_coef critic_loss) / d value.  One launch of ase_hip_ppo_head; nothing
    synchronises (the statistics are formed from the device accumulators by tensor operations)."""
    M, A = mu.shape
    _check(mu.dim() == 2 and 1 <= A <= 64, 'ppo_loss_head: mu [M, actions <= 64]')
    be, dev = _backend(), mu.device
    mu, value = _f32c(mu, 'mu'), _f32c(value.reshape(M, 1), 'value')
    masked = mask.numel() > 0
    mb = {'actions': _f32c(actions, 'actions', A), 'mu': _f32c(old_mu, 'old_mu', A), 'sigma': _f32c(old_sigma, 'old_sigma', A),
          'old_logp_actions': _f32c(old_neglogp.reshape(M, 1), 'old_neglogp'), 'advantages': _f32c(advantages.reshape(M, 1), 'advantages'),
          'old_values': _f32c(old_values.reshape(M, 1), 'old_values'), 'returns': _f32c(returns.reshape(M, 1), 'returns')}
    acc = torch.zeros(L.ACC_COUNT, dtype=torch.float64, device=dev)
    if masked:
        mb['rand_action_mask'] = _f32c(mask.reshape(M, 1).float(), 'mask')
        be.reduce_sum(mb['rand_action_mask'], M, False, acc, L.ACC_MASK_SUM)
    d_mu, d_value = torch.zeros(M, A, dtype=torch.float32, device=dev), torch.zeros(M, 1, dtype=torch.float32, device=dev)
    be.ppo_head(mu, value, mb, None, _f32c(logstd.reshape(-1), 'logstd'), d_mu, d_value, None, None, acc, M, M, A, 0, masked, False,
                False, bool(clip_value), e_clip, critic_coef, bounds_coef, 0.0, 0.0)
    den = acc[L.ACC_MASK_SUM] if masked else float(M)
    stats = torch.stack([acc[L.ACC_A_LOSS] / den, acc[L.ACC_C_LOSS] / M, acc[L.ACC_B_LOSS] / den, acc[L.ACC_ENTROPY] / den,
                         acc[L.ACC_CLIPPED] / den, acc[L.ACC_KL] / M]).float()
    return stats, d_mu, d_value


@ppo_loss_head.register_fake
def _(mu, value, actions, old_mu, old_sigma, old_neglogp, advantages, old_values, returns, mask, logstd, e_clip, critic_coef,
      bounds_coef, clip_value):
    return mu.new_empty(6), torch.empty_like(mu), mu.new_empty(mu.shape[0], 1)


@torch.library.custom_op('ase_hip::ppo_loss_head_ls', mutates_args=(), device_types='cuda')
def ppo_loss_head_ls(mu: torch.Tensor, value: torch.Tensor, actions: torch.Tensor, old_mu: torch.Tensor, old_sigma: torch.Tensor,
                     old_neglogp: torch.Tensor, advantages: torch.Tensor, old_values: torch.Tensor, returns: torch.Tensor,
                     mask: torch.Tensor, logstd: torch.Tensor, e_clip: float, critic_coef: float, bounds_coef: float,
                     clip_value: bool, entropy_coef: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ppo_loss_head with a LEARNED log-std (rl_games learn_sigma): logstd is the state-independent vector [A] (fixed_sigma) or
    the per-row output of the sigma head [M, A].  The loss gains - entropy_coef x entropy; d_logstd [M, A] = d (actor_loss +
    bounds_coef bound_loss - entropy_coef entropy) / d logstd per row (the KL takes sigma detached, as the reference's does).
    The vector's gradient is d_logstd.sum(0).  Returns (stats [6], d_mu, d_logstd, d_value)."""
    M, A = mu.shape
    _check(mu.dim() == 2 and 1 <= A <= 64, 'ppo_loss_head_ls: mu [M, actions <= 64]')
    rows = logstd.dim() == 2
    _check(tuple(logstd.shape) in ((M, A), (A,)), 'ppo_loss_head_ls: logstd [M, actions] or [actions]')
    be, dev = _backend(), mu.device
    mu, value = _f32c(mu, 'mu'), _f32c(value.reshape(M, 1), 'value')
    masked = mask.numel() > 0
    mb = {'actions': _f32c(actions, 'actions', A), 'mu': _f32c(old_mu, 'old_mu', A), 'sigma': _f32c(old_sigma, 'old_sigma', A),
          'old_logp_actions': _f32c(old_neglogp.reshape(M, 1), 'old_neglogp'), 'advantages': _f32c(advantages.reshape(M, 1), 'advantages'),
          'old_values': _f32c(old_values.reshape(M, 1), 'old_values'), 'returns': _f32c(returns.reshape(M, 1), 'returns')}
    acc = torch.zeros(L.ACC_COUNT, dtype=torch.float64, device=dev)
    if masked:
        mb['rand_action_mask'] = _f32c(mask.reshape(M, 1).float(), 'mask')
        be.reduce_sum(mb['rand_action_mask'], M, False, acc, L.ACC_MASK_SUM)
    f32 = dict(dtype=torch.float32, device=dev)
    d_mu, d_value, d_ls = torch.zeros(M, A, **f32), torch.zeros(M, 1, **f32), torch.zeros(M, A, **f32)
    ls = _f32c(logstd, 'logstd', A) if rows else _f32c(logstd, 'logstd')
    be.ppo_head(mu, value, mb, None, ls, d_mu, d_value, None, None, acc, M, M, A, 0, masked, False,
                False, bool(clip_value), e_clip, critic_coef, bounds_coef, 0.0, 0.0,
                ls_mode=L.LS_ROWS if rows else L.LS_VECTOR, d_logstd=d_ls, entropy_coef=entropy_coef)
    den = acc[L.ACC_MASK_SUM] if masked else float(M)
    stats = torch.stack([acc[L.ACC_A_LOSS] / den, acc[L.ACC_C_LOSS] / M, acc[L.ACC_B_LOSS] / den, acc[L.ACC_ENTROPY] / den,
                         acc[L.ACC_CLIPPED] / den, acc[L.ACC_KL] / M]).float()
    return stats, d_mu, d_ls, d_value


@ppo_loss_head_ls.register_fake
def _(mu, value, actions, old_mu, old_sigma, old_neglogp, advantages, old_values, returns, mask, logstd, e_clip, critic_coef,
      bounds_coef, clip_value, entropy_coef):
    return mu.new_empty(6), torch.empty_like(mu), torch.empty_like(mu), mu.new_empty(mu.shape[0], 1)


@torch.library.custom_op('ase_hip::disc_loss_gp', mutates_args=(), device_types='cuda')
def disc_loss_gp(logits: torch.Tensor, grad_demo: torch.Tensor, disc_coef: float) -> tuple[torch.Tensor, torch.Tensor]:
    """Discriminator loss head (learning/amp_agent.py:442-459,481-496).  logits [3 n, 1]: rows [0, 2 n) agent + replay (target 0),
    rows [2 n, 3 n) demo (target 1); grad_demo [n, D] = d logit / d (demo observation), from autograd or the engine's chain (an EMPTY
    tensor skips the penalty).  stats = [0.5 (BCE_agent + BCE_demo), gradient penalty = mean_rows |grad|^2, agent accuracy, demo
    accuracy]; d_logits = disc_coef x d (0.5 (BCE_agent + BCE_demo)) / d logits."""
    R = logits.shape[0]
    _check(logits.dim() == 2 and logits.shape[1] == 1 and R % 3 == 0, 'disc_loss_gp: logits [3 n, 1]')
    n, dev, be = R // 3, logits.device, _backend()
    lg = _f32c(logits, 'logits')
    acc = torch.zeros(L.ACC_COUNT, dtype=torch.float64, device=dev)
    d_logit = torch.zeros(R, 1, dtype=torch.float32, device=dev)
    be.disc_head(lg, d_logit, None, acc, n, n, disc_coef)
    if grad_demo.numel():
        g = _f32c(grad_demo, 'grad_demo')
        _check(g.dim() == 2 and g.shape[0] == n, 'disc_loss_gp: grad_demo [n, D]')
        be.sqnorm(g, n, g.shape[1], acc, L.ACC_GP, scale=1.0)
    stats = torch.stack([0.5 * (acc[L.ACC_BCE_AGENT] / (2 * n) + acc[L.ACC_BCE_DEMO] / n), acc[L.ACC_GP] / n,
                         acc[L.ACC_AGENT_ACC] / (2 * n), acc[L.ACC_DEMO_ACC] / n]).float()
    return stats, d_logit


@disc_loss_gp.register_fake
def _(logits, grad_demo, disc_coef):
    return logits.new_empty(4), torch.empty_like(logits)


@torch.library.custom_op('ase_hip::enc_div_loss', mutates_args=(), device_types='cuda')
def enc_div_loss(enc_pred: torch.Tensor, enc_z: torch.Tensor, mu: torch.Tensor, mu_div: torch.Tensor, z: torch.Tensor,
                 z_new: torch.Tensor, enc_coef: float, div_coef: float,
                 div_tar: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ASE's two extra loss heads (learning/ase_agent.py:413-418,445-467).  enc_pred [n, Z] = the encoder's PRE-normalisation output,
    enc_z [n, Z] the latents of those rows: enc_loss = mean(-<normalize(enc_pred), enc_z>), d_enc = enc_coef x its gradient.
    mu / mu_div [M, A] = the actor's means under the rollout's latents z [M, Z] and under fresh ones z_new [M, Z]:
    diversity loss = mean((div_tar - |clamp(mu) - clamp(mu_div)|^2 / A / (0.5 - 0.5 <z_new, z> + 1e-5))^2), d_mu / d_mu_div =
    div_coef x its gradients.  stats = [enc_loss, diversity_loss]."""
    n, Z = enc_pred.shape
    M, A = mu.shape
    _check(enc_z.shape == enc_pred.shape and Z <= 128, 'enc_div_loss: enc_pred / enc_z [n, Z <= 128]')
    _check(mu_div.shape == mu.shape and z.shape == (M, Z) and z_new.shape == (M, Z) and A <= 64, 'enc_div_loss: mu / mu_div [M, A], z / z_new [M, Z]')
    be, dev = _backend(), mu.device
    f32 = dict(dtype=torch.float32, device=dev)
    acc = torch.zeros(L.ACC_COUNT, dtype=torch.float64, device=dev)
    d_enc = torch.zeros(n, Z, **f32)
    be.enc_head(_f32c(enc_pred, 'enc_pred'), _f32c(enc_z, 'enc_z'), d_enc, None, None, acc, n, n, Z, enc_coef)
    # the diversity term rides in ase_hip_ppo_head's launch: with zero advantages, zero critic / bound coefficients its other terms vanish
    mu2 = torch.cat([_f32c(mu, 'mu'), _f32c(mu_div, 'mu_div')])
    zeros1, ones = torch.zeros(M, 1, **f32), torch.ones(M, A, **f32)
    mb = {'actions': mu2[:M], 'mu': mu2[:M], 'sigma': ones, 'old_logp_actions': zeros1, 'advantages': zeros1, 'old_values': zeros1,
          'returns': zeros1, 'ase_latents': _f32c(z, 'z')}
    d_mu2, d_v = torch.zeros(2 * M, A, **f32), torch.zeros(M, 1, **f32)
    be.ppo_head(mu2, zeros1, mb, _f32c(z_new, 'z_new'), torch.zeros(A, **f32), d_mu2, d_v, None, None, acc, M, M, A, Z, False, True,
                False, False, 0.2, 0.0, 0.0, div_coef, div_tar)
    stats = torch.stack([acc[L.ACC_ENC] / n, acc[L.ACC_DIV] / M]).float()
    return stats, d_enc, d_mu2[:M].clone(), d_mu2[M:].clone()          # (clones: a custom operator's outputs must not alias each other)


@enc_div_loss.register_fake
def _(enc_pred, enc_z, mu, mu_div, z, z_new, enc_coef, div_coef, div_tar):
    return mu.new_empty(2), torch.empty_like(enc_pred), torch.empty_like(mu), torch.empty_like(mu)


# ---- environment side: functional forms of the tensor functions a task runs every simulator step ----
_TASKS = {'heading': L.TASK_HEADING, 'location': L.TASK_LOCATION, 'reach': L.TASK_REACH, 'strike': L.TASK_STRIKE}


def _task_kind(kind):
    _check(kind in _TASKS, f"task kind must be one of {sorted(_TASKS)}, got {kind!r}")
    return _TASKS[kind]


def _opt_f32c(t, name):
    return None if t is None else _f32c(t, name)


@torch.library.custom_op('ase_hip::humanoid_obs_max', mutates_args=(), device_types='cuda')
def humanoid_obs_max(body_pos: torch.Tensor, body_rot: torch.Tensor, body_vel: torch.Tensor, body_ang_vel: torch.Tensor,
                     local_root_obs: bool, root_height_obs: bool) -> torch.Tensor:
    """compute_humanoid_observations_max (env/tasks/humanoid.py:592-636): [n, B, 3 | 4] state -> [n, 15 B - 2]."""
    _check(body_pos.dim() == 3 and body_pos.shape[2] == 3 and body_rot.shape == (*body_pos.shape[:2], 4) and
           body_vel.shape == body_pos.shape and body_ang_vel.shape == body_pos.shape,
           'humanoid_obs_max: body_pos / body_vel / body_ang_vel [n, B, 3], body_rot [n, B, 4]')
    n, B = body_pos.shape[0], body_pos.shape[1]
    obs = torch.empty(n, 15 * B - 2, dtype=torch.float32, device=body_pos.device)
    _backend().humanoid_obs_max(_f32c(body_pos, 'body_pos'), _f32c(body_rot, 'body_rot'), _f32c(body_vel, 'body_vel'),
                                _f32c(body_ang_vel, 'body_ang_vel'), local_root_obs, root_height_obs, obs)
    return obs


@humanoid_obs_max.register_fake
def _(body_pos, body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs):
    return body_pos.new_empty(body_pos.shape[0], 15 * body_pos.shape[1] - 2, dtype=torch.float32)


@torch.library.custom_op('ase_hip::humanoid_reset', mutates_args=(), device_types='cuda')
def humanoid_reset(progress_buf: torch.Tensor, contact_forces: torch.Tensor, body_pos: torch.Tensor,
                   termination_heights: torch.Tensor, contact_body_ids: list[int], max_episode_length: float,
                   enable_early_termination: bool, tar_contact_forces: torch.Tensor | None = None,
                   strike_body_ids: list[int] | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """compute_humanoid_reset (env/tasks/humanoid.py:645-672; strike form env/tasks/humanoid_strike.py:255-297 when
    tar_contact_forces and strike_body_ids are given) -> (reset, terminated), int64 [n]."""
    _check(progress_buf.dtype == torch.int64 and progress_buf.dim() == 1, 'humanoid_reset: progress_buf int64 [n]')
    _check(contact_forces.shape == body_pos.shape and body_pos.dim() == 3 and body_pos.shape[0] == progress_buf.shape[0] and
           termination_heights.numel() == body_pos.shape[1], 'humanoid_reset: contact_forces / body_pos [n, B, 3], termination_heights [B]')
    _check((tar_contact_forces is None) == (strike_body_ids is None), 'humanoid_reset: the strike form takes tar_contact_forces AND strike_body_ids')
    reset, terminated = torch.empty_like(progress_buf), torch.empty_like(progress_buf)
    _backend().humanoid_reset(progress_buf.contiguous(), _f32c(contact_forces, 'contact_forces'), _f32c(body_pos, 'body_pos'),
                              _f32c(termination_heights, 'termination_heights'), contact_body_ids, max_episode_length,
                              enable_early_termination, reset, terminated, _opt_f32c(tar_contact_forces, 'tar_contact_forces'),
                              strike_body_ids)
    return reset, terminated


@humanoid_reset.register_fake
def _(progress_buf, contact_forces, body_pos, termination_heights, contact_body_ids, max_episode_length, enable_early_termination,
      tar_contact_forces=None, strike_body_ids=None):
    return torch.empty_like(progress_buf), torch.empty_like(progress_buf)


@torch.library.custom_op('ase_hip::task_obs', mutates_args=(), device_types='cuda')
def task_obs(kind: str, root_states: torch.Tensor, tar_a: torch.Tensor | None = None, tar_b: torch.Tensor | None = None,
             tar_speed: torch.Tensor | None = None, tar_states: torch.Tensor | None = None) -> torch.Tensor:
    """Task observation of 'heading' | 'location' | 'reach' | 'strike' -> [n, 5 | 2 | 3 | 15] (operands: see ase_hip_task_obs)."""
    k = _task_kind(kind)
    obs = torch.empty(root_states.shape[0], L.TASK_OBS_COLS[k], dtype=torch.float32, device=root_states.device)
    _backend().task_obs(k, obs, 0, None, _f32c(root_states, 'root_states', 13), _opt_f32c(tar_a, 'tar_a'), _opt_f32c(tar_b, 'tar_b'),
                        _opt_f32c(tar_speed, 'tar_speed'), _opt_f32c(tar_states, 'tar_states'))
    return obs


@task_obs.register_fake
def _(kind, root_states, tar_a=None, tar_b=None, tar_speed=None, tar_states=None):
    return root_states.new_empty(root_states.shape[0], L.TASK_OBS_COLS[_task_kind(kind)], dtype=torch.float32)


@torch.library.custom_op('ase_hip::task_reward', mutates_args=(), device_types='cuda')
def task_reward(kind: str, n_envs: int, root_states: torch.Tensor | None = None, prev_root_pos: torch.Tensor | None = None,
                tar_a: torch.Tensor | None = None, tar_b: torch.Tensor | None = None, tar_speed: torch.Tensor | None = None,
                tar_speed_scalar: float = 0.0, tar_states: torch.Tensor | None = None, body_pos: torch.Tensor | None = None,
                body_id: int = 0, dt: float = 0.0) -> torch.Tensor:
    """Task reward of 'heading' | 'location' | 'reach' | 'strike' -> [n_envs] (operands: see ase_hip_task_reward)."""
    k = _task_kind(kind)
    some = next((t for t in (root_states, tar_a, tar_states, body_pos) if t is not None), None)
    _check(some is not None, 'task_reward: no operands')
    reward = torch.empty(n_envs, dtype=torch.float32, device=some.device)
    _backend().task_reward(k, reward, _opt_f32c(root_states, 'root_states'), _opt_f32c(prev_root_pos, 'prev_root_pos'),
                           _opt_f32c(tar_a, 'tar_a'), _opt_f32c(tar_b, 'tar_b'),
                           _opt_f32c(tar_speed, 'tar_speed') if tar_speed is not None else (tar_speed_scalar if k == L.TASK_LOCATION else None),
                           _opt_f32c(tar_states, 'tar_states'), _opt_f32c(body_pos, 'body_pos'), body_id, dt)
    return reward


@task_reward.register_fake
def _(kind, n_envs, root_states=None, prev_root_pos=None, tar_a=None, tar_b=None, tar_speed=None, tar_speed_scalar=0.0,
      tar_states=None, body_pos=None, body_id=0, dt=0.0):
    some = next(t for t in (root_states, tar_a, tar_states, body_pos) if t is not None)
    return some.new_empty(n_envs, dtype=torch.float32)


_RESET_RANGES = {'heading': ('tar_speed_min', 'tar_speed_max'), 'location': ('tar_dist_max',),
                 'reach': ('tar_dist_max', 'tar_height_min', 'tar_height_max'),
                 'strike': ('tar_dist_min', 'tar_dist_max', 'near_dist', 'near_prob')}


@torch.library.custom_op('ase_hip::task_reset', mutates_args=('change_steps', 'tar_a', 'tar_b', 'tar_speed', 'tar_states', 'rng_state'),
                         device_types='cuda')
def task_reset(kind: str, ranges: list[float], steps_low: int, steps_high: int, enable_rand_heading: bool,
               progress_buf: torch.Tensor | None, change_steps: torch.Tensor | None, root_states: torch.Tensor | None,
               tar_a: torch.Tensor | None, tar_b: torch.Tensor | None, tar_speed: torch.Tensor | None,
               tar_states: torch.Tensor | None, env_ids: torch.Tensor | None, u: torch.Tensor | None, steps: torch.Tensor | None,
               rng_state: torch.Tensor | None, advance: bool = True) -> None:
    """New targets and change steps of 'heading' | 'location' | 'reach' | 'strike' in one launch (operands: see
    ase_hip_task_reset).  ranges: heading [tar_speed_min, tar_speed_max], location [tar_dist_max], reach [tar_dist_max,
    tar_height_min, tar_height_max], strike [tar_dist_min, tar_dist_max, near_dist, near_prob].  env_ids None: every environment
    with progress_buf >= change_steps; draws from u / steps or, on the device, from rng_state (advanced unless advance is false).
    Every tensor is passed by position, None where the kind or the mode has none."""
    k = _task_kind(kind)
    names = _RESET_RANGES[kind]
    _check(len(ranges) == len(names), f'task_reset: {kind} takes ranges = [{", ".join(names)}]')
    _backend().task_reset(k, progress_buf, change_steps, root_states, tar_a, tar_b, tar_speed, tar_states, env_ids, u, steps, rng_state,
                          advance, steps_low, steps_high, enable_rand_heading=enable_rand_heading, **dict(zip(names, ranges)))


@torch.library.custom_op('ase_hip::proj_launch', mutates_args=('proj_states', 'rng_state', 'slot_out', 'ids_out', 'draws_out'),
                         device_types='cuda')
def proj_launch(root_states: torch.Tensor, body_pos: torch.Tensor, body_vel: torch.Tensor, proj_states: torch.Tensor,
                progress_buf: torch.Tensor | None, timesteps: torch.Tensor | None, slot: int, env_ids: torch.Tensor | None,
                u: torch.Tensor | None, eps: torch.Tensor | None, rng_state: torch.Tensor | None, advance: bool, tar_body: int,
                ranges: list[float], noise: float, slot_out: torch.Tensor | None, ids_out: torch.Tensor | None,
                draws_out: torch.Tensor | None) -> None:
    """One projectile launch of the perturbation task (operands: see ase_hip_proj_launch).  slot -1: due mode on
    progress_buf[0] and timesteps; slot >= 0: that projectile for every environment or for env_ids.  ranges = [dist_min,
    dist_max, h_min, h_max, speed_min, speed_max]; draws from u / eps or, on the device, from rng_state (advanced unless advance
    is false).  Every tensor is passed by position, None where the mode has none."""
    _check(len(ranges) == 6, 'proj_launch: ranges = [dist_min, dist_max, h_min, h_max, speed_min, speed_max]')
    for name, t, dt in (('root_states', root_states, torch.float32), ('body_pos', body_pos, torch.float32),
                        ('body_vel', body_vel, torch.float32), ('proj_states', proj_states, torch.float32),
                        ('progress_buf', progress_buf, torch.int64), ('timesteps', timesteps, torch.int32),
                        ('env_ids', env_ids, torch.int32), ('u', u, torch.float32), ('eps', eps, torch.float32),
                        ('rng_state', rng_state, torch.int64), ('slot_out', slot_out, torch.int32), ('ids_out', ids_out, torch.int32),
                        ('draws_out', draws_out, torch.float32)):
        _check(t is None or t.dtype == dt, f'proj_launch: {name} must be {dt}')
    _check(proj_states.dim() == 3 and proj_states.shape[2] == 13 and proj_states.stride(2) == 1,
           'proj_launch: proj_states f32 [n, K, 13] with unit stride in the last dimension')
    keys = ('dist_min', 'dist_max', 'h_min', 'h_max', 'speed_min', 'speed_max')
    _backend().proj_launch(root_states, body_pos, body_vel, proj_states, progress_buf, timesteps, slot, env_ids, u, eps, rng_state,
                           advance, tar_body, noise=noise, slot_out=slot_out, ids_out=ids_out, draws_out=draws_out,
                           **dict(zip(keys, ranges)))


@proj_launch.register_fake
def _(root_states, body_pos, body_vel, proj_states, progress_buf, timesteps, slot, env_ids, u, eps, rng_state, advance, tar_body,
      ranges, noise, slot_out, ids_out, draws_out):
    return None


@torch.library.custom_op('ase_hip::motion_sync', mutates_args=('motion_ids', 'progress_buf', 'reset_buf', 'terminate_buf', 'root_states',
                                                                'dof_pos', 'dof_vel', 'body_pos', 'body_rot', 'body_vel', 'body_ang_vel',
                                                                'ids_out'), device_types='cuda')
def motion_sync(mode: str, motion_ids: torch.Tensor, progress_buf: torch.Tensor, reset_buf: torch.Tensor, terminate_buf: torch.Tensor,
                motion_dt: float, root_states: torch.Tensor | None, dof_pos: torch.Tensor | None, dof_vel: torch.Tensor | None,
                body_pos: torch.Tensor | None, body_rot: torch.Tensor | None, body_vel: torch.Tensor | None,
                body_ang_vel: torch.Tensor | None, env_ids: torch.Tensor | None, ids_out: torch.Tensor | None, gts: torch.Tensor,
                grs: torch.Tensor, lrs: torch.Tensor, lengths: torch.Tensor, num_frames: torch.Tensor, clip_dt: torch.Tensor,
                length_starts: torch.Tensor, dof_body_ids: list[int], dof_offsets: list[int]) -> None:
    """The view-motion task's step ('sync') or reset ('reset') in one launch (operands: see ase_hip_motion_sync).  'sync': the
    end-of-clip test on progress_buf * motion_dt and the sampled pose written in place into root_states / dof_pos / dof_vel and
    the optional rigid-body tensors, at their own strides.  'reset': the rows with reset_buf != 0, or env_ids, move on to their
    next clip; no state tensor.  Every tensor is passed by position, None where the mode has none."""
    _check(mode in ('sync', 'reset'), "motion_sync: mode is 'sync' or 'reset'")
    for name, t, dt in (('motion_ids', motion_ids, torch.int32), ('progress_buf', progress_buf, torch.int64),
                        ('reset_buf', reset_buf, torch.int64), ('terminate_buf', terminate_buf, torch.int64),
                        ('root_states', root_states, torch.float32), ('dof_pos', dof_pos, torch.float32), ('dof_vel', dof_vel, torch.float32),
                        ('body_pos', body_pos, torch.float32), ('body_rot', body_rot, torch.float32), ('body_vel', body_vel, torch.float32),
                        ('body_ang_vel', body_ang_vel, torch.float32), ('env_ids', env_ids, torch.int32), ('ids_out', ids_out, torch.int32),
                        ('gts', gts, torch.float32), ('grs', grs, torch.float32), ('lrs', lrs, torch.float32), ('lengths', lengths, torch.float32),
                        ('num_frames', num_frames, torch.int32), ('clip_dt', clip_dt, torch.float32), ('length_starts', length_starts, torch.int32)):
        _check(t is None or t.dtype == dt, f'motion_sync: {name} must be {dt}')
    _check(gts.dim() == 3 and gts.is_contiguous() and grs.is_contiguous() and lrs.is_contiguous(), 'motion_sync: contiguous clip tensors')
    clips = dict(gts=gts, grs=grs, lrs=lrs, lengths=lengths, num_frames=num_frames, dt=clip_dt, length_starts=length_starts,
                 dof_body_ids=dof_body_ids, dof_offsets=dof_offsets)
    _backend().motion_sync(clips, motion_ids, progress_buf, reset_buf, terminate_buf, L.MOTION_SYNC if mode == 'sync' else L.MOTION_RESET,
                           motion_dt, root_states, dof_pos, dof_vel, body_pos, body_rot, body_vel, body_ang_vel, env_ids, ids_out)


@motion_sync.register_fake
def _(mode, motion_ids, progress_buf, reset_buf, terminate_buf, motion_dt, root_states, dof_pos, dof_vel, body_pos, body_rot, body_vel,
      body_ang_vel, env_ids, ids_out, gts, grs, lrs, lengths, num_frames, clip_dt, length_starts, dof_body_ids, dof_offsets):
    return None


@torch.library.custom_op('ase_hip::latent_renew', mutates_args=('latents', 'reset_steps', 'rng_state', 'z2'), device_types='cuda')
def latent_renew(latents: torch.Tensor, env_ids: torch.Tensor | None, eps: torch.Tensor | None, steps: torch.Tensor | None,
                 rng_state: torch.Tensor | None, advance: bool, progress_buf: torch.Tensor | None, reset_steps: torch.Tensor | None,
                 steps_add: bool, steps_low: int, steps_high: int, z2: torch.Tensor | None) -> None:
    """New unit latents (and step counts, when reset_steps is given) of the ASE agent's environments in one launch (operands: see
    ase_hip_latent_renew).  env_ids None: every environment with reset_steps <= progress_buf, and z2 [n_envs, dim] receives every
    environment's latent after the decision; draws from eps / steps or, on the device, from rng_state (advanced unless advance is
    false).  Every tensor is passed by position, None where the mode has none."""
    _check(latents.dim() == 2 and latents.dtype == torch.float32 and latents.stride(1) == 1, 'latent_renew: latents f32 [n_envs, dim]')
    for name, t, dts in (('env_ids', env_ids, (torch.int32,)), ('eps', eps, (torch.float32,)), ('steps', steps, (torch.int32,)),
                         ('rng_state', rng_state, (torch.int64,)), ('progress_buf', progress_buf, (torch.int32, torch.int64)),
                         ('reset_steps', reset_steps, (torch.int32,)), ('z2', z2, (torch.float32, torch.float16, torch.bfloat16))):
        _check(t is None or t.dtype in dts, f'latent_renew: {name} must be {" or ".join(str(d) for d in dts)}')
    _backend().latent_renew(latents, env_ids, eps, steps, rng_state, advance, progress_buf, reset_steps, steps_add, steps_low, steps_high, z2)


@latent_renew.register_fake
def _(latents, env_ids, eps, steps, rng_state, advance, progress_buf, reset_steps, steps_add, steps_low, steps_high, z2):
    return None


@torch.library.custom_op('ase_hip::amp_reset', mutates_args=('root_states', 'dof_pos', 'dof_vel', 'hist'), device_types='cuda')
def amp_reset(root_states: torch.Tensor, dof_pos: torch.Tensor, dof_vel: torch.Tensor, hist: torch.Tensor, body_pos: torch.Tensor,
              body_rot: torch.Tensor, body_vel: torch.Tensor, body_ang_vel: torch.Tensor, env_ids: torch.Tensor, kind: torch.Tensor,
              motion_ids: torch.Tensor | None, motion_times: torch.Tensor | None, src_rows: torch.Tensor | None,
              gts: torch.Tensor | None, grs: torch.Tensor | None, lrs: torch.Tensor | None, grvs: torch.Tensor | None,
              gravs: torch.Tensor | None, dvs: torch.Tensor | None, lengths: torch.Tensor | None, num_frames: torch.Tensor | None,
              dt: torch.Tensor | None, length_starts: torch.Tensor | None, tab_root_states: torch.Tensor | None,
              tab_dof_pos: torch.Tensor | None, tab_dof_vel: torch.Tensor | None, dof_body_ids: list[int], dof_offsets: list[int],
              key_body_ids: list[int], local_root_obs: bool, root_height_obs: bool, env_dt: float) -> None:
    """HumanoidAMP / HumanoidAMPGetup resets in one launch (operands: see ase_hip_amp_reset): root_states [N, 13], dof_pos /
    dof_vel [N, D] (strided views allowed) and hist [N, S, F] are written in place.  Rows of kind 'table' need the three tab_*
    tensors and src_rows, rows of kind 'motion' the clip tensors, motion_ids and motion_times; without them such rows are skipped."""
    clip = (gts, grs, lrs, grvs, gravs, dvs, lengths, num_frames, dt, length_starts, motion_ids, motion_times)
    tab = (tab_root_states, tab_dof_pos, tab_dof_vel, src_rows)
    has_motion, has_table = all(t is not None for t in clip), all(t is not None for t in tab)
    _check(has_motion or all(t is None for t in clip), 'amp_reset: the clip tensors, motion_ids and motion_times come together')
    _check(has_table or all(t is None for t in tab), 'amp_reset: the state table and src_rows come together')
    clips = {'dof_body_ids': dof_body_ids, 'dof_offsets': dof_offsets, 'key_body_ids': key_body_ids}
    if has_motion:
        clips.update(gts=gts, grs=grs, lrs=lrs, grvs=grvs, gravs=gravs, dvs=dvs, lengths=lengths, num_frames=num_frames, dt=dt,
                     length_starts=length_starts)
    _backend().amp_reset(clips, env_ids, kind, motion_ids, motion_times, src_rows, tab[:3] if has_table else None, root_states, dof_pos,
                         dof_vel, _f32c(body_pos, 'body_pos'), _f32c(body_rot, 'body_rot'), _f32c(body_vel, 'body_vel'),
                         _f32c(body_ang_vel, 'body_ang_vel'), local_root_obs, root_height_obs, env_dt, hist,
                         (L.RESET_HAS_TABLE if has_table else 0) | (L.RESET_HAS_MOTION if has_motion else 0))


_STATE_INIT = {'Default': L.INIT_DEFAULT, 'Start': L.INIT_START, 'Random': L.INIT_RANDOM, 'Hybrid': L.INIT_HYBRID}


@torch.library.custom_op('ase_hip::amp_reset_due',
                         mutates_args=('root_states', 'dof_pos', 'dof_vel', 'hist', 'reset_buf', 'rng_state', 'progress_buf',
                                       'terminate_buf', 'recovery_counter', 'env_ids_out', 'kind_out', 'motion_ids_out',
                                       'motion_times_out', 'src_rows_out'), device_types='cuda')
def amp_reset_due(root_states: torch.Tensor, dof_pos: torch.Tensor, dof_vel: torch.Tensor, hist: torch.Tensor, body_pos: torch.Tensor,
                  body_rot: torch.Tensor, body_vel: torch.Tensor, body_ang_vel: torch.Tensor, reset_buf: torch.Tensor,
                  rng_state: torch.Tensor, progress_buf: torch.Tensor | None, terminate_buf: torch.Tensor | None,
                  recovery_counter: torch.Tensor | None, env_ids_out: torch.Tensor | None, kind_out: torch.Tensor | None,
                  motion_ids_out: torch.Tensor | None, motion_times_out: torch.Tensor | None, src_rows_out: torch.Tensor | None,
                  gts: torch.Tensor | None, grs: torch.Tensor | None, lrs: torch.Tensor | None, grvs: torch.Tensor | None,
                  gravs: torch.Tensor | None, dvs: torch.Tensor | None, lengths: torch.Tensor | None, num_frames: torch.Tensor | None,
                  dt: torch.Tensor | None, length_starts: torch.Tensor | None, clip_cdf: torch.Tensor | None,
                  tab_root_states: torch.Tensor | None, tab_dof_pos: torch.Tensor | None, tab_dof_vel: torch.Tensor | None,
                  dof_body_ids: list[int], dof_offsets: list[int], key_body_ids: list[int], state_init: str, hybrid_init_prob: float,
                  getup: bool, recovery_episode_prob: float, recovery_steps: int, fall_init_prob: float, local_root_obs: bool,
                  root_height_obs: bool, env_dt: float, advance: bool = True) -> None:
    """HumanoidAMP / HumanoidAMPGetup resets of every environment with reset_buf != 0 in one launch, draws included (operands and
    the draw table: see ase_hip_amp_reset_due).  state_init 'Default' | 'Start' | 'Random' | 'Hybrid'; the clip tensors and clip_cdf
    come together (all but 'Default'), so do the three tab_* tensors ('Default', 'Hybrid', fall episodes) and the five plan
    outputs.  Every tensor is passed by position, None where the mode has none."""
    _check(state_init in _STATE_INIT, f'amp_reset_due: state_init is one of {list(_STATE_INIT)}')
    clip = (gts, grs, lrs, grvs, gravs, dvs, lengths, num_frames, dt, length_starts, clip_cdf)
    tab = (tab_root_states, tab_dof_pos, tab_dof_vel)
    outs = (env_ids_out, kind_out, motion_ids_out, motion_times_out, src_rows_out)
    has_clips, has_table, has_plan = (all(t is not None for t in ts) for ts in (clip, tab, outs))
    _check(has_clips or all(t is None for t in clip), 'amp_reset_due: the clip tensors and clip_cdf come together')
    _check(has_table or all(t is None for t in tab), 'amp_reset_due: the state table comes together')
    _check(has_plan or all(t is None for t in outs), 'amp_reset_due: the plan outputs come all or none')
    _check(has_clips or state_init == 'Default', f'amp_reset_due: {state_init} needs the clip tensors and clip_cdf')
    clips = {'dof_body_ids': dof_body_ids, 'dof_offsets': dof_offsets, 'key_body_ids': key_body_ids}
    if has_clips:
        clips.update(gts=gts, grs=grs, lrs=lrs, grvs=grvs, gravs=gravs, dvs=dvs, lengths=lengths, num_frames=num_frames, dt=dt,
                     length_starts=length_starts)
    plan = dict(zip(('env_ids', 'kind', 'motion_ids', 'motion_times', 'src_rows'), outs)) if has_plan else None
    _backend().amp_reset_due(clips, clip_cdf, tab if has_table else None, _STATE_INIT[state_init], hybrid_init_prob,
                             (recovery_episode_prob, recovery_steps, fall_init_prob) if getup else None, rng_state, progress_buf,
                             reset_buf, terminate_buf, recovery_counter, plan, root_states, dof_pos, dof_vel,
                             _f32c(body_pos, 'body_pos'), _f32c(body_rot, 'body_rot'), _f32c(body_vel, 'body_vel'),
                             _f32c(body_ang_vel, 'body_ang_vel'), local_root_obs, root_height_obs, env_dt, hist, advance)


@torch.library.custom_op('ase_hip::amp_demo_fetch', mutates_args=('out', 'rng_state', 'motion_ids_out', 'motion_times0_out'),
                         device_types='cuda')
def amp_demo_fetch(out: torch.Tensor, ring_rows: int, head: int, n: int, num_steps: int, truncate_time: float, dt: float,
                   motion_ids: torch.Tensor | None, motion_times0: torch.Tensor | None, rng_state: torch.Tensor | None,
                   clip_cdf: torch.Tensor | None, motion_ids_out: torch.Tensor | None, motion_times0_out: torch.Tensor | None,
                   gts: torch.Tensor, grs: torch.Tensor, lrs: torch.Tensor, grvs: torch.Tensor, gravs: torch.Tensor,
                   dvs: torch.Tensor, lengths: torch.Tensor, num_frames: torch.Tensor, clip_dt: torch.Tensor,
                   length_starts: torch.Tensor, dof_body_ids: list[int], dof_offsets: list[int], key_body_ids: list[int],
                   local_root_obs: bool, root_height_obs: bool, advance: bool = True, head_dev: torch.Tensor | None = None) -> None:
    """The demo fetch in one launch (operands and the draw table: see ase_hip_amp_demo_fetch): n demo observations of num_steps
    frames go to rows (head + i) % ring_rows of out [ring_rows, >= num_steps F].  Either motion_ids / motion_times0 are passed
    in or rng_state / clip_cdf draw them on the device; motion_ids_out / motion_times0_out come both or none."""
    given, drawn = (motion_ids, motion_times0), (rng_state, clip_cdf)
    has_given, has_drawn = all(t is not None for t in given), all(t is not None for t in drawn)
    _check(has_given or all(t is None for t in given), 'amp_demo_fetch: motion_ids and motion_times0 come together')
    _check(has_drawn or all(t is None for t in drawn), 'amp_demo_fetch: rng_state and clip_cdf come together')
    _check(has_given != has_drawn, 'amp_demo_fetch: either motion_ids / motion_times0 or rng_state / clip_cdf')
    _check((motion_ids_out is None) == (motion_times0_out is None), 'amp_demo_fetch: the draw outputs come both or none')
    _check(out.dim() == 2 and out.dtype == torch.float32 and out.is_cuda and out.stride(1) == 1, 'amp_demo_fetch: out is an f32 '
           'device tensor [ring_rows, >= num_steps F] with unit column stride')
    clips = dict(gts=gts, grs=grs, lrs=lrs, grvs=grvs, gravs=gravs, dvs=dvs, lengths=lengths, num_frames=num_frames, dt=clip_dt,
                 length_starts=length_starts, dof_body_ids=dof_body_ids, dof_offsets=dof_offsets, key_body_ids=key_body_ids)
    _backend().amp_demo_fetch(clips, out, ring_rows, head, n, num_steps, truncate_time, dt, local_root_obs, root_height_obs,
                              motion_ids=motion_ids, motion_times0=motion_times0, rng_state=rng_state, clip_cdf=clip_cdf,
                              advance=advance, draws_out=None if motion_ids_out is None else (motion_ids_out, motion_times0_out),
                              head_dev=head_dev)


@torch.library.custom_op('ase_hip::rollout_store', mutates_args=('dsts', 'rewards_out', 'dones_out', 'next_values_out', 'cur_rewards',
                                                             'cur_lengths', 'meter', 'done_ids_out'), device_types='cuda')
def rollout_store(dones: torch.Tensor, slot: int, n_slots: int, srcs: list[torch.Tensor], dsts: list[torch.Tensor],
                  rewards: torch.Tensor | None, shift: float, scale: float, rewards_out: torch.Tensor | None,
                  dones_out: torch.Tensor | None, next_values: torch.Tensor | None, terminate: torch.Tensor | None,
                  next_values_out: torch.Tensor | None, cur_rewards: torch.Tensor | None, cur_lengths: torch.Tensor | None,
                  meter: torch.Tensor | None, max_size: int, done_ids_out: torch.Tensor | None,
                  slot_dev: torch.Tensor | None = None) -> None:
    """One environment step stored into experience slot `slot` (operands: see ase_hip_rollout_store): srcs[i] [n_envs, D_i] is
    copied to dsts[i][slot] ([n_slots, n_envs, D_i]), the shaped reward, the done flags and the masked next value go to their
    slotted buffers, the episode accumulators are advanced in place, the two meters (meter f64 [4]) take the done rows and
    done_ids_out receives e / -1.  Every tensor is passed by position, None where a group is left out."""
    _check(len(srcs) == len(dsts) and len(srcs) <= L.ROLLOUT_STORE_MAX_FIELDS, 'rollout_store: as many sources as destinations, at most 16')
    kinds = (torch.uint8, torch.bool, torch.int32, torch.int64, torch.float32)
    _check(dones.dtype in kinds and (terminate is None or terminate.dtype in kinds),
           'rollout_store: dones / terminate must be uint8, bool, int32, int64 or float32')
    _check((cur_rewards is None) == (cur_lengths is None) == (meter is None), 'rollout_store: the accumulators and the meter come together')
    _backend().rollout_store(dones, slot=slot, n_slots=n_slots, fields=list(zip(srcs, dsts)), rewards=rewards, shift=shift,
                             scale=scale, rewards_out=rewards_out, dones_out=dones_out, next_values=next_values,
                             terminate=terminate, next_values_out=next_values_out, cur_rewards=cur_rewards,
                             cur_lengths=cur_lengths, meter=meter, max_size=max_size, done_ids_out=done_ids_out, slot_dev=slot_dev)


@rollout_store.register_fake
def _(dones, slot, n_slots, srcs, dsts, rewards, shift, scale, rewards_out, dones_out, next_values, terminate, next_values_out,
      cur_rewards, cur_lengths, meter, max_size, done_ids_out, slot_dev=None):
    return None


@torch.library.custom_op('ase_hip::rollout_head', mutates_args=('xa', 'xc', 'zc', 'zs', 'obses_out', 'z_out'), device_types='cuda')
def rollout_head(obs: torch.Tensor, z: torch.Tensor | None, mean: torch.Tensor | None, std: torch.Tensor | None,
                 xa: torch.Tensor | None, xc: torch.Tensor | None, zc: torch.Tensor | None, zs: torch.Tensor | None,
                 obses_out: torch.Tensor | None, z_out: torch.Tensor | None, slot: int, slot_dev: torch.Tensor | None = None) -> None:
    """The head of one environment step in one launch (operands: see ase_hip_rollout_head): obs [n, D] normalised with mean /
    std into xa / xc, the latents z [n, Z] converted into zc / zs, the raw rows copied into obses_out[slot] / z_out[slot]
    ([n_slots, n, D] / [n_slots, n, Z]); slot_dev int32 [1]: the slot is the word read when the launch runs.  Every tensor is
    passed by position, None where an output is left out."""
    _check(obs.dim() == 2 and obs.dtype == torch.float32, 'rollout_head: obs f32 [n, D]')
    _check(any(t is not None for t in (xa, xc, zc, zs, obses_out, z_out)), 'rollout_head: at least one output')
    _check((xa is None and xc is None) or (mean is not None and std is not None), 'rollout_head: xa / xc need mean and std')
    _backend().rollout_head(obs, z, mean, std, xa, xc, zc, zs, obses_out, z_out, slot, slot_dev)


@rollout_head.register_fake
def _(obs, z, mean, std, xa, xc, zc, zs, obses_out, z_out, slot, slot_dev=None):
    return None


@torch.library.custom_op('ase_hip::word_step', mutates_args=('word',), device_types='cuda')
def word_step(word: torch.Tensor, add: int, wrap: int) -> None:
    """word[0] = (word[0] + add) mod wrap on the device (wrap <= 0: no modulo); word int32 [1]."""
    _check(word.dtype == torch.int32 and word.numel() == 1, 'word_step: word int32 [1]')
    _backend().word_step(word, add, wrap)


@word_step.register_fake
def _(word, add, wrap):
    return None


@torch.library.custom_op('ase_hip::hrl_latent', mutates_args=(), device_types='cuda')
def hrl_latent(actions: torch.Tensor) -> torch.Tensor:
    _check(actions.dim() == 2 and actions.dtype == torch.float32 and 1 <= actions.shape[1] <= 128 and actions.stride(1) == 1,
           'hrl_latent: actions f32 [n, 1 <= d <= 128], unit column stride')
    z = torch.empty(actions.shape, dtype=torch.float32, device=actions.device)
    _backend().hrl_latent(actions, z=z)
    return z


@hrl_latent.register_fake
def _(actions):
    return actions.new_empty(actions.shape)


@torch.library.custom_op('ase_hip::hrl_llc_action', mutates_args=(), device_types='cuda')
def hrl_llc_action(mu: torch.Tensor, low: torch.Tensor, high: torch.Tensor, act: int, clip: bool) -> torch.Tensor:
    _check(mu.dim() == 2 and mu.dtype == torch.float32 and 1 <= act <= 128 and mu.shape[1] >= act and mu.stride(1) == 1,
           'hrl_llc_action: mu f32 [n, >= act], 1 <= act <= 128, unit column stride')
    out = torch.empty(mu.shape[0], act, dtype=torch.float32, device=mu.device)
    _backend().hrl_llc_action(mu, low.float().contiguous(), high.float().contiguous(), out, act, clip)
    return out


@hrl_llc_action.register_fake
def _(mu, low, high, act, clip):
    return mu.new_empty(mu.shape[0], act)


@torch.library.custom_op('ase_hip::hrl_accum', mutates_args=('acc', 'rewards_out', 'disc_out', 'dones_out', 'terminate_out'),
                         device_types='cuda')
def hrl_accum(rewards: torch.Tensor, dones: torch.Tensor, terminate: torch.Tensor | None, logit: torch.Tensor | None,
              disc_scale: float, acc: torch.Tensor, first: bool, last: bool, llc_steps: int, rewards_out: torch.Tensor | None,
              disc_out: torch.Tensor | None, dones_out: torch.Tensor | None, terminate_out: torch.Tensor | None) -> None:
    """One inner step of HRLAgent.env_step folded into acc f32 [4, n] (operands: see ase_hip_hrl_accum); with last the means and
    masks go to the four f32 outputs.  Every tensor is passed by position, None where a group is left out."""
    kinds = (torch.uint8, torch.bool, torch.int32, torch.int64, torch.float32)
    _check(dones.dtype in kinds and (terminate is None or terminate.dtype in kinds),
           'hrl_accum: dones / terminate must be uint8, bool, int32, int64 or float32')
    _check(llc_steps >= 1, 'hrl_accum: llc_steps >= 1')
    _backend().hrl_accum(rewards, dones, acc, first, last, llc_steps, terminate=terminate, logit=logit, disc_scale=disc_scale,
                         rewards_out=rewards_out, disc_out=disc_out, dones_out=dones_out, terminate_out=terminate_out)


@hrl_accum.register_fake
def _(rewards, dones, terminate, logit, disc_scale, acc, first, last, llc_steps, rewards_out, disc_out, dones_out, terminate_out):
    return None


@torch.library.custom_op('ase_hip::env_pre_step', mutates_args=('actions', 'targets', 'prev_root_pos', 'recovery_counter'),
                         device_types='cuda')
def env_pre_step(actions_in: torch.Tensor, actions: torch.Tensor, targets: torch.Tensor, clip_actions: float,
                 pd_offset: torch.Tensor | None, pd_scale: torch.Tensor | None, motor_efforts: torch.Tensor | None, power_scale: float,
                 root_states: torch.Tensor | None, prev_root_pos: torch.Tensor | None, recovery_counter: torch.Tensor | None) -> None:
    """The pre_physics_step chain in one launch (operands: see ase_hip_env_pre_step).  Every tensor is passed by position, None
    where a group is left out; actions, targets, prev_root_pos and recovery_counter are written in place."""
    _check(actions_in.dim() == 2 and actions_in.dtype == torch.float32, 'env_pre_step: actions_in f32 [n, D]')
    _check((pd_offset is None) == (pd_scale is None) and (pd_offset is None) != (motor_efforts is None),
           'env_pre_step: pd_offset AND pd_scale, or motor_efforts')
    _backend().env_pre_step(actions_in, actions, targets, clip_actions, pd_offset, pd_scale, motor_efforts, power_scale, root_states,
                            prev_root_pos, recovery_counter)


@env_pre_step.register_fake
def _(actions_in, actions, targets, clip_actions, pd_offset, pd_scale, motor_efforts, power_scale, root_states, prev_root_pos,
      recovery_counter):
    return None


@torch.library.custom_op('ase_hip::env_post_step', mutates_args=('progress_buf', 'obs', 'reward', 'reset', 'terminated', 'hist'),
                         device_types='cuda')
def env_post_step(body_pos: torch.Tensor, body_rot: torch.Tensor, body_vel: torch.Tensor, body_ang_vel: torch.Tensor,
                  contact_forces: torch.Tensor, progress_buf: torch.Tensor, obs: torch.Tensor, reward: torch.Tensor,
                  reset: torch.Tensor, terminated: torch.Tensor, termination_heights: torch.Tensor, contact_body_ids: list[int],
                  max_episode_length: float, enable_early_termination: bool, local_root_obs: bool, root_height_obs: bool,
                  col_offset: int, clip_obs: float, kind: str | None, enable_task_obs: bool, root_states: torch.Tensor | None,
                  prev_root_pos: torch.Tensor | None, tar_a: torch.Tensor | None, tar_b: torch.Tensor | None,
                  tar_speed: torch.Tensor | None, tar_speed_scalar: float, tar_states: torch.Tensor | None, reach_body_id: int,
                  dt: float, tar_contact_forces: torch.Tensor | None, strike_body_ids: list[int] | None,
                  recovery_counter: torch.Tensor | None, hist: torch.Tensor | None, dof_pos: torch.Tensor | None,
                  dof_vel: torch.Tensor | None, dof_offsets: list[int] | None, key_body_ids: list[int] | None) -> None:
    """Humanoid.post_physics_step + HumanoidAMP.post_physics_step in one launch on state read in place (operands: see
    ase_hip_env_post_step; kind: 'heading' | 'location' | 'reach' | 'strike' | None).  Every tensor is passed by position, None
    where a group is left out; progress_buf, obs, reward, reset, terminated and hist are written in place."""
    k = None if kind is None else _task_kind(kind)
    _check(body_pos.dim() == 3 and body_pos.shape[2] == 3, 'env_post_step: body_pos [n, B, 3]')
    _check((hist is None) or (dof_pos is not None and dof_vel is not None and dof_offsets is not None and key_body_ids is not None),
           'env_post_step: hist needs dof_pos, dof_vel, dof_offsets and key_body_ids')
    _backend().env_post_step(body_pos, body_rot, body_vel, body_ang_vel, contact_forces, progress_buf, obs, reward, reset, terminated,
                             termination_heights, contact_body_ids, max_episode_length, enable_early_termination, local_root_obs,
                             root_height_obs, col_offset=col_offset, clip_obs=clip_obs, task_kind=k, enable_task_obs=enable_task_obs,
                             root_states=root_states, prev_root_pos=prev_root_pos, tar_a=tar_a, tar_b=tar_b,
                             tar_speed=tar_speed if tar_speed is not None else (tar_speed_scalar if k == L.TASK_LOCATION else None),
                             tar_states=tar_states, reach_body_id=reach_body_id, dt=dt, tar_contact_forces=tar_contact_forces,
                             strike_body_ids=strike_body_ids, recovery_counter=recovery_counter, hist=hist, dof_pos=dof_pos,
                             dof_vel=dof_vel, dof_offsets=dof_offsets, key_body_ids=key_body_ids)


@env_post_step.register_fake
def _(body_pos, body_rot, body_vel, body_ang_vel, contact_forces, progress_buf, obs, reward, reset, terminated, termination_heights,
      contact_body_ids, max_episode_length, enable_early_termination, local_root_obs, root_height_obs, col_offset, clip_obs, kind,
      enable_task_obs, root_states, prev_root_pos, tar_a, tar_b, tar_speed, tar_speed_scalar, tar_states, reach_body_id, dt,
      tar_contact_forces, strike_body_ids, recovery_counter, hist, dof_pos, dof_vel, dof_offsets, key_body_ids):
    return None


@torch.library.custom_op('ase_hip::clip_frames', mutates_args=(), device_types='cuda')
def clip_frames(rotation: torch.Tensor, root_translation: torch.Tensor, root_velocity: torch.Tensor,
                root_angular_velocity: torch.Tensor, local_translation: torch.Tensor, clip_first: torch.Tensor,
                clip_num_frames: torch.Tensor, clip_fps: torch.Tensor, frame_clip: torch.Tensor, parent_indices: list[int],
                dof_body_ids: list[int], dof_offsets: list[int]
                ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The clip loader in one launch (operands: see ase_hip_clip_frames): the raw f64 contents of SkeletonMotion clips,
    concatenated -> (gts [T, B, 3], grs, lrs [T, B, 4], grvs, gravs [T, 3], dvs [T, D]), f32."""
    _check(rotation.dim() == 3 and rotation.shape[2] == 4, 'clip_frames: rotation [T, B, 4]')
    T, B = rotation.shape[0], rotation.shape[1]
    for t, name, dt in ((rotation, 'rotation', torch.float64), (root_translation, 'root_translation', torch.float64),
                        (root_velocity, 'root_velocity', torch.float64), (root_angular_velocity, 'root_angular_velocity', torch.float64),
                        (local_translation, 'local_translation', torch.float32), (clip_first, 'clip_first', torch.int32),
                        (clip_num_frames, 'clip_num_frames', torch.int32), (clip_fps, 'clip_fps', torch.float64),
                        (frame_clip, 'frame_clip', torch.int32)):
        _check(t.dtype == dt and t.is_cuda, f'clip_frames: {name} is a {dt} device tensor')
    Cn = clip_first.numel()
    _check(all(t.shape == (T, 3) for t in (root_translation, root_velocity, root_angular_velocity)),
           'clip_frames: root_translation / root_velocity / root_angular_velocity [T, 3]')
    _check(local_translation.shape == (Cn, B, 3) and clip_num_frames.shape == clip_fps.shape == clip_first.shape == (Cn,) and
           frame_clip.shape == (T,), 'clip_frames: local_translation [C, B, 3], clip_first / clip_num_frames / clip_fps [C], frame_clip [T]')
    _check(len(parent_indices) == B and len(dof_offsets) == len(dof_body_ids) + 1 and len(dof_body_ids) >= 1,
           'clip_frames: parent_indices [B], dof_body_ids [J], dof_offsets [J + 1]')
    return _backend().clip_frames(rotation.contiguous(), root_translation.contiguous(), root_velocity.contiguous(),
                                  root_angular_velocity.contiguous(), local_translation.contiguous(), parent_indices,
                                  clip_first.contiguous(), clip_num_frames.contiguous(), clip_fps.contiguous(),
                                  frame_clip.contiguous(), dof_body_ids, dof_offsets)


@clip_frames.register_fake
def _(rotation, root_translation, root_velocity, root_angular_velocity, local_translation, clip_first, clip_num_frames, clip_fps,
      frame_clip, parent_indices, dof_body_ids, dof_offsets):
    T, B = rotation.shape[0], rotation.shape[1]
    f = lambda *shape: rotation.new_empty(*shape, dtype=torch.float32)
    return f(T, B, 3), f(T, B, 4), f(T, B, 4), f(T, 3), f(T, 3), f(T, dof_offsets[-1])


def _rt_dev(name, *ts):
    for t in ts:
        _check(t.is_cuda and t.dtype in (torch.float64, torch.float32, torch.int32), f'{name}: f64 / f32 / int32 device tensors')
    return [t.contiguous() for t in ts]


def _rt_shape(name, what, cond):
    _check(cond, f'{name}: {what}')


@torch.library.custom_op('ase_hip::retarget_fk', mutates_args=(), device_types='cuda')
def retarget_fk(rotation: torch.Tensor, mode: int, tree: torch.Tensor, clip_first: torch.Tensor, clip_num_frames: torch.Tensor,
                src_first: torch.Tensor, frame_clip: torch.Tensor) -> torch.Tensor:
    """Global rotations of a tree (operands: see ase_hip_retarget_fk) -> f64 [T, B, 4]."""
    _rt_shape('retarget_fk', 'rotation f64 [Tsrc, B, 4], tree int32 [B, ld]',
              rotation.dim() == 3 and rotation.shape[2] == 4 and rotation.dtype == torch.float64 and tree.dim() == 2 and
              tree.shape[0] == rotation.shape[1] and tree.dtype == torch.int32)
    _rt_shape('retarget_fk', 'clip_first / clip_num_frames / src_first int32 [C], frame_clip int32 [T]',
              clip_first.dim() == 1 and clip_first.shape == clip_num_frames.shape == src_first.shape and frame_clip.dim() == 1 and
              all(t.dtype == torch.int32 for t in (clip_first, clip_num_frames, src_first, frame_clip)))
    return _backend().retarget_fk(*_rt_dev('retarget_fk', rotation), mode,
                                  *_rt_dev('retarget_fk', tree, clip_first, clip_num_frames, src_first, frame_clip))


@retarget_fk.register_fake
def _(rotation, mode, tree, clip_first, clip_num_frames, src_first, frame_clip):
    return rotation.new_empty(frame_clip.shape[0], rotation.shape[1], 4)


@torch.library.custom_op('ase_hip::retarget_chain', mutates_args=(), device_types='cuda')
def retarget_chain(src_global: torch.Tensor, rs_body: torch.Tensor, rs_parent: torch.Tensor, rt_src: torch.Tensor,
                   rt_tree: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """Source global rotations -> global rotations on the reduced target tree (see ase_hip_retarget_chain), f64 [T, M, 4]."""
    _rt_shape('retarget_chain', 'src_global f64 [T, Bs, 4], params f64 [12]',
              src_global.dim() == 3 and src_global.shape[2] == 4 and src_global.dtype == params.dtype == torch.float64 and
              params.shape == (12,))
    _rt_shape('retarget_chain', 'rs_body / rs_parent / rt_src int32 [M], rt_tree int32 [M, ld]',
              rs_body.dim() == 1 and rs_body.shape == rs_parent.shape == rt_src.shape and rt_tree.dim() == 2 and
              rt_tree.shape[0] == rs_body.shape[0] and all(t.dtype == torch.int32 for t in (rs_body, rs_parent, rt_src, rt_tree)))
    return _backend().retarget_chain(*_rt_dev('retarget_chain', src_global, rs_body, rs_parent, rt_src, rt_tree, params))


@retarget_chain.register_fake
def _(src_global, rs_body, rs_parent, rt_src, rt_tree, params):
    return src_global.new_empty(src_global.shape[0], rs_body.shape[0], 4)


@torch.library.custom_op('ase_hip::retarget_pose', mutates_args=(), device_types='cuda')
def retarget_pose(state_global: torch.Tensor, tpose_global: torch.Tensor, target_global: torch.Tensor,
                  root_translation: torch.Tensor, params: torch.Tensor, rt_body: torch.Tensor, ancestor: torch.Tensor,
                  parent_indices: torch.Tensor, clip_first: torch.Tensor, clip_num_frames: torch.Tensor, src_first: torch.Tensor,
                  frame_clip: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The pose transfer (see ase_hip_retarget_pose) -> (local rotations f64 [T, Bt, 4], root translation f64 [T, 3])."""
    _rt_shape('retarget_pose', 'state_global f64 [T, M, 4], tpose_global f64 [M, 4], target_global f64 [Bt, 4], root_translation f64 [Tsrc, 3]',
              state_global.dim() == 3 and state_global.shape[2] == 4 and tpose_global.shape == state_global.shape[1:] and
              target_global.shape == (ancestor.numel(), 4) and root_translation.dim() == 2 and root_translation.shape[1] == 3 and
              params.shape == (12,) and
              all(t.dtype == torch.float64 for t in (state_global, tpose_global, target_global, root_translation, params)))
    _rt_shape('retarget_pose', 'rt_body int32 [M], ancestor / parent_indices int32 [Bt], clip tables int32 [C], frame_clip int32 [T]',
              rt_body.shape == (state_global.shape[1],) and ancestor.dim() == 1 and parent_indices.shape == ancestor.shape and
              clip_first.dim() == 1 and clip_first.shape == clip_num_frames.shape == src_first.shape and
              frame_clip.shape == (state_global.shape[0],) and
              all(t.dtype == torch.int32 for t in (rt_body, ancestor, parent_indices, clip_first, clip_num_frames, src_first, frame_clip)))
    return _backend().retarget_pose(*_rt_dev('retarget_pose', state_global, tpose_global, target_global, root_translation, params,
                                             rt_body, ancestor, parent_indices, clip_first, clip_num_frames, src_first, frame_clip))


@retarget_pose.register_fake
def _(state_global, tpose_global, target_global, root_translation, params, rt_body, ancestor, parent_indices, clip_first,
      clip_num_frames, src_first, frame_clip):
    T = state_global.shape[0]
    return state_global.new_empty(T, ancestor.shape[0], 4), state_global.new_empty(T, 3)


def _rt_motion_shapes(name, local_rotation, root_translation, local_translation, tree):
    _rt_shape(name, 'local_rotation f64 [T, B, 4], root_translation f64 [T, 3], local_translation f32 [B, 3], tree int32 [B, ld]',
              local_rotation.dim() == 3 and local_rotation.shape[2] == 4 and root_translation.shape == (local_rotation.shape[0], 3) and
              local_translation.shape == (local_rotation.shape[1], 3) and tree.dim() == 2 and tree.shape[0] == local_rotation.shape[1] and
              local_rotation.dtype == root_translation.dtype == torch.float64 and local_translation.dtype == torch.float32 and
              tree.dtype == torch.int32)


@torch.library.custom_op('ase_hip::retarget_hinge', mutates_args=(), device_types='cuda')
def retarget_hinge(local_rotation: torch.Tensor, root_translation: torch.Tensor, local_translation: torch.Tensor,
                   tree: torch.Tensor, roles: torch.Tensor) -> torch.Tensor:
    """project_joints from a table (see ase_hip_retarget_hinge) -> local rotations f64 [T, B, 4]."""
    _rt_motion_shapes('retarget_hinge', local_rotation, root_translation, local_translation, tree)
    _rt_shape('retarget_hinge', 'roles int32 [B, 6]', roles.shape == (local_rotation.shape[1], 6) and roles.dtype == torch.int32)
    return _backend().retarget_hinge(*_rt_dev('retarget_hinge', local_rotation, root_translation, local_translation, tree, roles))


@retarget_hinge.register_fake
def _(local_rotation, root_translation, local_translation, tree, roles):
    return torch.empty_like(local_rotation)


@torch.library.custom_op('ase_hip::retarget_ground', mutates_args=(), device_types='cuda')
def retarget_ground(local_rotation: torch.Tensor, root_translation: torch.Tensor, local_translation: torch.Tensor,
                    tree: torch.Tensor, clip_first: torch.Tensor, clip_num_frames: torch.Tensor) -> torch.Tensor:
    """Per clip the minimum of global z (see ase_hip_retarget_ground) -> f64 [C]."""
    _rt_motion_shapes('retarget_ground', local_rotation, root_translation, local_translation, tree)
    _rt_shape('retarget_ground', 'clip_first / clip_num_frames int32 [C]',
              clip_first.dim() == 1 and clip_first.shape == clip_num_frames.shape and clip_first.dtype == clip_num_frames.dtype == torch.int32)
    return _backend().retarget_ground(*_rt_dev('retarget_ground', local_rotation, root_translation, local_translation, tree,
                                               clip_first, clip_num_frames))


@retarget_ground.register_fake
def _(local_rotation, root_translation, local_translation, tree, clip_first, clip_num_frames):
    return local_rotation.new_empty(clip_first.shape[0])


@torch.library.custom_op('ase_hip::retarget_finish', mutates_args=(), device_types='cuda')
def retarget_finish(local_rotation: torch.Tensor, root_translation: torch.Tensor, min_z: torch.Tensor, params: torch.Tensor,
                    local_translation: torch.Tensor, tree: torch.Tensor, frame_clip: torch.Tensor
                    ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The grounded motion (see ase_hip_retarget_finish) -> (global rotation f64 [T, B, 4], global translation f64 [T, B, 3],
    rotation f32 [T, B, 4], root translation f32 [T, 3])."""
    _rt_motion_shapes('retarget_finish', local_rotation, root_translation, local_translation, tree)
    _rt_shape('retarget_finish', 'min_z f64 [C], params f64 [12], frame_clip int32 [T]',
              min_z.dim() == 1 and params.shape == (12,) and frame_clip.shape == (local_rotation.shape[0],) and
              min_z.dtype == params.dtype == torch.float64 and frame_clip.dtype == torch.int32)
    return _backend().retarget_finish(*_rt_dev('retarget_finish', local_rotation, root_translation, min_z, params, local_translation,
                                               tree, frame_clip))


@retarget_finish.register_fake
def _(local_rotation, root_translation, min_z, params, local_translation, tree, frame_clip):
    T, B = local_rotation.shape[0], local_rotation.shape[1]
    f = lambda *shape: local_rotation.new_empty(*shape, dtype=torch.float32)
    return torch.empty_like(local_rotation), local_rotation.new_empty(T, B, 3), f(T, B, 4), f(T, 3)


@torch.library.custom_op('ase_hip::retarget_velocity', mutates_args=(), device_types='cuda')
def retarget_velocity(global_rotation: torch.Tensor, global_translation: torch.Tensor, clip_first: torch.Tensor,
                      clip_num_frames: torch.Tensor, clip_fps: torch.Tensor, frame_clip: torch.Tensor
                      ) -> tuple[torch.Tensor, torch.Tensor]:
    """Filtered velocities (see ase_hip_retarget_velocity) -> (global velocity, global angular velocity), f32 [T, B, 3]."""
    T, B = global_rotation.shape[0], global_rotation.shape[1]
    _rt_shape('retarget_velocity', 'global_rotation f64 [T, B, 4], global_translation f64 [T, B, 3], clip_fps f64 [C]',
              global_rotation.dim() == 3 and global_rotation.shape[2] == 4 and global_translation.shape == (T, B, 3) and
              global_rotation.dtype == global_translation.dtype == clip_fps.dtype == torch.float64)
    _rt_shape('retarget_velocity', 'clip_first / clip_num_frames int32 [C], frame_clip int32 [T]',
              clip_first.dim() == 1 and clip_first.shape == clip_num_frames.shape == clip_fps.shape and frame_clip.shape == (T,) and
              all(t.dtype == torch.int32 for t in (clip_first, clip_num_frames, frame_clip)))
    return _backend().retarget_velocity(*_rt_dev('retarget_velocity', global_rotation, global_translation, clip_first, clip_num_frames,
                                                 clip_fps, frame_clip))


@retarget_velocity.register_fake
def _(global_rotation, global_translation, clip_first, clip_num_frames, clip_fps, frame_clip):
    f = lambda: global_translation.new_empty(global_translation.shape, dtype=torch.float32)
    return f(), f()
