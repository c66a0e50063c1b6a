"""Supplementary measurements on one MI355X (not the headline bench line): the other BASELINE configurations and the
rollout-time inference path.  One JSON line per measurement on stdout.

    python scripts/bench_extra.py [--updates 4]

  amp   : config 1's agent at full yaml width (amp_humanoid.yaml: [1024, 512] nets, no latents), 4096 x 32 batch
  hrl   : config 4's high-level PPO update (obs 258, action 64, [1024, 512]), 4096 x 32 batch
  ase16k: config 5's batch (16384 envs x 32 = 524288 samples, 192 optimisation steps), ASE nets
  ase-f32 / ase-bf16x3: config 2 in the parity / split precision modes
  ase-mixed: config 2 under the reference's `mixed_precision: True` (f16 + dynamic loss scale)
  ase-dyn-gpx3: the headline mode (f16gpx3) with `loss_scale: dynamic` instead of its static gradient scale
  shard : ONE rank's share of the sharded data-parallel update (BASELINE configs[2]) on one GPU, for R = 2, 4, 8 ranks: the
          48 optimisation steps of an update at minibatch 16384 / R, amp minibatch 4096 / R (--shard-of R[,R...]); no collectives
          - the compute side of the scaling curve the driver's 8-GPU run would take, and the launch count it has to hide
  env-tensors: the environment-side launches (policy observation, reset test, task observations / rewards) at 4096 and 16384
          environments under a launch program, next to the same functions as plain torch ops on the device (reported, not gated)
  amp-reset: the fused HumanoidAMP reset launch (motion-state rows, 10 history slots) for 64 and 4096 of 4096 environments under a
          launch program, next to the same result composed from the sampler and the frame builder (reported, not gated)
  rollout-store: what play_steps does behind env_step for one step of config 2 (4096 envs, obs 253, actions 31, amp 1400, latents
          64, dones at 1/300): the host block (some thirty torch launches and dones.nonzero's round trip) next to the one
          rollout_store call, eager and replayed from a launch program (reported, not gated)
  rollout-program: one play_steps() of config 2 on HumanoidEnv over PlaybackPhysics, the step issued call by call
            (device_rollout) against the step recorded once as a launch program (rollout_program), alternated
  env-step: one step's environment work of the strike task with an AMP history of 10 at 4096 and 16384 environments: the
          composition of the separate entries (eager, and replayed from a launch program) and env_pre_step + env_post_step
  hrl-step: the glue of one high-level HRL step around the frozen controller's dense layers at config 4's size (4096 envs,
          llc_steps 5, obs 253 + 5 task, actions 31, amp 1400, latents 64) - the default path's per-statement launches next to
          hrl_latent once and rms_normalize / hrl_llc_action / rms_normalize / hrl_accum per inner step, eager and replayed from a
          launch program; the dense layers and the environment are left out of both (reported, not gated)
  perturb: one _update_proj of the perturbation task at 4096 environments on a step that is not due and on a due step: the
          reference-style torch composition with its progress_buf.cpu() read next to one ProjectileLauncher.update call, eager
          and replayed from a launch program (reported, not gated)
  infer : get_action_values (eval-mode normalisation + actor + critic forward + sample) on 4096 observations
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ase_amd  # noqa: E402
ase_amd.configure(cpu_threads=1)     # hardware queues before HIP initialises; one torch CPU thread
import torch  # noqa: E402


SIGMA_FORMS = {  # network space.continuous of the log-std forms (rl_games learn_sigma / fixed_sigma)
    'frozen': None,
    'vector': dict(learn_sigma=True, fixed_sigma=True, sigma_init={'name': 'const_initializer', 'val': -2.9}),
    'head': dict(learn_sigma=True, fixed_sigma=False, sigma_init={'name': 'random_uniform_initializer', 'a': -0.02, 'b': 0.02}),
}


def build(kind, num_envs, precision, graph=True, overrides=None, net_overrides=None, sigma=None):
    from ase_amd import cfg as defaults
    from ase_amd.learning import agents, models
    from ase_amd.learning.network_builder import AMPBuilder, ASEBuilder, HRLBuilder
    from ase_amd.synthetic import EnvSpec, SyntheticSource
    net_p, cfg = defaults.get(kind)
    cfg.update({k: v for k, v in (overrides or {}).items() if k == 'horizon_length'})
    for part, units in (net_overrides or {}).items():
        net_p[part]['units'] = list(units)
    if SIGMA_FORMS.get(sigma):
        net_p['space']['continuous'].update(SIGMA_FORMS[sigma])
    obs, act, amp = {'ase': (253, 31, 1400), 'amp': (253, 31, 1400), 'hrl': (258, 64, 0)}[kind]
    z = cfg.get('latent_dim', 0) if kind == 'ase' else 0
    spec = EnvSpec(num_envs=num_envs, horizon=cfg['horizon_length'], obs_size=obs, act_size=act, amp_obs_size=amp,
                   latent_dim=z, latent_steps_min=cfg.get('latent_steps_min', 1), latent_steps_max=cfg.get('latent_steps_max', 150))
    torch.manual_seed(0)
    B, M, A = {'ase': (ASEBuilder, models.ModelASEContinuous, agents.ASEAgent),
               'amp': (AMPBuilder, models.ModelAMPContinuous, agents.AMPAgent),
               'hrl': (HRLBuilder, models.ModelHRLContinuous, agents.CommonAgent)}[kind]
    b = B()
    b.load(net_p)
    sp = lambda n: types.SimpleNamespace(shape=(n,))
    cfg = dict(cfg)
    cfg.update(overrides or {})
    info = {'observation_space': sp(obs), 'action_space': sp(act)}
    if amp:
        info['amp_observation_space'] = sp(amp)
    cfg.update(network=M(b), num_actors=num_envs, device='cuda:0', precision=precision, graph_capture=graph,
               vec_env=SyntheticSource(spec, seed=1236), env_info=info)
    if precision == 'mixed':          # the reference's own flag and nothing else: f16 storage + the dynamic loss scale (GradScaler)
        del cfg['precision']
        cfg['mixed_precision'] = True
    elif precision.endswith('+dyn'):  # a named mode with GradScaler's dynamic scale instead of its static one
        cfg['precision'] = precision[:-4]
        cfg['loss_scale'] = 'dynamic'
    ag = A('extra', cfg)
    with torch.no_grad():
        ag.set_eval()
        exp = ag.vec_env.experience(ag._cpu_policy(), **ag._experience_kwargs())
        for k, v in exp.items():
            if k in ag.experience:
                ag.experience[k].copy_(v.to('cuda:0'))
        if amp:
            ag._init_amp_demo_buf()
    torch.cuda.synchronize()
    return ag, cfg, spec


def time_updates(ag, n):
    def one():
        return ag.update(ag._play_steps_tail())
    for _ in range(4):          # graph capture (two replay-source variants) + warm-up
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        one()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def env_tensors_case():
    """N5: every environment-side launch at 4096 and 16384 environments - HIP events around replays of a launch program that
    holds the call 50 times - next to the same function as plain torch ops on the same device (tests/emu_env_tensors.py, eager)."""
    from ase_amd import lib as L
    from ase_amd.backend import HipBackend
    from tests.emu_env_tensors import EmuEnvTensors
    be, emu, dev = HipBackend('cuda:0'), EmuEnvTensors(), 'cuda:0'
    B, F, REP = 17, 253, 50

    def events(fn, n):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    for N in (4096, 16384):
        g = torch.Generator().manual_seed(N)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)
        unit = lambda x: x / x.norm(dim=-1, keepdim=True)
        pos, rot, vel, ang = r(N, B, 3), unit(r(N, B, 4)), r(N, B, 3), r(N, B, 3)
        rs = torch.cat([pos[:, 0], rot[:, 0], vel[:, 0], ang[:, 0]], -1).contiguous()
        prev, tar_states = pos[:, 0] - r(N, 3) / 30, torch.cat([r(N, 3), unit(r(N, 4)), r(N, 6)], -1).contiguous()
        tar_dir, face, speed, tar2, tar3 = unit(r(N, 2)), unit(r(N, 2)), r(N).abs() + 1, r(N, 2), r(N, 3)
        contact, tar_contact, heights = r(N, B, 3), r(N, 3), torch.full((B,), 0.15, device=dev)
        progress = torch.randint(0, 300, (N,), generator=g).to(dev)
        obs, rew = torch.zeros(N, F + 15, device=dev), torch.zeros(N, device=dev)
        reset, term = torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
        dt = 1.0 / 30.0
        cases = [('humanoid_obs_max', lambda b: b.humanoid_obs_max(pos, rot, vel, ang, True, True, obs), N * (B * 13 + F) * 4),
                 ('humanoid_reset', lambda b: b.humanoid_reset(progress, contact, pos, heights, [11, 14], 300.0, True, reset, term),
                  N * (B * 6 * 4 + 24)),
                 ('humanoid_reset (strike form)', lambda b: b.humanoid_reset(progress, contact, pos, heights, [11, 14], 300.0, True, reset,
                                                                             term, tar_contact, [4, 5, 6, 8, 9, 10]), N * (B * 6 * 4 + 36))]
        ops = {'heading': (dict(root_states=rs, tar_a=tar_dir, tar_b=face, tar_speed=speed),
                           dict(root_states=rs, prev_root_pos=prev, tar_a=tar_dir, tar_b=face, tar_speed=speed, dt=dt)),
               'location': (dict(root_states=rs, tar_a=tar2), dict(root_states=rs, prev_root_pos=prev, tar_a=tar2, tar_speed=1.0, dt=dt)),
               'reach': (dict(root_states=rs, tar_a=tar3), dict(tar_a=tar3, body_pos=pos, body_id=5)),
               'strike': (dict(root_states=rs, tar_states=tar_states), dict(root_states=rs, prev_root_pos=prev, tar_states=tar_states, dt=dt))}
        for k, (task, (okw, rkw)) in enumerate(ops.items()):
            cases.append((f'task_obs {task}', lambda b, k=k, okw=okw: b.task_obs(k, obs, F, None, **okw), None))
            cases.append((f'task_reward {task}', lambda b, k=k, rkw=rkw: b.task_reward(k, rew, **rkw), None))
        assert list(ops) == ['heading', 'location', 'reach', 'strike'] and L.TASK_STRIKE == 3
        for name, call, byt in cases:
            prog = be.prog_create()
            be.prog_begin(prog)
            for _ in range(REP):
                call(be)
            be.prog_end(prog)
            us = events(lambda: be.prog_launch(prog), 400) / REP
            be.prog_destroy(prog)
            us_torch = events(lambda: call(emu), 100)
            line = {'measurement': 'env-tensors ' + name, 'envs': N, 'us_per_call': round(us, 2), 'torch_ops_us_per_call': round(us_torch, 1),
                    'ratio': round(us_torch / us, 1), 'how': f'HIP events around 400 replays of a launch program of {REP} calls (operands stay cache-resident); '
                    'torch leg: the same function as eager torch ops on the device, 100 calls', 'device': torch.cuda.get_device_name(0)}
            if byt:
                line.update(bytes=byt, GB_per_s=round(byt / us / 1e3, 1))
            print(json.dumps(line), flush=True)


def amp_reset_case():
    """N6: ase_hip_amp_reset for n_ids of 4096 environments, every row a motion-state row - HIP events around replays of a launch
    program that holds the call 50 times - next to the same result built from the entries that existed before it: motion_state at
    the sampled times, three indexed writes, build_amp_obs of the current frame, motion_state at the S - 1 earlier times per row,
    build_amp_obs into a temporary, two indexed writes into the history (eager: the torch ops between the launches cannot be
    recorded)."""
    from ase_amd import lib as L
    from ase_amd.backend import HipBackend
    from ase_amd.motion_lib import DeviceMotionLib
    be, dev = HipBackend('cuda:0'), 'cuda:0'
    clips = torch.load(os.path.join(ROOT, 'tests', 'golden', 'motion_state.pt'), weights_only=False)['clips']
    ml = DeviceMotionLib.from_arrays(clips, be, dev)
    c = ml.clips
    N, B, S, REP, dt = 4096, c['gts'].shape[1], 10, 50, 1.0 / 30.0
    D, J, K, kb = c['dof_offsets'][-1], len(c['dof_body_ids']), len(c['key_body_ids']), c['key_body_ids']
    F = 13 + 6 * J + D + 3 * K

    def events(fn, n):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    pos, rot, vel, ang = r(N, B, 3), r(N, B, 4), r(N, B, 3), r(N, B, 3)
    rot = (rot / rot.norm(dim=-1, keepdim=True)).contiguous()
    root, dof_pos, dof_vel, hist = r(N, 13), r(N, D), r(N, D), torch.zeros(N, S, F, device=dev)
    for n_ids in (64, 4096):
        ids = torch.randperm(N, generator=g)[:n_ids].to(torch.int32).to(dev)
        mids = torch.randint(0, ml.num_motions(), (n_ids,), generator=g).to(torch.int32).to(dev)
        times = (torch.rand(n_ids, generator=g).to(dev) * c['lengths'][mids.long()]).contiguous()
        kind = torch.full_like(ids, L.RESET_MOTION)

        def fused():
            be.amp_reset(c, ids, kind, mids, times, None, None, root, dof_pos, dof_vel, pos, rot, vel, ang, True, True, dt, hist,
                         L.RESET_HAS_MOTION)

        idl = ids.long()
        cur, past = torch.zeros(n_ids, 1, F, device=dev), torch.zeros(n_ids * (S - 1), 1, F, device=dev)
        mids_h = mids.view(-1, 1).expand(n_ids, S - 1).reshape(-1).contiguous()
        steps = -dt * (torch.arange(0, S - 1, device=dev) + 1)

        def composed():
            rp, rq, dp, rv, rw, dv, _ = be.motion_state(c, mids, times)
            root[idl] = torch.cat([rp, rq, rv, rw], -1)
            dof_pos[idl] = dp
            dof_vel[idl] = dv
            be.build_amp_obs(pos[idl, 0], rot[idl, 0], vel[idl, 0], ang[idl, 0], dp, dv, pos[idl][:, kb].contiguous(), c['dof_offsets'],
                             True, True, cur, shift=False)
            st = be.motion_state(c, mids_h, (times.unsqueeze(-1) + steps).reshape(-1))
            be.build_amp_obs(st[0], st[1], st[3], st[4], st[2], st[5], st[6], c['dof_offsets'], True, True, past, shift=False)
            hist[idl, 0] = cur[:, 0]
            hist[idl, 1:] = past.view(n_ids, S - 1, F)

        composed()
        want = (root.clone(), dof_pos.clone(), hist.clone())
        hist.zero_()
        fused()
        torch.cuda.synchronize()
        diff = max(float((a - b).abs().max()) for a, b in zip(want, (root, dof_pos, hist)))
        prog = be.prog_create()
        be.prog_begin(prog)
        for _ in range(REP):
            fused()
        be.prog_end(prog)
        us = events(lambda: be.prog_launch(prog), 400) / REP
        be.prog_destroy(prog)
        us_eager = events(fused, 200)
        us_comp = events(composed, 100)
        byt = n_ids * (S * F + 13 + 2 * D) * 4
        print(json.dumps({'measurement': 'amp-reset motion rows', 'envs': N, 'n_ids': n_ids, 'history_slots': S, 'us_per_call': round(us, 2),
                          'eager_us_per_call': round(us_eager, 1), 'composed_us_per_call': round(us_comp, 1),
                          'ratio': round(us_comp / us, 1), 'max_abs_diff_to_composed': diff, 'bytes_written': byt,
                          'how': f'HIP events around 400 replays of a launch program of {REP} calls (operands stay cache-resident); eager: '
                          '200 calls from Python; composed: motion_state x2, build_amp_obs x2 and the torch indexed writes, eager, 100 calls',
                          'device': torch.cuda.get_device_name(0)}), flush=True)


def rollout_store_case():
    """One environment step's stores of config 2, three ways on the same tensors.  Calls are issued back to back and timed
    between two events - the larger of host and GPU time; the host block waits for the device in every call (nonzero).  Seven
    repeats of 100 calls each: median and spread."""
    from ase_amd.backend import HipBackend
    from ase_amd.learning.agents import AverageMeter
    be = HipBackend('cuda:0')
    g = torch.Generator().manual_seed(0)
    N, H, OBS, ACT, AMP, Z = 4096, 32, 253, 31, 1400, 64
    dev = 'cuda:0'
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    E = {'actions': (ACT,), 'neglogpacs': (), 'values': (1,), 'mus': (ACT,), 'sigmas': (ACT,), 'next_obses': (OBS,), 'rewards': (1,),
         'next_values': (1,), 'amp_obs': (AMP,), 'rand_action_mask': (), 'ase_latents': (Z,)}
    E = {k: torch.zeros(H, N, *shp, device=dev) for k, shp in E.items()}
    E['dones'] = torch.zeros(H, N, dtype=torch.uint8, device=dev)
    res = {'actions': rnd(N, ACT), 'neglogpacs': rnd(N), 'values': rnd(N, 1), 'mus': rnd(N, ACT), 'sigmas': rnd(N, ACT),
           'rand_action_mask': torch.ones(N, device=dev)}
    obs, amp_obs, latents, next_values = rnd(N, OBS), rnd(N, AMP), rnd(N, Z), rnd(N, 1)
    rewards = torch.ones(N, 1, device=dev)
    dones_b = torch.rand(N, generator=g) < 1.0 / 300
    dones = dones_b.to(torch.uint8).to(dev)
    terminate = (dones_b & (torch.rand(N, generator=g) < 0.5)).to(dev)
    shift, scale, n = 0.0, 1.0, 5

    class Host:          # CommonAgent.play_steps' statements behind env_step, with the ASE agent's _rollout_extras
        current_rewards = torch.zeros(N, 1, device=dev)
        current_lengths = torch.zeros(N, device=dev)
        game_rewards, game_lengths = AverageMeter(1, 100), AverageMeter(1, 100)

    def host_block(a=Host):
        for k in ('actions', 'neglogpacs', 'values', 'mus', 'sigmas'):
            E[k][n].copy_(res[k].view(E[k][n].shape))
        E['rewards'][n].copy_((rewards + shift) * scale)
        E['next_obses'][n].copy_(obs)
        E['dones'][n].copy_(dones)
        E['amp_obs'][n].copy_(amp_obs)
        E['rand_action_mask'][n].copy_(res['rand_action_mask'])
        E['ase_latents'][n].copy_(latents)
        terminated = terminate.float().unsqueeze(-1)
        E['next_values'][n].copy_(next_values * (1.0 - terminated))
        a.current_rewards += rewards
        a.current_lengths += 1
        all_done_indices = dones.nonzero(as_tuple=False)
        done_indices = all_done_indices[::1]
        a.game_rewards.update(a.current_rewards[done_indices])
        a.game_lengths.update(a.current_lengths[done_indices])
        not_dones = 1.0 - dones.float()
        a.current_rewards = a.current_rewards * not_dones.unsqueeze(1)
        a.current_lengths = a.current_lengths * not_dones
        done_indices = done_indices[:, 0]

    cur_r, cur_l = torch.zeros(N, 1, device=dev), torch.zeros(N, device=dev)
    meter, ids = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    fields = [(res[k], E[k]) for k in ('actions', 'neglogpacs', 'values', 'mus', 'sigmas')] + \
        [(obs, E['next_obses']), (amp_obs, E['amp_obs']), (res['rand_action_mask'], E['rand_action_mask']), (latents, E['ase_latents'])]

    def one_call():
        be.rollout_store(dones, slot=n, fields=fields, rewards=rewards, shift=shift, scale=scale, rewards_out=E['rewards'],
                         dones_out=E['dones'], next_values=next_values, terminate=terminate, next_values_out=E['next_values'],
                         cur_rewards=cur_r, cur_lengths=cur_l, meter=meter, max_size=100, done_ids_out=ids)
    prog = be.prog_create()
    be.prog_begin(prog)
    one_call()
    be.prog_end(prog)

    def timeit(fn, calls=100):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls * 1e3
    byt = sum(2 * 4 * N * int(s.shape[1] if s.dim() > 1 else 1) for s, _ in fields) + N * (4 * 4 + 4 * 4 + 3)
    for name, fn in (('rollout step stores, host block (play_steps behind env_step, with dones.nonzero)', host_block),
                     ('rollout step stores, one rollout_store call', one_call),
                     ('rollout step stores, one rollout_store call replayed from a launch program', lambda: be.prog_launch(prog))):
        reps = sorted(timeit(fn) for _ in range(7))
        print(json.dumps({'measurement': name, 'envs': N, 'done_rows': int(dones_b.sum()), 'bytes': byt,
                          'us_per_call_median': round(reps[3], 1), 'us_per_call_min': round(reps[0], 1),
                          'us_per_call_max': round(reps[-1], 1), 'repeats': 7, 'calls_per_repeat': 100}), flush=True)
    be.prog_destroy(prog)


def perturb_case():
    """HumanoidPerturb._update_proj at 4096 environments, 13 projectiles behind one actor, three ways on the same tensors, on a
    step that is not due (progress_buf[0] = 59) and on a due step (60).  The torch composition is the reference's statements
    (env/tasks/humanoid_perturb.py:172-213) on the device, its host read of progress_buf included.  Timed as rollout_store_case:
    seven repeats of 100 calls, median and spread."""
    import numpy as np
    from ase_amd.backend import HipBackend
    from ase_amd.perturb import PERTURB_OBJS, ProjectileLauncher
    be = HipBackend('cuda:0')
    g = torch.Generator().manual_seed(0)
    N, A, B, dev = 4096, 14, 15, 'cuda:0'
    K = len(PERTURB_OBJS)
    root_states = torch.randn(N * A, 13, generator=g).to(dev)
    rb = torch.randn(N, B, 13, generator=g).to(dev)
    view = root_states.view(N, A, 13)
    humanoid_root_states, proj_states = view[:, 0], view[:, A - K:]
    rigid_body_pos, rigid_body_vel = rb[..., 0:3], rb[..., 7:10]
    progress_buf = torch.zeros(N, dtype=torch.int64, device=dev)
    perturb_timesteps = np.cumsum(PERTURB_OBJS)

    def torch_update():
        curr_timestep = progress_buf.cpu().numpy()[0]
        curr_timestep = curr_timestep % (perturb_timesteps[-1] + 1)
        perturb_step = np.where(perturb_timesteps == curr_timestep)[0]
        if len(perturb_step) > 0:
            perturb_id = perturb_step[0]
            n = N
            humanoid_root_pos = humanoid_root_states[..., 0:3]
            rand_theta = torch.rand([n], dtype=proj_states.dtype, device=proj_states.device)
            rand_theta *= 2 * np.pi
            rand_dist = (5 - 4) * torch.rand([n], dtype=proj_states.dtype, device=proj_states.device) + 4
            pos_x = rand_dist * torch.cos(rand_theta)
            pos_y = -rand_dist * torch.sin(rand_theta)
            pos_z = (2 - 0.25) * torch.rand([n], dtype=proj_states.dtype, device=proj_states.device) + 0.25
            proj_states[..., perturb_id, 0] = humanoid_root_pos[..., 0] + pos_x
            proj_states[..., perturb_id, 1] = humanoid_root_pos[..., 1] + pos_y
            proj_states[..., perturb_id, 2] = pos_z
            proj_states[..., perturb_id, 3:6] = 0.0
            proj_states[..., perturb_id, 6] = 1.0
            launch_tar_pos = rigid_body_pos[..., 1, :]
            launch_dir = launch_tar_pos - proj_states[..., perturb_id, 0:3]
            launch_dir += 0.1 * torch.randn_like(launch_dir)
            launch_dir = torch.nn.functional.normalize(launch_dir, dim=-1)
            launch_speed = (40 - 30) * torch.rand_like(launch_dir[:, 0:1]) + 30
            launch_vel = launch_speed * launch_dir
            launch_vel[..., 0:2] += rigid_body_vel[..., 1, 0:2]
            proj_states[..., perturb_id, 7:10] = launch_vel
            proj_states[..., perturb_id, 10:13] = 0.0

    la = ProjectileLauncher(be, N, device=dev)
    state = dict(humanoid_root_states=humanoid_root_states, rigid_body_pos=rigid_body_pos, rigid_body_vel=rigid_body_vel,
                 proj_states=proj_states)
    prog = be.prog_create()
    be.prog_begin(prog)
    la.update(state, progress_buf)
    be.prog_end(prog)

    def timeit(fn, calls=100):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls * 1e3
    for p0, what in ((59, 'not due'), (60, 'due')):
        progress_buf[0] = p0
        for name, fn in (('torch composition with the progress_buf.cpu() read', torch_update),
                         ('one ProjectileLauncher.update call', lambda: la.update(state, progress_buf)),
                         ('one ProjectileLauncher.update call replayed from a launch program', lambda: be.prog_launch(prog))):
            reps = sorted(timeit(fn) for _ in range(7))
            print(json.dumps({'measurement': f'perturb _update_proj, {what} step, {name}', 'envs': N, 'projectiles': K,
                              'progress_buf0': p0, 'us_per_call_median': round(reps[3], 1), 'us_per_call_min': round(reps[0], 1),
                              'us_per_call_max': round(reps[-1], 1), 'repeats': 7, 'calls_per_repeat': 100}), flush=True)
    be.prog_destroy(prog)


def hrl_step_case():
    """The glue of one high-level step of config 4 (HRLAgent.env_step around the LLC's dense layers and vec_env.step), both ways on
    the same tensors: the default path's statements (ForwardEngine.policy_forward / amp_heads / _calc_disc_rewards and the torch
    lines of env_step, dense layers left out) and the device_llc_step sequence.  Steps are issued back to back and timed between
    two events - the larger of host and GPU time.  Seven repeats of 100 high-level steps each: median and spread."""
    from ase_amd.backend import HipBackend
    from ase_amd.forward import P
    from ase_amd.learning.agents import rescale_actions
    be = HipBackend('cuda:0')
    g = torch.Generator().manual_seed(0)
    N, T, OBS, TASK, ACT, AMP, Z = 4096, 5, 253, 5, 31, 1400, 64
    dev, bf16, f32 = 'cuda:0', torch.bfloat16, torch.float32
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    obs, amp_obs, actions = rnd(N, OBS + TASK), rnd(N, AMP), rnd(N, Z) * 1.5
    MU, HD = rnd(N, P(ACT)), rnd(N, 64)                          # the padded head outputs the dense layers leave behind
    low, high = -torch.rand(ACT, generator=g).to(dev) - 0.5, torch.rand(ACT, generator=g).to(dev) + 0.5
    rewards = torch.ones(N, device=dev)
    dones = (torch.rand(N, generator=g) < 1.0 / 300).to(torch.uint8).to(dev)
    terminate = (torch.rand(N, generator=g) < 1.0 / 600).to(dev)
    obs_state = torch.cat([rnd(OBS).double(), torch.rand(OBS, generator=g).double().to(dev) + 0.5, torch.ones(1, dtype=torch.float64, device=dev)])
    amp_state = torch.cat([rnd(AMP).double(), torch.rand(AMP, generator=g).double().to(dev) + 0.5, torch.ones(1, dtype=torch.float64, device=dev)])
    kpad = P(OBS) + P(Z)
    Xa, Xc, Zs, Xd = (torch.zeros(N, c, dtype=bf16, device=dev) for c in (kpad, kpad, P(Z), P(AMP)))
    z, mu = torch.zeros(N, Z, device=dev), torch.zeros(N, ACT, device=dev)
    om, os_, am, as_ = (torch.zeros(1, c, device=dev) for c in (OBS, OBS, AMP, AMP))
    scale = 2.0

    def default_path():
        a = torch.clamp(actions, -1.0, 1.0)
        r = dr = dc = tc = 0.0
        for t in range(T):
            llc_obs = obs[..., :OBS].contiguous()
            be.normalize_rows(a, z, N, Z)
            be.rms_finalize(obs_state, OBS, None, 0, 0, om, os_)
            be.rms_normalize(llc_obs, OBS, None, (0, 0), N, om[0], os_[0], [Xa, Xc])
            be.gather_rows(z, Z, None, (0, 0), N, Xc[:, P(OBS):])
            be.gather_rows(z, Z, None, (0, 0), N, Zs)
            be.gather_rows(MU, ACT, None, (0, 0), N, mu)
            rescale_actions(low, high, torch.clamp(mu, -1.0, 1.0))
            be.rms_finalize(amp_state, AMP, None, 0, 0, am, as_)
            be.rms_normalize(amp_obs, AMP, None, (0, 0), N, am[0], as_[0], [Xd])
            d = torch.empty(N, 1, dtype=f32, device=dev)
            be.disc_reward(HD, d, N, scale)
            r = r + rewards
            dc = dc + dones.float()
            tc = tc + terminate.float()
            dr = dr + d
        r, dr = r / T, dr / T
        return r, dr, (dc > 0).to(dc.dtype), (tc > 0).to(tc.dtype)

    acc, outs, env_actions = torch.zeros(4, N, device=dev), torch.zeros(4, N, device=dev), torch.zeros(N, ACT, device=dev)
    be.rms_finalize(obs_state, OBS, None, 0, 0, om, os_)        # the frozen statistics, once
    be.rms_finalize(amp_state, AMP, None, 0, 0, am, as_)

    def key_path():
        be.hrl_latent(actions, z2=Zs, dim=Z)
        for t in range(T):
            be.rms_normalize(obs[:, :OBS], OBS, None, (0, 0), N, om[0], os_[0], [Xa])
            be.hrl_llc_action(MU, low, high, env_actions, ACT)
            be.rms_normalize(amp_obs, AMP, None, (0, 0), N, am[0], as_[0], [Xd])
            be.hrl_accum(rewards, dones, acc, t == 0, t == T - 1, T, terminate=terminate, logit=HD, disc_scale=scale,
                         rewards_out=outs[0], disc_out=outs[1], dones_out=outs[2], terminate_out=outs[3])
    prog = be.prog_create()
    be.prog_begin(prog)
    key_path()
    be.prog_end(prog)
    entries = be.prog_size(prog)

    def timeit(fn, calls=100):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls * 1e3
    for name, fn, launches in (('hrl step glue, default path (per-statement launches, eager)', default_path, None),
                               ('hrl step glue, device_llc_step (eager)', key_path, entries),
                               ('hrl step glue, device_llc_step replayed from a launch program', lambda: be.prog_launch(prog), entries)):
        reps = sorted(timeit(fn) for _ in range(7))
        print(json.dumps({'measurement': name, 'envs': N, 'llc_steps': T, 'launches_per_step': launches,
                          'us_per_step_median': round(reps[3], 1), 'us_per_step_min': round(reps[0], 1),
                          'us_per_step_max': round(reps[-1], 1), 'repeats': 7, 'steps_per_repeat': 100}), flush=True)
    be.prog_destroy(prog)


def env_step_case():
    """One step's environment work of the strike task with an AMP history of 10 (N14), at 4096 and 16384 environments, on seeded
    state in the packed simulator layout, three ways on the same tensors: the composition HumanoidEnv(fused_step=False) makes of
    the separate entries (contiguous copies, torch glue) eager; the same recorded in a launch program (its torch glue as host
    calls); the two launches env_pre_step / env_post_step recorded.  The physics step itself and update_task (nothing for strike)
    are left out.  The three are alternated inside every repeat and timed between two events; seven repeats of 200 steps."""
    from ase_amd import lib as L
    from ase_amd.amp_env import action_to_pd_targets
    from ase_amd.backend import HipBackend
    be = HipBackend('cuda:0')
    dev, f32 = 'cuda:0', torch.float32
    offs = [0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31]
    keys, contact, strike = [5, 8, 11, 14, 6, 9], [11, 14], [4, 5, 6, 8, 9, 10]
    B, D, S, F, FA = 17, 31, 10, 253, 140
    for N in (4096, 16384):
        g = torch.Generator().manual_seed(N)
        rnd = lambda *s: torch.randn(*s, generator=g)
        rb = rnd(N, B + 1, 13)
        rb[:, :, 3:7] = rb[:, :, 3:7] / rb[:, :, 3:7].norm(dim=-1, keepdim=True)
        rb, dof, root = rb.to(dev), (rnd(N, D, 2) * 0.5).to(dev), rb[:, [0, B]].contiguous().to(dev)
        cf = (rnd(N, B + 1, 3) * (torch.rand(N, B + 1, 1, generator=g) < 0.3)).to(dev)
        pos, rot, vel, ang = rb[:, :B, 0:3], rb[:, :B, 3:7], rb[:, :B, 7:10], rb[:, :B, 10:13]
        rs, ts, cfb, tcf, dp, dv = root[:, 0], root[:, 1], cf[:, :B], cf[:, B], dof[:, :, 0], dof[:, :, 1]
        heights = torch.full((B,), 0.15, device=dev)
        actions_in = (rnd(N, D) * 0.8).to(dev)
        off, sc = rnd(D).to(dev), (torch.rand(D, generator=g) + 0.5).to(dev)

        def buffers():
            z = lambda *s, dt=f32: torch.zeros(*s, dtype=dt, device=dev)
            return dict(obs=z(N, F + 15), rew=z(N), reset=z(N, dt=torch.int64), term=z(N, dt=torch.int64), prog=z(N, dt=torch.int64),
                        hist=z(N, S, FA), acts=z(N, D), tg=z(N, D), prev=z(N, 3), cnt=z(N, dt=torch.int32))
        u, f = buffers(), buffers()

        # the composition's contiguous copies go into FIXED buffers (a replay needs stable addresses; an eager .contiguous()
        # would allocate on top of this)
        fixed = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in (pos, rot, vel, ang, cfb, rs, ts, tcf)]
        amp_in = [torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev),
                  torch.empty(N, D, device=dev), torch.empty(N, D, device=dev), torch.empty(N, len(keys), 3, device=dev)]

        def glue_pre():
            u['acts'].copy_(torch.clamp(actions_in, -1.0, 1.0))
            u['tg'].copy_(action_to_pd_targets(u['acts'], off, sc))
            u['prev'].copy_(rs[:, 0:3])
            u['cnt'].sub_(1).clamp_min_(0)
            u['prog'].add_(1)
            for dst, src in zip(fixed, (pos, rot, vel, ang, cfb, rs, ts, tcf)):
                dst.copy_(src)

        def glue_amp():
            rec = u['cnt'] > 0
            u['reset'].masked_fill_(rec, 0)
            u['term'].masked_fill_(rec, 0)
            for dst, src in zip(amp_in, (pos[:, 0], rot[:, 0], vel[:, 0], ang[:, 0], dp, dv, pos[:, keys])):
                dst.copy_(src)

        def composition(glue):
            cp, cr, cv, ca, cc, crs, cts, ctc = fixed
            glue(glue_pre)
            be.humanoid_obs_max(cp, cr, cv, ca, True, True, u['obs'], 0)
            be.task_obs(L.TASK_STRIKE, u['obs'], F, None, root_states=crs, tar_states=cts)
            be.task_reward(L.TASK_STRIKE, u['rew'], root_states=crs, prev_root_pos=u['prev'], tar_states=cts, dt=1.0 / 30.0)
            be.humanoid_reset(u['prog'], cc, cp, heights, contact, 300.0, True, u['reset'], u['term'], ctc, strike)
            glue(glue_amp)
            be.build_amp_obs(*amp_in, offs, True, True, u['hist'], shift=True)
            glue(lambda: u['obs'].clamp_(-5.0, 5.0))

        def eager():
            composition(lambda fn: fn())

        def fused():
            be.env_pre_step(actions_in, f['acts'], f['tg'], 1.0, pd_offset=off, pd_scale=sc, root_states=rs, prev_root_pos=f['prev'],
                            recovery_counter=f['cnt'])
            be.env_post_step(pos, rot, vel, ang, cfb, f['prog'], f['obs'], f['rew'], f['reset'], f['term'], heights, contact, 300.0, True,
                             True, True, clip_obs=5.0, task_kind=L.TASK_STRIKE, root_states=rs, prev_root_pos=f['prev'], tar_states=ts,
                             dt=1.0 / 30.0, tar_contact_forces=tcf, strike_body_ids=strike, recovery_counter=f['cnt'], hist=f['hist'],
                             dof_pos=dp, dof_vel=dv, dof_offsets=offs, key_body_ids=keys)
        eager()
        fused()
        torch.cuda.synchronize()
        same = all(torch.equal(u[k], f[k]) for k in ('obs', 'rew', 'reset', 'term', 'prog', 'hist', 'acts', 'tg', 'prev', 'cnt'))
        p_comp, p_fused = be.prog_create(), be.prog_create()
        be.prog_begin(p_comp)
        composition(be.host_call)
        be.prog_end(p_comp)
        be.prog_begin(p_fused)
        fused()
        be.prog_end(p_fused)
        variants = (('env step, composition of the separate entries (eager)', eager, None),
                    ('env step, composition of the separate entries replayed from a launch program', lambda: be.prog_launch(p_comp),
                     be.prog_size(p_comp)),
                    ('env step, env_pre_step + env_post_step replayed from a launch program', lambda: be.prog_launch(p_fused),
                     be.prog_size(p_fused)))
        times = {name: [] for name, _, _ in variants}
        for name, fn, _ in variants:                          # warm every shape
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(7):
            for name, fn, _ in variants:
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(200):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(e) / 200 * 1e3)
        for name, _, entries in variants:
            reps = sorted(times[name])
            print(json.dumps({'measurement': name, 'envs': N, 'task': 'strike', 'amp_obs_steps': S, 'program_entries': entries,
                              'outputs_bitwise_equal': same, 'us_per_step_median': round(reps[3], 1), 'us_per_step_min': round(reps[0], 1),
                              'us_per_step_max': round(reps[-1], 1), 'repeats': 7, 'steps_per_repeat': 200}), flush=True)
        be.prog_destroy(p_comp)
        be.prog_destroy(p_fused)


def rollout_program_case(rollouts=7, warmup=3):
    """One play_steps() of config 2 - 4096 environments, horizon 32, the real widths, ASE with device_latents and device_rollout -
    on HumanoidEnv over PlaybackPhysics (device-resident: SyntheticVecEnv draws on the CPU and would hide the difference), the
    step issued call by call (_play_steps_device) against the step recorded once as a launch program (rollout_program).  Two
    agents of the same seed on environments of the same recording; host wall time of one play_steps() ending in a device
    synchronise, after `warmup` rollouts of each (the program agent needs two before it replays), the two alternated inside one
    process, `rollouts` of each."""
    import statistics
    from ase_amd import cfg as defaults
    from ase_amd.backend import HipBackend
    from ase_amd.learning import agents, models
    from ase_amd.learning.network_builder import ASEBuilder
    from tests import env_step_cases as CS
    N, dev = 4096, 'cuda:0'
    Gf, clips, A = CS.load()
    small = CS.recording(Gf)
    reps = (N + Gf['num_envs'] - 1) // Gf['num_envs']
    frames = {k: v.repeat(1, reps, *([1] * (v.dim() - 2)))[:, :N].contiguous() for k, v in small.items()}

    def agent(**extra):
        be = HipBackend(dev)
        env = CS.make_env(be, 'cuda', Gf, clips, A, None, False, True, frames=frames,
                          cfg_update=dict(numAMPObsSteps=10, episodeLength=300))
        net_p, cfg = defaults.get('ase')
        torch.manual_seed(0)
        b = ASEBuilder()
        b.load(net_p)
        cfg = dict(cfg)
        info = {'observation_space': env.observation_space, 'action_space': env.action_space,
                'amp_observation_space': env.amp_observation_space}
        cfg.update(network=models.ModelASEContinuous(b), num_actors=N, device=dev, precision='bf16', backend=be, vec_env=env,
                   env_info=info, print_stats=False, device_latents=True, device_rollout=True, **extra)
        return agents.ASEAgent('rollout', cfg)
    eager, prog = agent(), agent(rollout_program=True)
    shapes = dict(obs=eager.obs_shape[0], actions=eager.actions_num, amp=eager.experience['amp_obs'].shape[-1],
                  latents=eager.experience['ase_latents'].shape[-1], horizon=eager.horizon_length)
    times = {'eager': [], 'program': []}

    def one(ag, seed):
        torch.manual_seed(seed)                   # (HumanoidEnv's host reset path draws from the global generator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ag.play_steps()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for i in range(warmup):
        one(eager, i)
        one(prog, i)
    assert prog._rp is not None
    for i in range(rollouts):
        times['eager'].append(one(eager, warmup + i))
        times['program'].append(one(prog, warmup + i))
    same = all(torch.equal(eager.experience[k], prog.experience[k]) for k in eager.experience)
    for name, ts in times.items():
        print(json.dumps({'measurement': 'rollout-program', 'path': name, 'envs': N, **shapes, 'precision': 'bf16',
                          'environment': 'HumanoidEnv over PlaybackPhysics (fused step)', 'ms_per_play_steps_mean': round(statistics.mean(ts), 3),
                          'ms_min': round(min(ts), 3), 'ms_max': round(max(ts), 3), 'ms_stdev': round(statistics.stdev(ts), 3),
                          'rollouts': rollouts, 'warmup': warmup, 'program_entries': prog.backend.prog_size(prog._rp['prog']),
                          'experience_equal_after_last_rollout': same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--updates', type=int, default=4)
    ap.add_argument('--only', default='')
    ap.add_argument('--shard-of', default='', help='comma list of rank counts R: time one rank\'s share of the sharded update')
    ap.add_argument('--precision', default='bf16')
    ap.add_argument('--engine-opts', default='', help='JSON dict of UpdateEngine.engine_opts overrides (the --shard-of runs)')
    ap.add_argument('--sigma', choices=sorted(SIGMA_FORMS), default=None,
                    help='time config 2 (ase, 4096 envs, --precision) with this log-std form: frozen / learned vector / sigma head')
    args = ap.parse_args()
    if args.sigma:
        ag, cfg, spec = build('ase', 4096, args.precision, sigma=args.sigma)
        dt = time_updates(ag, args.updates)
        print(json.dumps({'measurement': f'sigma-{args.sigma}', 'what': 'config 2 update with the log-std form ' + args.sigma,
                          'precision': args.precision, 'ms_per_update': round(dt * 1e3, 3),
                          'trainable': int(ag.model.a2c_network.trainable_numel)}), flush=True)
        return
    if args.shard_of:
        for R in [int(x) for x in args.shard_of.split(',')]:
            ov = {'minibatch_size': 16384 // R, 'amp_minibatch_size': 4096 // R}
            if args.engine_opts:
                ov['engine_opts'] = json.loads(args.engine_opts)
            ag, cfg, spec = build('ase', 4096, args.precision, overrides=ov)

            def one():
                return ag.update(ag._play_steps_tail(), max_steps=48)
            for _ in range(3):
                one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                one()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.updates
            progs = [g for g in ag._graphs.values() if not g['hipgraph']]
            entries = max((sum(ag.backend.prog_size(p) for p in g['graphs']) for g in progs), default=0)
            print(json.dumps({'measurement': f'shard-of-{R}', 'what': 'one rank\'s compute of the sharded data-parallel update: 48 '
                              f'optimisation steps at minibatch {16384 // R} / amp {4096 // R} rows + the epoch tail (whole batch: the tail '
                              'is sharded too in the real run), no collectives', 'ranks': R, 'ms_per_update': round(dt * 1e3, 3),
                              'us_per_step': round(dt * 1e6 / 48, 1), 'program_entries_per_step': entries, 'precision': args.precision,
                              'allreduce_bytes_per_step': int(ag.model.a2c_network.trainable_numel) * 4, 'gp_stream': bool(ag.engine._gp_side),
                              'ideal_us_per_step_from_1gpu': None}), flush=True)
            del ag
            torch.cuda.empty_cache()
        return
    # BASELINE configs[0] at its OWN size (64 envs x horizon 16, [256, 128] MLPs, minibatch 256 / amp 64, 24 optimisation steps):
    # the case the reference's CPU path is timed on (oracle/time_reference.py --config amp_cfg1) - launch-bound on a GPU
    cfg1 = dict(horizon_length=16, minibatch_size=256, mini_epochs=6, amp_minibatch_size=64, amp_batch_size=128,
                amp_obs_demo_buffer_size=512, amp_replay_buffer_size=2048)
    runs = [('amp', 'amp', 4096, 'bf16'), ('hrl', 'hrl', 4096, 'bf16'), ('ase16k', 'ase', 16384, 'bf16'),
            ('ase-f32', 'ase', 4096, 'f32'), ('ase-bf16x3', 'ase', 4096, 'bf16x3'), ('amp-cfg1', 'amp', 64, 'f32'),
            ('amp-cfg1-bf16', 'amp', 64, 'bf16'), ('ase-mixed', 'ase', 4096, 'mixed'), ('ase-dyn-gpx3', 'ase', 4096, 'f16gpx3+dyn')]
    for name, kind, envs, prec in runs:
        if args.only and name not in args.only.split(','):
            continue
        if name.startswith('amp-cfg1'):
            ag, cfg, spec = build(kind, envs, prec, overrides=cfg1, net_overrides={'mlp': [256, 128], 'disc': [256, 128]})
        else:
            ag, cfg, spec = build(kind, envs, prec, overrides=({'engine_opts': json.loads(args.engine_opts)} if args.engine_opts else None))
        dt = time_updates(ag, args.updates if (prec in ('bf16', 'mixed') or prec.endswith('+dyn')) else 2)
        B = ag.batch_size
        steps = cfg['mini_epochs'] * (B // cfg['minibatch_size'])
        print(json.dumps({'measurement': name, 'metric': 'PPO-update samples/sec', 'value': round(B / dt, 1), 'unit': 'samples/s',
                          'ms_per_update': round(dt * 1e3, 3), 'envs': envs, 'horizon': cfg['horizon_length'], 'batch': B,
                          'optimisation_steps': steps, 'precision': prec, 'params': int(ag.model.a2c_network.trainable_numel),
                          'replay': 'program', 'data': 'synthetic',
                          **({'loss_scaler': ag.engine.scaler_state(), 'what': ('config 2 under `mixed_precision: True`: f16 storage' if prec == 'mixed'
                              else 'config 2 in the headline mode with `loss_scale: dynamic`') + '; GradScaler on the device, per step: overflow '
                              'reported by the producing launches (scale records), skipped step + backoff / growth in front of the fused '
                              'optimizer launch, cross-step schedule kept'}
                             if ag.engine.dyn_scale else {})}), flush=True)
        del ag
        torch.cuda.empty_cache()
    if not args.only or 'infer' in args.only.split(','):
        ag, cfg, spec = build('ase', 4096, 'bf16', graph=False)
        obs = ag.experience['obses'][0].contiguous()
        z = ag.experience['ase_latents'][0].contiguous()
        ag.set_eval()
        for _ in range(5):
            ag.get_action_values({'obs': obs}, z)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 200
        for _ in range(n):
            ag.get_action_values({'obs': obs}, z)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        print(json.dumps({'measurement': 'infer', 'metric': 'rollout inference (get_action_values) env-steps/sec',
                          'value': round(4096 / dt, 1), 'unit': 'env-steps/s', 'us_per_call': round(dt * 1e6, 1), 'envs': 4096,
                          'precision': 'bf16', 'hipgraph': False}), flush=True)
    if not args.only or 'env-tensors' in args.only.split(','):
        env_tensors_case()
    if not args.only or 'amp-reset' in args.only.split(','):
        amp_reset_case()
    if not args.only or 'rollout-store' in args.only.split(','):
        rollout_store_case()
    if not args.only or 'perturb' in args.only.split(','):
        perturb_case()
    if not args.only or 'hrl-step' in args.only.split(','):
        hrl_step_case()
    if not args.only or 'env-step' in args.only.split(','):
        env_step_case()
    if not args.only or 'rollout-program' in args.only.split(','):
        rollout_program_case()
    if not args.only or 'ampobs' in args.only.split(','):
        # N2: observation production for 4096 envs (one frame + history push) and 5120 demo samples (512 x 10 steps)
        from ase_amd.backend import HipBackend
        be = HipBackend('cuda:0')
        g = torch.Generator().manual_seed(0)
        offs = [0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31]
        N, D, K, S = 4096, 31, 6, 10
        q = torch.randn(N, 4, generator=g)
        q = (q / q.norm(dim=-1, keepdim=True)).cuda()
        st = [torch.randn(N, 3, generator=g).cuda(), q, torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda(),
              (torch.randn(N, D, generator=g) * 0.5).cuda(), torch.randn(N, D, generator=g).cuda(), torch.randn(N, K, 3, generator=g).cuda()]
        hist = torch.zeros(N, S, 140, device='cuda')

        def timeit(fn, n=200):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / n * 1e3
        us = timeit(lambda: be.build_amp_obs(*st, offs, True, True, hist, shift=True))
        byt = N * (S * 140 * 4 * 2 + (13 + 2 * D + 3 * K) * 4)
        print(json.dumps({'measurement': 'amp-obs frame + history push', 'envs': N, 'us_per_call': round(us, 1),
                          'GB_per_s': round(byt / us / 1e3, 1), 'bytes': byt}), flush=True)
        F_, B = 4000, 17
        lr = torch.randn(F_, B, 4, generator=g)
        clips = {'gts': torch.randn(F_, B, 3, generator=g).cuda(), 'grs': (lr / lr.norm(dim=-1, keepdim=True)).cuda(),
                 'lrs': (lr / lr.norm(dim=-1, keepdim=True)).cuda(), 'grvs': torch.randn(F_, 3, generator=g).cuda(),
                 'gravs': torch.randn(F_, 3, generator=g).cuda(), 'dvs': torch.randn(F_, D, generator=g).cuda(),
                 'lengths': torch.full((40,), 3.3).cuda(), 'dt': torch.full((40,), 1 / 30).cuda(),
                 'num_frames': torch.full((40,), 100, dtype=torch.int32).cuda(),
                 'length_starts': (torch.arange(40, dtype=torch.int32) * 100).cuda(),
                 'dof_body_ids': [1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16], 'dof_offsets': offs, 'key_body_ids': [5, 10, 13, 16, 6, 9]}
        n = 5120
        ids = torch.randint(0, 40, (n,), generator=g).to(torch.int32).cuda()
        tt = (torch.rand(n, generator=g) * 3.3).cuda()
        us = timeit(lambda: be.motion_state(clips, ids, tt))
        print(json.dumps({'measurement': 'motion-clip sampler', 'samples': n, 'us_per_call': round(us, 1)}), flush=True)
        # the wired pipeline: HumanoidAMP.fetch_amp_obs_demo for one demo-ring refill of config 2 (amp_batch_size 512 samples x 10 frames)
        from ase_amd.motion_lib import AmpObsDemoSource, DeviceMotionLib
        host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in clips.items()}
        ml = DeviceMotionLib.from_arrays(host, be, 'cuda:0')
        src = AmpObsDemoSource(ml, be, num_amp_obs_steps=10, dt=1.0 / 30.0)
        for ns in (512, 4096):
            us = timeit(lambda: src.fetch_amp_obs_demo(ns), n=100)
            print(json.dumps({'measurement': 'fetch_amp_obs_demo (sample motions + times, motion state, 10-frame observations)',
                              'samples': ns, 'us_per_call': round(us, 1), 'out_bytes': ns * 1400 * 4}), flush=True)
        # one demo-ring refill of config 2 (512 samples x 10 frames; the ring here has 8192 rows, its size does not enter), both
        # ways in this process: the host-driven chain (torch draws, two launches, staging tensor, ring_store) and the one launch
        # that draws on the device and stores into the ring itself (N11).  Seven repeats of 100 calls each: median and spread.
        # Calls are issued back to back and timed between two events, as every figure above: the larger of host and GPU time.
        from ase_amd.learning.replay_buffer import ReplayBuffer
        ring_a, ring_b = ReplayBuffer(8192, 'cuda:0', be), ReplayBuffer(8192, 'cuda:0', be)
        ways = (('demo-ring refill, host-driven chain (fetch_amp_obs_demo + ring_store)', lambda: ring_a.store(src.fetch_amp_obs_demo(512))),
                ('demo-ring refill, one launch (amp_demo_fetch into the ring)', lambda: ring_b.store_with(src.fetch_into, 512, 1400)))
        for name, fn in ways:
            reps = sorted(timeit(fn, n=100) for _ in range(7))
            print(json.dumps({'measurement': name, 'samples': 512, 'frames': 10, 'us_per_call_median': round(reps[3], 1),
                              'us_per_call_min': round(reps[0], 1), 'us_per_call_max': round(reps[-1], 1), 'repeats': 7,
                              'calls_per_repeat': 100}), flush=True)


if __name__ == '__main__':
    main()
