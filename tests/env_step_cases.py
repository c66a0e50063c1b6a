"""Shared set-up of tests/test_env_step_emu.py and tests/test_gpu_env_step.py: the state of tests/golden/env_tensors.pt in the
packed simulator layout (with seeded dof state for the AMP frame), a ``PlaybackPhysics`` recording made of it, and the driver
that runs a ``HumanoidEnv`` for a number of steps the way an agent's rollout loop does.  TEST INFRASTRUCTURE ONLY."""
import os

import torch

from ase_amd.humanoid_env import HumanoidEnv, PlaybackPhysics
from ase_amd.motion_lib import DeviceMotionLib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TASKS = (None, 'heading', 'location', 'reach', 'strike')
BODY_NAMES = [f'b{i}' for i in range(17)]


def load():
    G = torch.load(os.path.join(GOLDEN, 'env_tensors.pt'), weights_only=False)
    clips = torch.load(os.path.join(GOLDEN, 'motion_state.pt'), weights_only=False)['clips']
    A = torch.load(os.path.join(GOLDEN, 'amp_reset.pt'), weights_only=False)
    return G, clips, A


def dof_state(n, D, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, 2, generator=g) * 0.5


def packed(i, dof, extra_body=True):
    """The fixture's inputs `i` as one frame of packed simulator tensors: [n, B (+ 1), 13] rigid bodies, [n, D, 2] dofs,
    [n, 2, 13] root states (actor 1: the strike target), [n, B (+ 1), 3] contact forces (the last body: the target's)."""
    n, B = i['body_pos'].shape[:2]
    bpe = B + (1 if extra_body else 0)
    rb = torch.full((n, bpe, 13), 7.0)
    rb[:, :B, 0:3], rb[:, :B, 3:7], rb[:, :B, 7:10], rb[:, :B, 10:13] = i['body_pos'], i['body_rot'], i['body_vel'], i['body_ang_vel']
    root = torch.stack([i['root_states'], i['tar_states']], 1)
    cf = torch.full((n, bpe, 3), 7.0)
    cf[:, :B] = i['contact_forces']
    if extra_body:
        rb[:, B] = i['tar_states']
        cf[:, B] = i['tar_contact_forces']
    return {'rigid_body_state': rb, 'dof_state': dof.clone(), 'root_states': root, 'contact_forces': cf}


def recording(G, T=6, shift=7, n=None):
    """T frames: frame t is the fixture with its environments rotated by shift * t rows, so every environment meets the
    fixture's falling, contact and target cases in turn.  Data only: no dynamics."""
    i = G['inputs']
    N = G['num_envs']
    dof = dof_state(N, 31)
    frames = []
    for t in range(T):
        roll = lambda x: torch.roll(x, shifts=shift * t, dims=0)
        frames.append(packed({k: (roll(v) if v.shape[:1] == (N,) else v) for k, v in i.items()}, roll(dof)))
    return {k: torch.stack([f[k] for f in frames])[:, :n].contiguous() for k in frames[0]}


def env_cfg(G, task, getup, episode_length=5):
    cfg = dict(numEnvs=G['num_envs'], episodeLength=episode_length, localRootObs=True, enableEarlyTermination=True, pdControl=True,
               powerScale=1.0, stateInit='Hybrid', hybridInitProb=0.5, numAMPObsSteps=3, contactBodies=['b11', 'b14'],
               terminationHeight=[float(x) for x in G['inputs']['termination_heights']], enableTaskObs=True)
    if task == 'heading':
        cfg.update(tarSpeedMin=1.5, tarSpeedMax=1.6, headingChangeStepsMin=2, headingChangeStepsMax=4, enableRandHeading=True)
    elif task == 'location':
        cfg.update(tarSpeed=1.0, tarChangeStepsMin=2, tarChangeStepsMax=4, tarDistMax=10.0)
    elif task == 'reach':
        cfg.update(tarSpeed=1.0, tarChangeStepsMin=2, tarChangeStepsMax=4, tarDistMax=1.0, tarHeightMin=0.2, tarHeightMax=2.0,
                   reachBodyName='b5')
    elif task == 'strike':
        cfg.update(strikeBodyNames=[f'b{b}' for b in G['strike_body_ids']])
    if getup:
        cfg.update(recoveryEpisodeProb=0.5, recoverySteps=3, fallInitProb=0.2)
    return cfg


def make_env(backend, device, G, clips, A, task, getup, fused, frames=None, pd=True, seed=3, cfg_update=None, n=None):
    """A HumanoidEnv on a PlaybackPhysics of the recording (its first n environments), with initial and fall states set."""
    frames = recording(G, n=n) if frames is None else frames
    g = torch.Generator().manual_seed(5)
    D = 31
    lo = -torch.rand(D, generator=g) - 0.2
    hi = torch.rand(D, generator=g) + 0.2
    ph = PlaybackPhysics(frames, 17, clips['dof_offsets'], lo, hi, torch.rand(D, generator=g) * 100 + 10, BODY_NAMES, dt=G['dt'],
                         device=device)
    dev_clips = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in clips.items()}
    ml = DeviceMotionLib.from_arrays(dev_clips, backend if device != 'cpu' else None, device, generator=torch.Generator(device=device).manual_seed(9))
    cfg = env_cfg(G, task, getup)
    cfg['numEnvs'] = ph.num_envs
    cfg['pdControl'] = pd
    cfg.update(cfg_update or {})
    env = HumanoidEnv(backend, ph, cfg, motion_lib=ml, task=task, getup=getup, fused_step=fused, seed=seed)
    f0 = ph.frames
    env.set_initial_state(f0['root_states'][0, :, 0], f0['dof_state'][0, :, :, 0], f0['dof_state'][0, :, :, 1])
    if getup:
        env.set_fall_states(*[t.to(device) for t in A['tables']['fall']])
    return env


def actions_of(step, n, D):
    """Seeded actions, some beyond the clip."""
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(n, D, generator=g) * 0.8


def run(env, steps, device_resets, device='cpu'):
    """The rollout loop of an agent: reset everything, then step / reset the done rows -> the list of per-step records (clones)."""
    torch.manual_seed(17)                     # the torch draws of the host reset path (amp.reset) use the global generator
    n, D = env.num_envs, env.action_space.shape[0]
    out = []
    obs0 = env.reset()
    for k in range(steps):
        obs, rew, dones, infos = env.step(actions_of(k, n, D).to(device))
        rec = dict(obs=obs.clone(), rewards=rew.clone(), dones=dones.clone(), terminate=infos['terminate'].clone(),
                   amp_obs=infos['amp_obs'].clone(), progress_buf=env.progress_buf.clone(), prev_root_pos=env.prev_root_pos.clone(),
                   targets=env.targets.clone(), actions=env.actions.clone(),
                   recovering=(env.amp.recovery_counter > 0).clone() if env.getup else torch.zeros(n, dtype=torch.bool, device=device))
        if device_resets:
            rec['reset_obs'] = env.reset_done(dones).clone()
        else:
            rec['reset_obs'] = env.reset(dones.nonzero().view(-1)).clone()
        out.append(rec)
    return obs0, out
