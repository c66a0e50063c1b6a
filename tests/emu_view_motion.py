"""Plain-torch restatement of ``HipBackend.motion_sync`` with the same signature, composed from the host
statement tests/ref_view_motion.py (which restates the sampler through tests/ref_amp_obs.py), and the helpers that put a
``ViewMotionEnv`` on a ``ClipPhysics``.  TEST INFRASTRUCTURE ONLY: the CPU stand-in for the backend in the host tests.

The arithmetic runs in the dtype of root_states: f32 repeats the reference's operations, f64 is the yardstick on the same f32
times.  ``wrong`` selects a single-term wrong restatement, for the tests that show the checks can fail."""
import torch

from ase_amd import lib as L
from tests import ref_amp_obs as R
from tests import ref_view_motion as RV
from tests.emu_env_step import EmuEnvStep

WRONG = ('>=', '+1', 'velocities', 'pre-increment', 'state on reset', 'dof_vel stride')
BODY_NAMES = [f'b{i}' for i in range(RV.BODIES)]


class EmuMotionSync:
    name = "emu-motion-sync"
    device = torch.device('cpu')
    wrong = None

    def motion_state(self, clips, motion_ids, times):
        out, _ = R.get_motion_state(clips, motion_ids, times, torch.float32)
        return tuple(out[k] for k in R.OUT_NAMES)

    def motion_sync(self, clips, motion_ids, progress_buf, reset_buf, terminate_buf, mode=L.MOTION_SYNC, motion_dt=0.0,
                    root_states=None, dof_pos=None, dof_vel=None, body_pos=None, body_rot=None, body_vel=None, body_ang_vel=None,
                    env_ids=None, ids_out=None):
        M, n = clips['lengths'].numel(), motion_ids.numel()
        assert motion_ids.dtype == torch.int32 and all(t.dtype == torch.int64 for t in (progress_buf, reset_buf, terminate_buf))
        state = dict(root_states=root_states, dof_pos=dof_pos, dof_vel=dof_vel, body_pos=body_pos, body_rot=body_rot, body_vel=body_vel,
                     body_ang_vel=body_ang_vel)
        if mode == L.MOTION_RESET:
            assert all(v is None for v in state.values()), 'RESET takes no state operand'
            assert env_ids is None or ids_out is None
            if env_ids is not None and env_ids.numel() == 0:
                return
            ids64 = motion_ids.long()
            done = RV.advance(ids64, progress_buf, reset_buf, terminate_buf, M, env_ids, wrong=self.wrong)
            motion_ids.copy_(ids64)
            if ids_out is not None:
                ids_out.copy_(done)
            if self.wrong == 'state on reset' and bool((done >= 0).any()):       # the base class's indexed set, which the override omits
                self._write(clips, motion_ids, progress_buf, self._last_dt, (done >= 0).nonzero().view(-1), self._last_state)
            return
        assert mode == L.MOTION_SYNC and env_ids is None and ids_out is None
        assert root_states is not None and dof_pos is not None and dof_vel is not None
        rows = ((motion_ids >= 0) & (motion_ids < M)).nonzero().view(-1)
        self._last_state, self._last_dt = state, motion_dt
        if rows.numel() == 0:
            return
        s = self._write(clips, motion_ids, progress_buf, motion_dt, rows, state)
        reset_buf[rows] = s['reset']
        terminate_buf[rows] = 0

    def _write(self, clips, motion_ids, progress_buf, motion_dt, rows, state):
        dt = state['root_states'].dtype
        s = RV.sync(clips, motion_ids[rows], progress_buf[rows], motion_dt, dt, wrong=self.wrong)
        state['root_states'][rows] = s['root']
        state['dof_pos'][rows] = s['dof_pos']
        dv = state['dof_vel']
        if self.wrong == 'dof_vel stride' and dv.stride(1) != 1:                 # dof d at [d], not at [d * element stride]
            dv = torch.as_strided(dv, dv.shape, (dv.stride(0), 1), dv.storage_offset())
        dv[rows] = s['dof_vel']
        for k in ('body_pos', 'body_rot'):
            if state[k] is not None:
                state[k][rows] = s[k]
        for k in ('body_vel', 'body_ang_vel'):
            if state[k] is not None:
                state[k][rows] = 0.0
        return s


class EmuEnvViewMotion(EmuEnvStep, EmuMotionSync):
    """The environment stand-in with the view-motion launch: what ``ViewMotionEnv`` runs on without a GPU."""
    name = "emu-env-view-motion"


def env_cfg(n, episode_length=300, cfi=2, steps=3):
    return dict(numEnvs=n, episodeLength=episode_length, localRootObs=True, enableEarlyTermination=True, pdControl=True, powerScale=1.0,
                stateInit='Random', numAMPObsSteps=steps, contactBodies=['b11', 'b14'], terminationHeight=0.15,
                keyBodies=[f'b{b}' for b in RV.KEY_BODY_IDS], controlFrequencyInv=cfi)


def make_env(backend, device, clips, n, fused, cfi=2, sim_dt=1.0 / 60.0, others=2, **cfg_kw):
    """A ViewMotionEnv on a ClipPhysics with `others` actors beside the humanoid."""
    from ase_amd.motion_lib import DeviceMotionLib
    from ase_amd.view_motion import ClipPhysics, ViewMotionEnv
    g = torch.Generator().manual_seed(5)
    D = clips['dof_offsets'][-1]
    lo, hi = -torch.rand(D, generator=g) - 0.2, torch.rand(D, generator=g) + 0.2
    ph = ClipPhysics(n, clips['gts'].shape[1], clips['dof_offsets'], lo, hi, BODY_NAMES, dt=sim_dt, device=device, num_other_actors=others)
    dev_clips = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in clips.items()}
    ml = DeviceMotionLib.from_arrays(dev_clips, backend if device != 'cpu' else None, device,
                                     generator=torch.Generator(device=device).manual_seed(9))
    return ViewMotionEnv(backend, ph, env_cfg(n, cfi=cfi, **cfg_kw), ml, fused=fused)


def run_env(env, steps, device='cpu', device_resets=True):
    """Reset everything, then step / reset the done rows the way an agent's rollout loop does -> per-step records (clones)."""
    from tests import env_step_cases as CS
    n, D = env.num_envs, env.action_space.shape[0]
    env.reset()
    out = []
    for k in range(steps):
        ids, t = env.motion_ids.clone(), (env.progress_buf + 1) * env.motion_dt
        obs, rew, dones, infos = env.step(CS.actions_of(k, n, D).to(device))
        ph = env.physics
        rec = dict(obs=obs.clone(), rewards=rew.clone(), dones=dones.clone(), terminate=infos['terminate'].clone(),
                   amp_obs=infos['amp_obs'].clone(), progress_buf=env.progress_buf.clone(), sync_ids=ids, sync_t=t,
                   root_states=ph.root_states.clone(), dof_state=ph.dof_state.clone(), rigid_body_state=ph.rigid_body_state.clone(),
                   actions=env.actions.clone(), targets=env.targets.clone())
        rec['reset_obs'] = (env.reset_done(dones) if device_resets else env.reset(dones.nonzero().view(-1))).clone()
        rec['motion_ids'] = env.motion_ids.clone()
        rec['reset_ids'] = env.reset_ids.clone()
        out.append(rec)
    return out


def expected_frame(be, clips, ids, t, key_body_ids, F):
    """The AMP frame of the pose the sync launch wrote at (ids, t), by entries that existed before it: ``motion_state`` with every
    body as a key body, the velocities zeroed, then ``build_amp_obs`` on the key bodies' rows -> [n, F]."""
    B = clips['gts'].shape[1]
    rp, rq, dp, rv, rw, dv, kp = be.motion_state(dict(clips, key_body_ids=list(range(B))), ids, t)
    hist = torch.zeros(ids.numel(), 1, F, dtype=torch.float32, device=rp.device)
    be.build_amp_obs(rp, rq, torch.zeros_like(rv), torch.zeros_like(rw), dp, torch.zeros_like(dv), kp[:, list(key_body_ids)].contiguous(),
                     clips['dof_offsets'], True, True, hist, shift=False)
    return hist[:, 0]


# ---- one launch on windows of NaN-filled allocations with wider pitches -------------------------------------------------------------
NAN = float('nan')
ISENT = -77


class Case:
    """The operands of ``motion_sync`` as windows: the humanoid's row inside [n + 2, actors, 16] (NaN pitch columns, NaN actors
    beside it), the interleaved dof state [n + 2, D + 1, 2] or two padded [n + 2, D + 3] tensors, bodies inside [n + 2, B + 1,
    w + 2]; the integer buffers inside [n + 2] with sentinel words.  dtype f64: the yardstick run of the stand-in."""

    def __init__(self, clips, n, dev='cpu', actors=3, interleaved=True, bodies=True, dtype=torch.float32):
        self.clips, self.n, self.dev = clips, n, dev
        B, D = clips['gts'].shape[1], clips['dof_offsets'][-1]
        self.B, self.D = B, D
        f = lambda *shape: torch.full(shape, NAN, dtype=dtype, device=dev)
        self.root_whole = f(n + 2, actors, 16)
        self.root = self.root_whole[1:n + 1, 0, :13]
        if interleaved:
            self.dof_whole = [f(n + 2, D + 1, 2)]
            self.dof_pos, self.dof_vel = self.dof_whole[0][1:n + 1, :D, 0], self.dof_whole[0][1:n + 1, :D, 1]
        else:
            self.dof_whole = [f(n + 2, D + 3), f(n + 2, D + 3)]
            self.dof_pos, self.dof_vel = (w[1:n + 1, :D] for w in self.dof_whole)
        self.body_whole, self.body = {}, {}
        if bodies:
            for k, w in (('body_pos', 3), ('body_rot', 4), ('body_vel', 3), ('body_ang_vel', 3)):
                self.body_whole[k] = f(n + 2, B + 1, w + 2)
                self.body[k] = self.body_whole[k][1:n + 1, :B, :w]
        i = lambda dt: torch.full((n + 2,), ISENT, dtype=dt, device=dev)
        self.int_whole = {'motion_ids': i(torch.int32), 'progress': i(torch.int64), 'reset': i(torch.int64), 'terminate': i(torch.int64),
                          'ids_out': i(torch.int32)}
        self.motion_ids, self.progress, self.reset, self.terminate, self.ids_out = (self.int_whole[k][1:n + 1] for k in self.int_whole)

    def set(self, motion_ids, progress, reset=7, terminate=7):
        self.motion_ids.copy_(torch.as_tensor(motion_ids).to(torch.int32))
        self.progress.copy_(torch.as_tensor(progress))
        self.reset.fill_(reset) if isinstance(reset, int) else self.reset.copy_(torch.as_tensor(reset))
        self.terminate.fill_(terminate) if isinstance(terminate, int) else self.terminate.copy_(torch.as_tensor(terminate))

    def wholes(self):
        return [self.root_whole] + self.dof_whole + list(self.body_whole.values()) + list(self.int_whole.values())

    def snapshot(self):
        return [w.cpu().clone() for w in self.wholes()]

    def sync(self, be, motion_dt):
        be.motion_sync(self.clips, self.motion_ids, self.progress, self.reset, self.terminate, L.MOTION_SYNC, motion_dt, self.root,
                       self.dof_pos, self.dof_vel, **self.body)

    def advance(self, be, env_ids=None, export=True):
        be.motion_sync(self.clips, self.motion_ids, self.progress, self.reset, self.terminate, L.MOTION_RESET, env_ids=env_ids,
                       ids_out=self.ids_out if export and env_ids is None else None)

    def sentinels_ok(self, rows=None):
        """Every element outside the windows is what it was filled with; with rows, the windows' other rows are too."""
        n = self.n
        ok = True
        masks = [(self.root_whole, self.root)] + list(zip(self.dof_whole, (self.dof_pos, self.dof_vel))) \
            + [(self.body_whole[k], self.body[k]) for k in self.body]
        if len(self.dof_whole) == 1:
            masks[1:3] = [(self.dof_whole[0], self.dof_whole[0][1:n + 1, :self.D])]
        for whole, win in masks:
            m = torch.zeros(whole.shape, dtype=torch.bool, device=whole.device)
            view = torch.as_strided(m, win.shape, win.stride(), win.storage_offset())
            if rows is None:
                view.fill_(True)
            else:
                view[rows] = True
            ok = ok and bool(torch.isnan(whole[~m]).all())
        for w in self.int_whole.values():
            ok = ok and int(w[0]) == ISENT and int(w[n + 1]) == ISENT
        return ok
