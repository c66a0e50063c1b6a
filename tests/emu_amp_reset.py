"""Plain-torch restatement of ``HipBackend.amp_reset`` with the same signature, plus ``build_amp_obs`` so that
``ase_amd.amp_env.HumanoidAMPTensors`` runs on it.  TEST INFRASTRUCTURE ONLY: the CPU stand-in of the host tests and the f64
leg of tests/golden/amp_reset.pt (scripts/make_golden_amp_reset.py).

Written from the contract in include/ase_hip.h, following env/tasks/humanoid_amp.py:141-246,257-275 and
env/tasks/humanoid_amp_getup.py:105-129 of the reference; composed from ``oracle.amp_obs.motion_state`` /
``build_amp_observations``.  It computes in the dtype of ``hist``: with every float operand cast to f64 it is the f64 result the
device tests compare with (the history times are then formed in f64 from the f32 ``motion_times``)."""
import contextlib
import os

import torch

from ase_amd import lib as L
from oracle import amp_obs as A


@contextlib.contextmanager
def _default_dtype(dtype):
    """oracle.amp_obs.motion_state allocates its dof positions in torch's default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _clips(clips, dtype):
    c = dict(clips)
    for k in ('num_frames', 'length_starts'):
        c[k] = clips[k].long()
    for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'dt'):
        c[k] = clips[k].to(dtype)
    return c


class EmuAmpReset:
    name = "emu-amp-reset"
    device = torch.device('cpu')

    def host_call(self, fn):
        fn()

    def build_amp_obs(self, root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, dof_offsets,
                      local_root_obs, root_height_obs, hist, shift=True):
        frame = A.build_amp_observations(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos,
                                         local_root_obs, root_height_obs, dof_offsets)
        if shift:
            A.push_history(hist, frame)
        else:
            hist[:, 0] = frame

    def amp_reset(self, clips, env_ids, kind, motion_ids, motion_times, src_rows, table, root_states, dof_pos, dof_vel, body_pos,
                  body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs, env_dt, hist,
                  kinds=L.RESET_HAS_TABLE | L.RESET_HAS_MOTION):
        n, S, F = hist.shape
        dtype = hist.dtype
        offs, kb = [int(x) for x in clips['dof_offsets']], [int(x) for x in clips['key_body_ids']]
        ids = env_ids.long()
        ok = (ids >= 0) & (ids < n) & (kind >= 0) & (kind <= L.RESET_MOTION)
        if kinds & L.RESET_HAS_TABLE:
            ok &= (kind != L.RESET_TABLE) | ((src_rows >= 0) & (src_rows < table[0].shape[0]))
        else:
            ok &= kind != L.RESET_TABLE
        if not kinds & L.RESET_HAS_MOTION:
            ok &= kind != L.RESET_MOTION
        m1, m2 = ok & (kind == L.RESET_TABLE), ok & (kind == L.RESET_MOTION)
        # ---- _reset_default / _reset_fall_episode: rows of the state table
        if m1.any():
            e, src = ids[m1], src_rows[m1].long()
            root_states[e] = table[0][src]
            dof_pos[e] = table[1][src]
            dof_vel[e] = table[2][src]
        # ---- _reset_ref_state_init + _set_env_state
        if m2.any():
            c = _clips(clips, dtype)
            e, mid, t = ids[m2], motion_ids[m2].long(), motion_times[m2].to(dtype)
            with _default_dtype(dtype):
                rp, rq, dp, rv, rw, dv, _ = A.motion_state(c, mid, t)
            root_states[e, 0:3], root_states[e, 3:7], root_states[e, 7:10], root_states[e, 10:13] = rp, rq, rv, rw
            dof_pos[e] = dp
            dof_vel[e] = dv
        # ---- _compute_amp_observations(env_ids): the current frame from the rigid-body tensors and the fresh dof state
        if ok.any():
            e = ids[ok]
            hist[e, 0] = A.build_amp_observations(body_pos[e][:, 0], body_rot[e][:, 0], body_vel[e][:, 0], body_ang_vel[e][:, 0],
                                                  dof_pos[e], dof_vel[e], body_pos[e][:, kb], local_root_obs, root_height_obs, offs)
        # ---- _init_amp_obs_default
        if m1.any() and S > 1:
            e = ids[m1]
            hist[e, 1:] = hist[e, 0:1]
        # ---- _init_amp_obs_ref: times k steps back, unclamped; f32: t + (float)(-dt) * (float)k
        if m2.any() and S > 1:
            e, mid, t = ids[m2], motion_ids[m2].long(), motion_times[m2].to(dtype)
            steps = torch.tensor(-env_dt, dtype=dtype) * torch.arange(1, S).to(dtype)
            times = (t.unsqueeze(-1) + steps).view(-1)
            mids = mid.unsqueeze(-1).expand(-1, S - 1).reshape(-1)
            with _default_dtype(dtype):
                rp, rq, dp, rv, rw, dv, kp = A.motion_state(c, mids, times)
            frames = A.build_amp_observations(rp, rq, rv, rw, dp, dv, kp, local_root_obs, root_height_obs, offs)
            hist[e, 1:] = frames.view(e.shape[0], S - 1, F)


# ---- the fixture tests/golden/amp_reset.pt (scripts/make_golden_amp_reset.py) ----------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GROUPS = ('root', 'dof_pos', 'frame0', 'hist')


def load_fixture():
    """(fixture, clips): the clips are those of tests/golden/motion_state.pt, read only."""
    G = torch.load(os.path.join(GOLDEN, 'amp_reset.pt'), weights_only=False)
    clips = torch.load(os.path.join(GOLDEN, 'motion_state.pt'), weights_only=False)['clips']
    return G, clips


def hist_pattern(N, S, F):
    """The history before a reset: an arithmetic pattern (exact in every float format), so that untouched rows are detectable."""
    return ((torch.arange(N * S * F) * 7919) % 2003).to(torch.float32).view(N, S, F) / 100.0 - 10.0


def prefill(G, dtype=torch.float32, device='cpu'):
    """The buffers before a scenario's reset: the fixture's seeded state (f64: the f32 values cast up) and the patterned
    history -> (state dict of HumanoidAMPTensors, dict of progress_buf / reset_buf / terminate_buf / recovery_counter)."""
    s = {k: v.clone() for k, v in G['inputs'].items()}
    s['amp_obs_buf'] = hist_pattern(G['num_envs'], G['num_amp_obs_steps'], G['num_amp_obs_per_step'])
    s = {k: v.to(dtype).contiguous().to(device) for k, v in s.items()}
    bufs = {k: v.clone().to(device) for k, v in G['buffers'].items()}
    return s, bufs


def tables(G, dtype=torch.float32, device='cpu'):
    """(initial state, fall states), each (root_states, dof_pos, dof_vel); the fall-state rows are pairwise distinct."""
    cast = lambda ts: tuple(t.to(dtype).contiguous().to(device) for t in ts)
    return cast(G['tables']['init']), cast(G['tables']['fall'])


def plan_of(G, sc, device='cpu'):
    """The reference's recorded draw as the plan of ase_hip_amp_reset (rows in the order of the scenario's env_ids)."""
    P = sc['plan']
    return {'env_ids': torch.tensor(P['env_ids'], dtype=torch.int32, device=device),
            'kind': torch.tensor(P['kind'], dtype=torch.int32, device=device),
            'motion_ids': torch.tensor(P['motion_ids'], dtype=torch.int32, device=device),
            'motion_times': P['motion_times'].to(torch.float32).to(device),
            'src_rows': torch.tensor(P['src_rows'], dtype=torch.int32, device=device)}


def expected_f64(G, clips, sc):
    """The f64 result of a scenario: this file's restatement on the scenario's inputs cast up (the reference's MotionLib
    refuses f64).  -> dict of the state tensors and the history after the reset."""
    s, _ = prefill(G, torch.float64)
    init, fall = tables(G, torch.float64)
    table = tuple(torch.cat([a, b]) for a, b in zip(init, fall))
    p = plan_of(G, sc)
    EmuAmpReset().amp_reset(clips, p['env_ids'], p['kind'], p['motion_ids'], p['motion_times'], p['src_rows'], table,
                            s['humanoid_root_states'], s['dof_pos'], s['dof_vel'], s['rigid_body_pos'], s['rigid_body_rot'],
                            s['rigid_body_vel'], s['rigid_body_ang_vel'], G['local_root_obs'], G['root_height_obs'], G['dt'],
                            s['amp_obs_buf'])
    return s


def group_errors(got, want, rows2, rows_all):
    """max |got - want| per output group: root position + rotation and dof positions of the motion rows (rows2), the slot-0
    frame of every touched row, the history slots 1.. of the motion rows.  got / want: dicts as of prefill()."""
    d = lambda k: (got[k].double().cpu() - want[k].double().cpu()).abs()
    mx = lambda t: float(t.max()) if t.numel() else 0.0
    return {'root': mx(d('humanoid_root_states')[rows2, 0:7]), 'dof_pos': mx(d('dof_pos')[rows2]),
            'frame0': mx(d('amp_obs_buf')[rows_all, 0]), 'hist': mx(d('amp_obs_buf')[rows2, 1:])}


def allowance(G, group):
    """The bar of the device tests: max |x - f64| <= 2 e_ref + 1e-7, e_ref = what the reference's own f32 run loses against
    the f64 result (stored by the generator per output group)."""
    return 2.0 * G['e_ref'][group] + 1e-7
