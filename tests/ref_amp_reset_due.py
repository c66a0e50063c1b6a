"""The draws of ``ase_hip_amp_reset_due`` stated in numpy, from the draw table in include/ase_hip.h, on the stream
of tests/ref_rollout.py - and with them the CPU stand-in of ``HipBackend.amp_reset_due``.  TEST INFRASTRUCTURE ONLY.

Draw j of environment e is element ``8 e + j`` of the Philox stream at (seed, offset): j = 0 the recovery uniform, 1 the fall
uniform, 2 word 0 for the fall row (multiply-shift), 3 the Hybrid uniform, 4 the 24-bit integer behind the uniform for the clip
(``searchsorted(cdf, v, side='right')``), 5 the uniform of the motion time (one f32 product with the clip's length)."""
import numpy as np
import torch

from ase_amd import lib as L
from tests import ref_rollout as RR
from tests.emu_amp_reset import EmuAmpReset

PLAN_KEYS = ('env_ids', 'kind', 'motion_ids', 'motion_times', 'src_rows')
SEED = (1 << 33) + 3         # above 2^32; with the fixture's options it reaches every branch at offsets 0 and 5 (the tests assert it)


def reset_pattern(n):
    """A reset_buf with two rows in three due, the due rows holding different non-zero values (the test is != 0)."""
    e = torch.arange(n)
    return torch.where(e % 3 != 1, torch.tensor([1, 2, -1, 7])[e % 4], 0).to(torch.int64)


def block_pattern(n, rows_per_block):
    """A reset_buf by blocks of the launch, in turn: no row due, only the last row, every row, only the first row."""
    e = torch.arange(n)
    b, r = e // rows_per_block, e % rows_per_block
    last = torch.minimum((b + 1) * rows_per_block, torch.tensor(n)) - 1 - b * rows_per_block
    mode = b % 4
    return ((mode == 2) | ((mode == 1) & (r == last)) | ((mode == 3) & (r == 0))).to(torch.int64)


def draws(seed, offset, n_envs):
    """Every environment's six draws -> dict of [n_envs] arrays: u0, u1, u3, u5 f32 uniforms, word2 uint32, v4 uint32 (24 bits)."""
    e8 = np.uint64(8) * np.arange(n_envs, dtype=np.uint64)
    w = [RR.philox4x32_10(e8 + np.uint64(j), offset, seed) for j in range(6)]
    return {'u0': RR.keep_uniform(w[0][2]), 'u1': RR.keep_uniform(w[1][2]), 'word2': w[2][0], 'u3': RR.keep_uniform(w[3][2]),
            'v4': w[4][2] >> np.uint32(8), 'u5': RR.keep_uniform(w[5][2])}


def ref_plan(seed, offset, reset_buf, terminate_buf, cfg, cdf, lengths, n_fall):
    """The full-length plan of one launch -> dict of numpy arrays [n_envs] (PLAN_KEYS; int32, motion_times f32).
    cfg: dict(state_init='Default' | 'Start' | 'Random' | 'Hybrid', hybrid_init_prob, getup=None | (recovery_episode_prob,
    recovery_steps, fall_init_prob)); cdf / lengths: the clip table and the f32 clip lengths (unused for 'Default');
    n_fall: the fall rows behind the n_envs initial rows of the state table."""
    reset = np.asarray(reset_buf).astype(np.int64)
    N = reset.shape[0]
    d = draws(seed, offset, N)
    e = np.arange(N)
    due = reset != 0
    recovery = np.zeros(N, dtype=bool)
    fall = np.zeros(N, dtype=bool)
    if cfg.get('getup') is not None:
        p_rec, _, p_fall = cfg['getup']
        recovery = (d['u0'] < np.float32(p_rec)) & (np.asarray(terminate_buf).astype(np.int64) == 1)
        fall = ~recovery & (d['u1'] < np.float32(p_fall))
    rest = ~recovery & ~fall
    init = cfg['state_init']
    if init == 'Default':
        motion = np.zeros(N, dtype=bool)
    elif init == 'Hybrid':
        motion = rest & (d['u3'] < np.float32(cfg['hybrid_init_prob']))
    else:
        motion = rest.copy()
    default = rest & ~motion
    kind = np.where(recovery, L.RESET_FRAME, np.where(motion, L.RESET_MOTION, L.RESET_TABLE))
    fall_rows = N + ((d['word2'].astype(np.uint64) * np.uint64(n_fall)) >> np.uint64(32)).astype(np.int64)
    src = np.where(fall, fall_rows, np.where(default, e, 0))
    mid = np.zeros(N, dtype=np.int64)
    t = np.zeros(N, dtype=np.float32)
    if init != 'Default':
        clip = np.searchsorted(np.asarray(cdf).astype(np.int64), d['v4'].astype(np.int64), side='right')
        mid = np.where(motion, clip, 0)
        if init != 'Start':
            t = np.where(motion, d['u5'] * np.asarray(lengths, dtype=np.float32)[np.minimum(clip, len(lengths) - 1)], np.float32(0))
    z = lambda a, dt: np.where(due, a, 0).astype(dt)
    return {'env_ids': np.where(due, e, -1).astype(np.int32), 'kind': z(kind, np.int32), 'motion_ids': z(mid, np.int32),
            'motion_times': z(t, np.float32), 'src_rows': z(src, np.int32)}


def plan_tensors(plan, device='cpu'):
    return {k: torch.from_numpy(np.ascontiguousarray(plan[k])).to(device) for k in PLAN_KEYS}


def due_rows(plan):
    """The plan of ``apply_reset`` that holds the due rows only."""
    keep = plan['env_ids'] >= 0
    return {k: v[keep].contiguous() for k, v in plan.items()}


def bookkeeping(plan, n_envs, progress_buf, reset_buf, terminate_buf, recovery_counter, getup):
    """``_reset_env_tensors`` and the recovery counter for the rows of a (torch) plan whose env_ids are not -1."""
    keep = plan['env_ids'] >= 0
    ids = plan['env_ids'][keep].long()
    for buf in (progress_buf, reset_buf, terminate_buf):
        if buf is not None:
            buf[ids] = 0
    if getup is not None:
        kind, src = plan['kind'][keep], plan['src_rows'][keep]
        counted = (kind == L.RESET_FRAME) | ((kind == L.RESET_TABLE) & (src >= n_envs))
        recovery_counter[ids] = torch.where(counted, int(getup[1]), 0).to(torch.int32)


class EmuAmpResetDue(EmuAmpReset):
    """``HipBackend.amp_reset_due`` on the CPU: the reference plan, ``EmuAmpReset.amp_reset`` on it, the book-keeping."""
    name = "emu-amp-reset-due"

    def amp_reset_due(self, clips, clip_cdf, table, state_init, hybrid_init_prob, getup, rng_state, progress_buf, reset_buf,
                      terminate_buf, recovery_counter, plan, root_states, dof_pos, dof_vel, body_pos, body_rot, body_vel,
                      body_ang_vel, local_root_obs, root_height_obs, env_dt, hist, advance=True):
        n = hist.shape[0]
        cfg = dict(state_init=('Default', 'Start', 'Random', 'Hybrid')[state_init], hybrid_init_prob=hybrid_init_prob, getup=getup)
        motion = state_init != L.INIT_DEFAULT
        P = ref_plan(int(rng_state[0]), int(rng_state[1]), reset_buf.numpy(), None if terminate_buf is None else terminate_buf.numpy(),
                     cfg, clip_cdf.numpy() if motion else None, clips['lengths'].numpy() if motion else None,
                     0 if table is None else table[0].shape[0] - n)
        P = plan_tensors(P)
        kinds = (L.RESET_HAS_MOTION if motion else 0) | (L.RESET_HAS_TABLE if table is not None else 0)
        self.amp_reset(clips, P['env_ids'], P['kind'], P['motion_ids'], P['motion_times'], P['src_rows'], table, root_states, dof_pos,
                       dof_vel, body_pos, body_rot, body_vel, body_ang_vel, local_root_obs, root_height_obs, env_dt, hist, kinds)
        bookkeeping(P, n, progress_buf, reset_buf, terminate_buf, recovery_counter, getup)
        if plan is not None:
            for k in PLAN_KEYS:
                plan[k].copy_(P[k])
        if advance:
            rng_state[1] += 1
