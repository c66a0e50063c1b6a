"""Golden vectors of the view-motion task, recorded from the reference's own unmodified
``compute_view_motion_reset`` and the method bodies ``HumanoidViewMotion._motion_sync`` / ``_compute_reset`` /
``_reset_env_tensors`` with the reference's ``MotionLib``.  TEST INFRASTRUCTURE ONLY (needs the reference tree; isaacgym comes
from the restatement in oracle/rl_games_shim).

    python scripts/make_golden_view_motion.py      # writes tests/golden/view_motion.pt (tensors, plain lists and numbers only)

Neither class can be constructed without Isaac Gym and clip files, but the methods run on bare instances (``object.__new__``)
that carry the attributes they read: the ``MotionLib`` gets the clip tensors of tests/ref_view_motion.py ``library`` (two-,
three- and four-frame synthetic clips and 24 frames of a shipped clip), the task a stub ``gym`` that counts the two indexed set
calls.

What the file carries:
  clips       the five-clip library; a case with num_motions = m uses its first m clips.
  cases       n_envs 1, 3, 70 x num_motions 1, 2, 5 x motion_dt 1/30 (controlFrequencyInv 2) and 1/60, in rounds: every
              environment meets the counters 0, 1, mid-clip and the two integers on either side of length / motion_dt.  Per
              round: motion_ids, progress, the reference's motion_times (so the f32 product is pinned, not assumed), reset,
              terminate (int64 vectors, stored as lists), the humanoid's root rows and dof positions after _motion_sync (the dof velocities are asserted here
              to be +0.0 and not stored), and motion_ids / progress after _reset_env_tensors on reset.nonzero().
  e_ref       per round and group max |reference f32 - f64 restatement|: the device tests allow 2 e_ref + 2^-23 max |ref| +
              1e-7.  Asserted here to be at most 64 * 2^-24 * max(|group|, 1) (rotations and dof positions: 1e-4, slerp's acos of close frames).
The f32 restatement tests/ref_view_motion.py ``sync`` is asserted here to be bitwise the reference.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'rl_games_shim'))
sys.path.insert(0, REFERENCE)

from env.tasks import humanoid_view_motion as HV              # noqa: E402  (reference code)
from utils.motion_lib import MotionLib                        # noqa: E402  (reference code)

from tests import ref_view_motion as RV                       # noqa: E402

ACTORS = 3                                                    # the humanoid and two other actors in the packed root tensor
ROUNDINGS = 64


class _Gym:
    def __init__(self):
        self.sets = []

    def set_actor_root_state_tensor_indexed(self, sim, states, ids, n):
        self.sets.append(('root', n))

    def set_dof_state_tensor_indexed(self, sim, states, ids, n):
        self.sets.append(('dof', n))


class _Motion:
    num_joints = RV.BODIES


def bare_lib(clips):
    ml = object.__new__(MotionLib)
    ml._dof_body_ids, ml._dof_offsets, ml._num_dof = clips['dof_body_ids'], clips['dof_offsets'], clips['dof_offsets'][-1]
    ml._key_body_ids, ml._device = torch.tensor(clips['key_body_ids']), 'cpu'
    m = clips['lengths'].numel()
    ml._motions = [_Motion()] * m
    for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs'):
        setattr(ml, k, clips[k])
    ml._motion_lengths, ml._motion_dt = clips['lengths'], clips['dt']
    ml._motion_num_frames, ml.length_starts = clips['num_frames'].long(), clips['length_starts'].long()
    return ml


def bare_task(clips, n, motion_dt, motion_ids, progress):
    o = object.__new__(HV.HumanoidViewMotion)
    D = clips['dof_offsets'][-1]
    o._motion_lib, o._motion_dt, o.num_envs, o.device = bare_lib(clips), motion_dt, n, 'cpu'
    o._motion_ids, o.progress_buf = motion_ids.clone(), progress.clone()
    o.reset_buf, o._terminate_buf = torch.full((n,), 7, dtype=torch.int64), torch.full((n,), 7, dtype=torch.int64)
    o._root_states = torch.full((n * ACTORS, 13), 3.0)
    o._humanoid_root_states = o._root_states.view(n, ACTORS, 13)[:, 0]
    o._dof_state = torch.full((n * D, 2), 3.0)
    o._dof_pos, o._dof_vel = o._dof_state.view(n, D, 2)[..., 0], o._dof_state.view(n, D, 2)[..., 1]
    o._humanoid_actor_ids = ACTORS * torch.arange(n, dtype=torch.int32)
    o.gym, o.sim = _Gym(), None
    return o


def build():
    lib = RV.library()
    G = {'clips': lib, 'actors': ACTORS, 'roundings': ROUNDINGS, 'cases': {}}
    for n in RV.N_ENVS:
        for m in RV.NUM_MOTIONS:
            clips = RV.sub_library(lib, m)
            for cfi, sim_dt in RV.MOTION_DTS:
                motion_dt = cfi * sim_dt                                   # humanoid_view_motion.py:10-11
                for r in range(RV.case_rounds(n)):
                    ids, progress = RV.case_inputs(clips, n, m, motion_dt, r)
                    o = bare_task(clips, n, motion_dt, ids, progress)
                    HV.HumanoidViewMotion._compute_reset(o)
                    HV.HumanoidViewMotion._motion_sync(o)
                    assert o.gym.sets == [('root', n), ('dof', n)]
                    times = o.progress_buf * o._motion_dt                  # the statement of line 47
                    assert times.dtype == torch.float32
                    zero = torch.zeros(1).view(torch.int32)
                    assert bool((o._dof_vel.contiguous().view(torch.int32) == zero).all()), 'dof velocities are +0.0'
                    assert bool((o._humanoid_root_states[:, 7:13].contiguous().view(torch.int32) == zero).all())
                    assert bool((o._root_states.view(n, ACTORS, 13)[:, 1:] == 3.0).all()), 'the other actors are untouched'
                    rec = {'n': n, 'm': m, 'cfi': cfi, 'sim_dt': sim_dt, 'motion_dt': motion_dt, 'motion_ids': ids, 'progress': progress,
                           'motion_times': times.clone(), 'reset': o.reset_buf.clone(), 'terminate': o._terminate_buf.clone(),
                           'root': o._humanoid_root_states.clone(), 'dof_pos': o._dof_pos.clone()}
                    env_ids = o.reset_buf.nonzero().view(-1)
                    before = o._root_states.clone(), o._dof_state.clone()
                    HV.HumanoidViewMotion._reset_env_tensors(o, env_ids)
                    assert torch.equal(o._root_states, before[0]) and torch.equal(o._dof_state, before[1]), 'a reset writes no state'
                    rec.update(motion_ids_after=o._motion_ids.clone(), progress_after=o.progress_buf.clone(),
                               reset_after=o.reset_buf.clone(), terminate_after=o._terminate_buf.clone())
                    # the restatement: f32 bit for bit, f64 the yardstick
                    s32, s64 = (RV.sync(clips, ids, progress, motion_dt, dt) for dt in (torch.float32, torch.float64))
                    for k in ('reset', 'terminate', 'root', 'dof_pos'):
                        assert torch.equal(s32[k], rec[k]), f'{RV.case_name(n, m, cfi, r)}: the f32 restatement of {k} is not the reference'
                    assert torch.equal(s32['t'], rec['motion_times'])
                    ids2, p2, r2, t2 = ids.clone(), progress.clone(), rec['reset'].clone(), rec['terminate'].clone()
                    RV.advance(ids2, p2, r2, t2, m)
                    assert torch.equal(ids2, rec['motion_ids_after']) and torch.equal(p2, rec['progress_after'])
                    assert not bool(r2.any()) and not bool(rec['reset_after'].any()) and not bool(rec['terminate_after'].any())
                    rec['e_ref'] = {}
                    for g, (k, cols) in RV.GROUPS.items():
                        e = float((rec[k][:, cols].double() - s64[k][:, cols]).abs().max())
                        cap = ROUNDINGS * 2.0 ** -24 * max(float(rec[k][:, cols].abs().max()), 1.0)
                        if g in ('root_rot', 'dof_pos'):
                            # frames 0.02 .. 0.04 rad apart: slerp's acos(c) at 1 - c ~ 4e-4 keeps eps / (1 - c) ~ 1.5e-4 of its
                            # value in f32, and the angle-axis map doubles what is left of it in the blended quaternion
                            cap = 1e-4
                        assert e <= cap, f'{RV.case_name(n, m, cfi, r)} {g}: the reference itself loses {e:.3g} in f32 (cap {cap:.3g})'
                        rec['e_ref'][g] = e
                    del rec['reset_after'], rec['terminate_after']           # (asserted above to be zero)
                    # the integer vectors as plain lists: a tensor costs a few hundred bytes of container each
                    G['cases'][RV.case_name(n, m, cfi, r)] = {k: (v.tolist() if torch.is_tensor(v) and v.dtype == torch.int64 else v)
                                                              for k, v in rec.items()}
    kinds = sum(sum(c['reset']) for c in G['cases'].values()), sum(len(c['reset']) - sum(c['reset']) for c in G['cases'].values())
    print(len(G['cases']), 'rounds;', kinds[0], 'rows past their clip,', kinds[1], 'inside it')
    assert kinds[0] > 0 and kinds[1] > 0
    return G


def main():
    G = build()
    path = os.path.join(ROOT, 'tests', 'golden', 'view_motion.pt')
    torch.save(G, path)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 256 * 1024


if __name__ == '__main__':
    main()
