"""The view-motion task restated on the host, on the sampler restatement of tests/ref_amp_obs.py (the f64
reference tests/test_gpu_amp_obs.py uses): ``sync`` is ``compute_view_motion_reset`` + ``_motion_sync`` of the reference's
env/tasks/humanoid_view_motion.py, ``advance`` is ``_reset_env_tensors``.  In f32 ``sync`` must be bitwise the recording
tests/golden/view_motion.pt (scripts/make_golden_view_motion.py); in f64, on the same f32 times cast up, it is the yardstick of
the device tests.  Also the fixture's clip library and case table, shared by the generator and the tests.  TEST INFRASTRUCTURE
ONLY."""
import os

import torch

from tests import ref_amp_obs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DOF_BODY_IDS = [1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16]            # env/tasks/humanoid.py:191-192
DOF_OFFSETS = [0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31]
KEY_BODY_IDS = [5, 10, 13, 16, 6, 9]
BODIES = 17
N_ENVS = (1, 3, 70)
NUM_MOTIONS = (1, 2, 5)
MOTION_DTS = ((2, 1.0 / 60.0), (1, 1.0 / 60.0))         # (controlFrequencyInv, sim dt): motion_dt 1/30 and 1/60
# the library: (frames, fps); None: the shipped clip 0 of tests/golden/motion_state.pt cut to SHIPPED_FRAMES
LIB = ((2, 30), (3, 60), None, (2, 60), (4, 30))
SHIPPED_FRAMES = 24
KINDS = ('zero', 'one', 'mid', 'end_lo', 'end_hi')      # progress values: 0, 1, mid-clip, the integers around length / motion_dt
GROUPS = {'root_pos': ('root', slice(0, 3)), 'root_rot': ('root', slice(3, 7)), 'dof_pos': ('dof_pos', slice(None))}


def library():
    """Five clips of the humanoid's skeleton: two-, three- and four-frame synthetic clips and 24 frames of a shipped one."""
    shipped = torch.load(os.path.join(GOLDEN, 'motion_state.pt'), weights_only=False)['clips']
    g = R._gen(41)
    B, D = BODIES, DOF_OFFSETS[-1]
    hinge_bodies = {DOF_BODY_IDS[j] for j in range(len(DOF_BODY_IDS)) if DOF_OFFSETS[j + 1] - DOF_OFFSETS[j] == 1}
    parts = {k: [] for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs')}
    nfs, fps = [], []
    for spec in LIB:
        if spec is None:
            s0 = int(shipped['length_starts'][0])
            assert int(shipped['num_frames'][0]) >= SHIPPED_FRAMES and shipped['gts'].shape[1] == B
            for k in parts:
                parts[k].append(shipped[k][s0:s0 + SHIPPED_FRAMES].double())
            nfs.append(SHIPPED_FRAMES)
            fps.append(round(1.0 / float(shipped['dt'][0])))
            continue
        nf, f = spec
        k = torch.arange(nf, dtype=torch.float64).view(nf, 1, 1)
        parts['gts'].append(torch.randn(1, B, 3, generator=g, dtype=torch.float64) + 0.05 * k * torch.randn(1, B, 3, generator=g, dtype=torch.float64))
        parts['lrs'].append(torch.stack([R._pattern('generic', nf, b in hinge_bodies, g) for b in range(B)], 1))
        parts['grs'].append(torch.stack([R._pattern('generic', nf, False, g) for _ in range(B)], 1))
        parts['grvs'].append(torch.randn(nf, 3, generator=g, dtype=torch.float64))
        parts['gravs'].append(torch.randn(nf, 3, generator=g, dtype=torch.float64))
        parts['dvs'].append(torch.randn(nf, D, generator=g, dtype=torch.float64))
        nfs.append(nf)
        fps.append(f)
    clips = {k: torch.cat(v).float() for k, v in parts.items()}
    nf_t = torch.tensor(nfs)
    clips['num_frames'] = nf_t.to(torch.int32)
    clips['length_starts'] = (torch.cumsum(nf_t, 0) - nf_t).to(torch.int32)
    clips['dt'] = torch.tensor([1.0 / f for f in fps], dtype=torch.float64).float()                       # motion_lib.py:194-196
    clips['lengths'] = torch.tensor([1.0 / f * (nf - 1) for nf, f in zip(nfs, fps)], dtype=torch.float64).float()
    clips.update(dof_body_ids=list(DOF_BODY_IDS), dof_offsets=list(DOF_OFFSETS), key_body_ids=list(KEY_BODY_IDS))
    return clips


def sub_library(clips, m):
    """The library of the first m clips."""
    frames = int(clips['num_frames'][:m].sum())
    out = {k: clips[k][:frames] for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs')}
    out.update({k: clips[k][:m] for k in ('num_frames', 'length_starts', 'dt', 'lengths')})
    out.update({k: clips[k] for k in ('dof_body_ids', 'dof_offsets', 'key_body_ids')})
    return out


def progress_values(length, motion_dt):
    """The five counters of a clip: 0, 1, mid-clip and the two integers on either side of length / motion_dt, decided by the
    f32 product itself - lo is the last counter whose time does not exceed the length, hi = lo + 1 the first that does."""
    mdt = torch.tensor(motion_dt, dtype=torch.float64).float()
    lo = int(float(length) / motion_dt)
    while float(torch.tensor(float(lo + 1)) * mdt) <= float(length):
        lo += 1
    while lo > 0 and float(torch.tensor(float(lo)) * mdt) > float(length):
        lo -= 1
    return [0, 1, max(lo // 2, 0), lo, lo + 1]


def case_rounds(n):
    return 1 if n >= 25 else len(KINDS)


def case_inputs(clips, n, m, motion_dt, r):
    """Round r of the case (n environments, the first m clips): motion ids as the class starts them, counters by kind."""
    ids = torch.arange(n, dtype=torch.int64) % m
    vals = [progress_values(clips['lengths'][i], motion_dt) for i in range(m)]
    progress = torch.tensor([vals[int(ids[e])][(e // m + r) % len(KINDS)] for e in range(n)], dtype=torch.int64)
    return ids, progress


def case_name(n, m, cfi, r):
    return f'n{n}_m{m}_cfi{cfi}_r{r}'


def sync(clips, motion_ids, progress, motion_dt, dtype, wrong=None):
    """compute_view_motion_reset + _motion_sync in dtype on the f32 times, plus every body by the sampler's two expressions ->
    dict(t f32, reset, terminate int64 [n], root [n, 13], dof_pos, dof_vel [n, D], body_pos [n, B, 3], body_rot [n, B, 4])."""
    ids = motion_ids.long()
    t32 = (progress - 1 if wrong == 'pre-increment' else progress) * motion_dt           # f32: int64 tensor * Python float
    assert t32.dtype == torch.float32
    lengths = clips['lengths'][ids]
    reset = (t32 >= lengths if wrong == '>=' else t32 > lengths).long()
    B = clips['gts'].shape[1]
    every = dict(clips, key_body_ids=list(range(B)))
    out, dec = R.get_motion_state(every, ids, t32, dtype)
    c = {k: clips[k].to(dtype) for k in ('grs', 'lengths', 'dt')}
    blend = R.calc_frame_blend(t32.to(dtype), c['lengths'][ids], clips['num_frames'].long()[ids], c['dt'][ids])[2]
    body_rot, _ = R.slerp(c['grs'][dec['f0']], c['grs'][dec['f1']], blend.view(-1, 1, 1))
    n = ids.numel()
    vel = torch.cat([out['root_vel'], out['root_ang_vel']], -1) if wrong == 'velocities' else torch.zeros(n, 6, dtype=dtype)
    root = torch.cat([out['root_pos'], out['root_rot'], vel], -1)
    return dict(t=t32, reset=reset, terminate=torch.zeros_like(reset), root=root, dof_pos=out['dof_pos'],
                dof_vel=out['dof_vel'] if wrong == 'velocities' else torch.zeros_like(out['dof_pos']), body_pos=out['key_pos'],
                body_rot=body_rot)


def advance(motion_ids, progress, reset, terminate, num_motions, env_ids=None, wrong=None):
    """_reset_env_tensors, in place, for the rows with reset != 0 or for env_ids (-1 and ids outside the buffers skipped); a row
    whose motion id is outside the library is left as it is -> the full-length id list (e, or -1)."""
    n = motion_ids.numel()
    if env_ids is None:
        due = reset != 0
    else:
        e = env_ids.long()
        due = torch.zeros(n, dtype=torch.bool)
        due[e[(e >= 0) & (e < n)]] = True
    due = due & (motion_ids >= 0) & (motion_ids < num_motions)
    step = 1 if wrong == '+1' else n
    motion_ids[due] = torch.remainder(motion_ids[due] + step, num_motions).to(motion_ids.dtype)
    for buf in (progress, reset, terminate):
        buf[due] = 0
    return torch.where(due, torch.arange(n), -1).to(torch.int32)


def allowance(e_ref, ref64):
    """The bar of the device tests: 2 e_ref + 2^-23 max |ref| + 1e-7 against the f64 restatement."""
    return 2.0 * e_ref + 2.0 ** -23 * float(ref64.abs().max()) + 1e-7


def load_fixture():
    return torch.load(os.path.join(GOLDEN, 'view_motion.pt'), weights_only=False)
