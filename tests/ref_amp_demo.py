"""The draws of ``ase_hip_amp_demo_fetch`` stated in numpy, from the draw table in include/ase_hip.h, on the stream
of tests/ref_rollout.py and ``clip_cdf``'s search - and the fixtures the two test files of the demo fetch share.  TEST
INFRASTRUCTURE ONLY.

Draw j of sample i is element ``2 i + j`` of the Philox stream at (seed, offset): j = 0 the 24-bit integer behind the uniform
for the clip (``searchsorted(cdf, v, side='right')``: the first m with v < cdf[m]), j = 1 the uniform u of the time,
``t0 = u * (length[m] - trunc) + trunc`` in ``np.float32``, operation by operation."""
import numpy as np
import torch

from tests import ref_amp_obs as R
from tests import ref_rollout as RR

SEED = (1 << 33) + 11            # above 2^32
OFFSETS = (0, (1 << 32) + 7)
WEIGHTS = (None, [0.0, 1.0, 0.0, 2.0])       # equal weights; two clips that are never drawn
DT, STEPS = 1.0 / 30.0, 10                   # the fixture's history: truncate_time = 0.3 - clips 0 and 1 are shorter, 2 and 3 longer


def truncate_time(dt, steps):
    """What ``AmpObsDemoSource`` passes: the f64 product, rounded to f32 where torch subtracts / adds it."""
    return np.float32(dt * (steps - 1))


def draws(seed, offset, n):
    """Every sample's two draws -> dict of [n] arrays: v uint32 (24 bits), u f32 uniform."""
    e2 = np.uint64(2) * np.arange(n, dtype=np.uint64)
    w0 = RR.philox4x32_10(e2, offset, seed)
    w1 = RR.philox4x32_10(e2 + np.uint64(1), offset, seed)
    return {'v': w0[2] >> np.uint32(8), 'u': RR.keep_uniform(w1[2])}


def ref_draws(seed, offset, n, cdf, lengths, trunc):
    """The draw table -> (motion_ids int32 [n], motion_times0 f32 [n]).  cdf: the integer clip table; lengths: f32 clip lengths;
    trunc: the f32 scalar the host passes."""
    d = draws(seed, offset, n)
    m = np.searchsorted(np.asarray(cdf).astype(np.int64), d['v'].astype(np.int64), side='right')
    length = np.asarray(lengths, dtype=np.float32)[m]
    tr = np.float32(trunc)
    span = (length - tr).astype(np.float32)
    t0 = ((d['u'] * span).astype(np.float32) + tr).astype(np.float32)
    return m.astype(np.int32), t0


def slot_times(t0, dt, steps):
    """The f32 time of every (sample, slot): t0 + (float)(-dt) * (float)k, product and sum rounded on their own."""
    t0 = np.asarray(t0, dtype=np.float32)
    step = (np.float32(-dt) * np.arange(steps, dtype=np.float32)).astype(np.float32)
    return (t0[:, None] + step[None, :]).astype(np.float32)


INTERIOR, BEFORE_START, LAST_FRAME = 0, 1, 2


def frame_pair_kinds(clips, ids, times):
    """Per (sample, slot) the kind of frame pair ``calc_frame_blend`` (utils/motion_lib.py:263-272, in f32) gives: a negative time
    clamps to the first frame (the blend turns negative), a time at or beyond the end pairs the last frame with itself."""
    ids = torch.as_tensor(np.asarray(ids)).long()
    t = torch.as_tensor(np.asarray(times, dtype=np.float32))
    shape = t.shape
    idx = ids.view(-1, 1).expand(shape).reshape(-1)
    i0, i1, _, _, _ = R.calc_frame_blend(t.reshape(-1), clips['lengths'][idx], clips['num_frames'].long()[idx], clips['dt'][idx])
    kind = torch.full_like(i0, INTERIOR)
    kind[t.reshape(-1) < 0] = BEFORE_START
    kind[i0 == i1] = LAST_FRAME
    return kind.view(shape).numpy()


def layout_library(layout, seed=0):
    """Three random clips for the character of ``ref_amp_obs.LAYOUTS[layout]``: J + 2 bodies (body 0 the root, joint j on body
    j + 1, one body no joint uses), key bodies spread over all of them (repeated when there are more keys than bodies)."""
    offs, K = R.LAYOUTS[layout]
    J, D = len(offs) - 1, offs[-1]
    B = J + 2
    g = torch.Generator().manual_seed(7000 + seed + sum(map(ord, layout)))
    frames, dts = (2, 7, 12), (1.0 / 30.0, 1.0 / 60.0, 1.0 / 30.0)
    T = sum(frames)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    unit = lambda q: q / q.norm(dim=-1, keepdim=True)
    clips = {'gts': rn(T, B, 3).float(), 'grs': unit(rn(T, B, 4)).float(), 'lrs': unit(rn(T, B, 4)).float(), 'grvs': rn(T, 3).float(),
             'gravs': rn(T, 3).float(), 'dvs': rn(T, D).float()}
    nfs = torch.tensor(frames)
    clips['num_frames'] = nfs.to(torch.int32)
    clips['length_starts'] = (torch.cumsum(nfs, 0) - nfs).to(torch.int32)
    clips['dt'] = torch.tensor(dts, dtype=torch.float64).float()
    clips['lengths'] = torch.tensor([dt * (nf - 1) for nf, dt in zip(frames, dts)], dtype=torch.float64).float()
    clips.update(dof_body_ids=list(range(1, J + 1)), dof_offsets=list(offs), key_body_ids=[(3 * k + 1) % B for k in range(K)])
    return clips


TINY_OFFSETS, TINY_KEYS = [0, 1], [2, 0, 1, 2, 1, 0, 2, 1]    # F = 13 + 6 + 1 + 24 = 44: one slot is the tiny agents' AMP observation
TINY_STEPS = 1


def tiny_library(seed=0):
    """Two clips of a one-hinge character with eight key bodies (F = 44), for the agents of tests/golden/amp_tiny.pt."""
    g = torch.Generator().manual_seed(7100 + seed)
    frames, dts = (9, 14), (1.0 / 30.0, 1.0 / 60.0)
    T, B = sum(frames), 3
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    unit = lambda q: q / q.norm(dim=-1, keepdim=True)
    clips = {'gts': rn(T, B, 3).float(), 'grs': unit(rn(T, B, 4)).float(), 'lrs': unit(rn(T, B, 4)).float(), 'grvs': rn(T, 3).float(),
             'gravs': rn(T, 3).float(), 'dvs': rn(T, 1).float()}
    nfs = torch.tensor(frames)
    clips['num_frames'] = nfs.to(torch.int32)
    clips['length_starts'] = (torch.cumsum(nfs, 0) - nfs).to(torch.int32)
    clips['dt'] = torch.tensor(dts, dtype=torch.float64).float()
    clips['lengths'] = torch.tensor([dt * (nf - 1) for nf, dt in zip(frames, dts)], dtype=torch.float64).float()
    clips.update(dof_body_ids=[1], dof_offsets=list(TINY_OFFSETS), key_body_ids=list(TINY_KEYS))
    return clips


def ring_rows_of(head, n, ring_rows):
    return (head + torch.arange(n)) % ring_rows
