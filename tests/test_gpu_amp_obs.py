"""``ase_hip_build_amp_obs`` and ``ase_hip_motion_state`` (csrc/amp_obs.hip, csrc/amp_frames.h, the f32 half of csrc/quat.h) on
the MI355X against tests/ref_amp_obs.py: the reference's own expressions in f64 - NOT the emulator, which
tests/test_amp_obs_ref.py holds to the same cases and bounds on the CPU.  Floats per group (one output or column block within
one decision class) within 2 max e_ref + 2^-23 max |ref| + 1e-7 (+ the acos allowance derived in the reference module);
copies, shifted history slots and untouched elements bitwise; outputs and the history are windows of NaN-filled allocations,
inputs sit in NaN-filled allocations, every guard word is checked after each launch.  ``ASE_AMP_OBS_REPORT=<path>`` writes
the cases run, elements compared, guard words checked and max |hip - f64| beside max e_ref per output and group."""
import json
import os

import pytest
import torch

from tests import ref_amp_obs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FLAGS = ((True, True), (True, False), (False, True), (False, False))


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    yield HipBackend()
    out = os.environ.get('ASE_AMP_OBS_REPORT')
    if out:
        with open(out, 'w') as f:
            json.dump(R.report(), f, indent=1)


@pytest.fixture(scope='module')
def motion_cases():
    return {n: R.motion_case(n) for n in R.MOTION_N}


@pytest.mark.parametrize('n', R.MOTION_N)
def test_motion_state(be, motion_cases, n):
    R.check_motion(be, DEV, motion_cases[n])


def test_motion_state_then_build_amp_obs(be, motion_cases):
    R.check_chain(be, DEV, motion_cases[130])


def test_build_amp_obs(be):
    missed = []                                        # every case runs; a miss of a bound does not hide the later ones
    for c in R.obs_plan():
        try:
            R.check_obs(be, DEV, c)
        except AssertionError as e:
            missed.append((c['name'], str(e)[:300]))
    assert not missed, missed


@pytest.mark.parametrize('flags', (FLAGS[0], FLAGS[3]), ids=('local', 'world'))
def test_non_finite(be, flags):
    """NaN / +-inf in the root rotation, a hinge, an exponential map (-> the identity rotation, as the reference), the root
    velocity and a key position: what the reference module produces, element by element."""
    c = R.nonfinite_case(flags)
    got = R.check_obs(be, DEV, c)[:, 0]
    f32 = R.obs_reference(c)[0]
    r = 3 + 2 * len(R.NONFINITE)                       # the rows with a non-finite exponential map component: joint 1
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    for k in range(3):
        assert torch.equal(f32[r + k, 19:25], ident) and torch.equal(got[r + k, 19:25], ident)


def _library(be, motion_cases):
    from ase_amd.motion_lib import DeviceMotionLib
    return DeviceMotionLib.from_arrays(motion_cases[130]['clips'], be, DEV)


def _direct(be, ml, ids, times):
    wins = [R.window(s, DEV) for s in ((ids.shape[0], 3), (ids.shape[0], 4), (ids.shape[0], R.LIB_OFFSETS[-1]), (ids.shape[0], 3),
                                       (ids.shape[0], 3), (ids.shape[0], R.LIB_OFFSETS[-1]), (ids.shape[0], len(R.LIB_KEYS), 3))]
    outs = [w[0] for w in wins]
    R.run_motion_state(be, ml.clips, ids, times, outs)
    for k, (v, whole) in zip(R.OUT_NAMES, wins):
        R.guards_intact(whole, v.numel(), 'motion_state ' + k)
    return outs


def test_device_motion_lib_is_the_direct_entry(be, motion_cases):
    c = motion_cases[130]
    ml = _library(be, motion_cases)
    got = ml.get_motion_state(c['ids'].long().to(DEV), c['times'].to(DEV))
    want = _direct(be, ml, c['ids'].to(DEV), c['times'].to(DEV).contiguous())
    for k, a, b in zip(R.OUT_NAMES, got, want):
        R.bitwise(a, b, 'DeviceMotionLib.get_motion_state ' + k)


def test_fetch_amp_obs_demo_is_the_direct_entries(be, motion_cases):
    from ase_amd.motion_lib import AmpObsDemoSource
    ml = _library(be, motion_cases)
    src = AmpObsDemoSource(ml, be, num_amp_obs_steps=10, dt=1.0 / 30.0)
    seen = {}
    sample_motions, sample_time = ml.sample_motions, ml.sample_time
    ml.sample_motions = lambda n: seen.setdefault('ids', sample_motions(n))
    ml.sample_time = lambda ids, truncate_time=None: seen.setdefault('t', sample_time(ids, truncate_time=truncate_time))
    n, S = 37, 10
    got = src.fetch_amp_obs_demo(n).clone()
    trunc = src.dt * (S - 1)
    times0 = seen['t'] + trunc
    times = (times0.unsqueeze(-1) + (-src.dt * torch.arange(0, S, device=DEV))).reshape(-1)
    ids = seen['ids'].view(-1, 1).expand(n, S).reshape(-1).to(torch.int32).contiguous()
    o = dict(zip(R.OUT_NAMES, _direct(be, ml, ids, times.float().contiguous())))
    F = 13 + 6 * R.LIB_J + R.LIB_OFFSETS[-1] + 3 * len(R.LIB_KEYS)
    hist, whole = R.window((n * S, 1, F), DEV)
    i = {'root_pos': o['root_pos'], 'root_rot': o['root_rot'], 'root_vel': o['root_vel'], 'root_ang_vel': o['root_ang_vel'],
         'dof_pos': o['dof_pos'], 'dof_vel': o['dof_vel'], 'key_body_pos': o['key_pos']}
    R.run_build(be, i, R.LIB_OFFSETS, (True, True), hist, False)
    R.guards_intact(whole, hist.numel(), 'fetch_amp_obs_demo')
    assert got.shape == (n, S * F)
    R.bitwise(got, hist.view(n, S * F), 'fetch_amp_obs_demo')
