"""The clip loader on the MI355X: ``DeviceMotionLib.from_file`` -> ``ase_hip_clip_frames`` against the reference
loader's recorded arrays (tests/golden/motion_load.pt, tests/golden/motion_state.pt), end to end from a file to
``get_motion_state`` and to a ``HumanoidAMPTensors`` reset batch, the torch operator, and memory the launch must not touch.

Tolerances (derived, not measured).  Copies are bitwise: lrs, grvs, gravs, every table.  The computed arrays differ from the
recording only through the device's f64 ``sqrt`` / ``acos`` and the order of the sums inside a norm - a few units of 2^-53
relative per operation - and then one rounding to f32:
  gts, grs   |x - ref| <= ulp_f32(ref) + 1e-12: a value near a rounding boundary may round the other way; 1e-12 absolute for
             components near zero (chain depth <= 6, about 20 operations per link, magnitudes <= 10 m: 10 x 120 x 1.1e-16)
  dvs        |x - ref| <= ulp_f32(ref) + 6e-8 / dt: acos(2 w^2 - 1) is ill-conditioned near the identity; an argument error of
             16 x 2^-53 moves the angle by at most min(delta / angle, sqrt(2 delta)) = 6e-8 rad
"""
import os

import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd import motion_lib as ML
from ase_amd.amp_env import HumanoidAMPTensors
from ase_amd.motion_lib import DeviceMotionLib
from tests import emu_amp_reset as R
from tests import emu_motion_load as E

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = ['a', 'b', 'c']


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(DEV)


@pytest.fixture(scope='module')
def G():
    return E.load_fixture()


def _frame_dt(clips):
    """The f64 frame time 1 / fps of every frame's clip, [T, 1] (from the recorded f32 table: the bound needs no more)."""
    return torch.repeat_interleave(clips['dt'].double().cpu(), clips['num_frames'].long().cpu()).unsqueeze(-1)


def _check_arrays(got, ref, dt, what):
    """got / ref: dicts of the six arrays (got on any device); dt [T, 1].  Prints the largest deviation per array and the
    number of elements that are not bitwise equal, then asserts the bounds of the module docstring.  -> all bitwise?"""
    all_equal = True
    for k in E.ARRAYS:
        x, r = got[k].cpu(), ref[k]
        assert x.shape == r.shape and x.dtype == r.dtype == torch.float32, (what, k, x.shape, r.shape)
        assert bool(torch.isfinite(x).all()), (what, k)
        err = (x.double() - r.double()).abs()
        n_diff = int((x.view(torch.int32) != r.view(torch.int32)).sum())
        all_equal &= n_diff == 0
        print(f'{what} {k}: max |hip - ref| {float(err.max()):.3g}, {n_diff} of {x.numel()} elements not bitwise equal')
        if k in ('lrs', 'grvs', 'gravs'):
            assert n_diff == 0, (what, k, n_diff)
            continue
        bound = E.ulp_f32(r) + (1e-12 if k in ('gts', 'grs') else 6e-8 / dt)
        bad = err > bound
        assert not bool(bad.any()), (what, k, int(bad.sum()), float((err - bound).max()))
    return all_equal


@pytest.mark.parametrize('name', CASES)
def test_from_file_matches_the_reference_loader(be, G, name):
    g = G[name]
    ml = DeviceMotionLib.from_file(*E.case_args(g), be, DEV)
    torch.cuda.synchronize()
    c = g['clips']
    assert all(ml.clips[k].is_cuda for k in E.ARRAYS + E.TABLES)
    _check_arrays(ml.clips, c, _frame_dt(c), name)
    E.bits_equal(ml.clips['lengths'].cpu(), c['lengths'])
    E.bits_equal(ml.clips['dt'].cpu(), c['dt'])
    E.bits_equal(ml.clips['num_frames'].cpu(), c['num_frames'].to(torch.int32))
    E.bits_equal(ml.clips['length_starts'].cpu(), c['length_starts'].to(torch.int32))
    E.bits_equal(ml._motion_weights.cpu(), g['weights'])
    E.bits_equal(ml.fps, g['fps'])
    assert [os.path.basename(f) for f in ml.motion_files] == g['motion_files']


def test_first_two_clips_match_the_motion_state_fixture(be, G, golden_dir):
    M = torch.load(os.path.join(golden_dir, 'motion_state.pt'), weights_only=False)['clips']
    ml = DeviceMotionLib.from_file(*E.case_args(G['a']), be, DEV)
    T2 = M['gts'].shape[0]
    _check_arrays({k: ml.clips[k][:T2] for k in E.ARRAYS}, M, _frame_dt(M), 'motion_state.pt')
    for k in E.TABLES:
        assert torch.equal(ml.clips[k][:2].cpu().long() if k in ('num_frames', 'length_starts') else ml.clips[k][:2].cpu(), M[k]), k


@pytest.mark.parametrize('name', CASES)
def test_motion_state_from_a_file(be, G, name):
    """File -> from_file -> get_motion_state against the reference's outputs: 2e-5 for the interpolated ones
    (tests/test_gpu_ops.py::test_motion_state_matches_reference); root_vel / root_ang_vel are rows of grvs / gravs (bitwise),
    dof_vel rows of dvs (the bound of dvs)."""
    from tests.helpers import close
    g = G[name]
    ml = DeviceMotionLib.from_file(*E.case_args(g), be, DEV)
    out = ml.get_motion_state(g['motion_ids'].to(DEV), g['times'].to(DEV))
    torch.cuda.synchronize()
    assert len(out) == 7
    for k, o in zip(E.OUT_NAMES, out):
        ref = g['outputs'][k]
        o = o.cpu()
        assert o.shape == ref.shape, k
        if k in ('root_vel', 'root_ang_vel'):
            E.bits_equal(o, ref)
        elif k == 'dof_vel':
            dt = g['clips']['dt'].double()[g['motion_ids']].unsqueeze(-1)
            err = (o.double() - ref.double()).abs()
            print(f'{name} dof_vel: max |hip - ref| {float(err.max()):.3g}')
            assert bool((err <= E.ulp_f32(ref) + 6e-8 / dt).all()), k
        else:
            close(o, ref, 2e-5, 2e-5, f'{name} motion {k}')


def _reset_batch(be, GR, ml, sc):
    """One reset batch of a recorded scenario of tests/golden/amp_reset.pt on the motion library ml -> state and history."""
    at = HumanoidAMPTensors(be, ml, GR['num_envs'], num_amp_obs_steps=GR['num_amp_obs_steps'], dt=GR['dt'],
                            state_init=sc['state_init'], hybrid_init_prob=GR['hybrid_init_prob'], local_root_obs=GR['local_root_obs'],
                            root_height_obs=GR['root_height_obs'], generator=torch.Generator(device=DEV).manual_seed(0))
    init, _ = R.tables(GR, device=DEV)
    at.set_initial_state(*init)
    s, bufs = R.prefill(GR, device=DEV)
    s.pop('amp_obs_buf')
    at.amp_obs_buf.copy_(R.hist_pattern(*at.amp_obs_buf.shape))
    at.apply_reset(s, R.plan_of(GR, sc, DEV), bufs['progress_buf'], bufs['reset_buf'], bufs['terminate_buf'])
    torch.cuda.synchronize()
    res = {k: s[k].cpu() for k in ('humanoid_root_states', 'dof_pos', 'dof_vel')}
    res['amp_obs_buf'] = at.amp_obs_buf.cpu()
    return res


@pytest.mark.parametrize('scenario', ['random', 'hybrid'])
def test_reset_batch_from_files_equals_reset_batch_from_arrays(be, G, tmp_path, scenario):
    """Wiring: a HumanoidAMPTensors reset on a library loaded from the files of the two clips of tests/golden/amp_reset.pt and
    on from_arrays of the recorded arrays.  Bitwise where the loaded arrays are bitwise equal to the recorded ones, otherwise
    within 2e-5 (the tolerance of the motion-state test)."""
    GR, clips = R.load_fixture()
    files = G['a']['motion_files'][:2]                     # the two clips of motion_state.pt, on which amp_reset.pt was recorded
    assert all(G['a'][k] == clips[k] for k in ('dof_body_ids', 'dof_offsets', 'key_body_ids'))
    sc = GR['scenarios'][scenario]
    assert not sc['getup'] and any(k == 2 for k in sc['plan']['kind'])           # rows that read the clips
    y = tmp_path / 'two.yaml'
    y.write_text('motions:\n' + ''.join(f'  - file: "{os.path.join(E.CLIP_DIR, c)}"\n    weight: 0.5\n' for c in files))
    from_files = DeviceMotionLib.from_file(str(y), clips['dof_body_ids'], clips['dof_offsets'], clips['key_body_ids'], be, DEV)
    from_arrays = DeviceMotionLib.from_arrays(clips, be, DEV)
    bitwise = _check_arrays(from_files.clips, clips, _frame_dt(clips), 'amp_reset clips')
    for k in E.TABLES:
        assert torch.equal(from_files.clips[k], from_arrays.clips[k]), k
    a, b = _reset_batch(be, GR, from_files, sc), _reset_batch(be, GR, from_arrays, sc)
    for k in a:
        assert a[k].shape == b[k].shape
        err = float((a[k].double() - b[k].double()).abs().max())
        print(f'{scenario} {k}: loaded arrays bitwise equal: {bitwise}, max |files - arrays| {err:.3g}')
        if bitwise:
            E.bits_equal(a[k], b[k])
        else:
            assert err <= 2e-5, (k, err)
    assert not torch.equal(a['amp_obs_buf'], R.hist_pattern(*a['amp_obs_buf'].shape))      # (the batch wrote something)


def _raw(g):
    """The uploaded operands of a case, in the argument order of HipBackend.clip_frames."""
    h = ML.read_motion_files(*E.case_args(g))
    up = lambda k, dt: torch.as_tensor(h[k], dtype=dt).contiguous().to(DEV)
    return (up('rotation', torch.float64), up('root_translation', torch.float64), up('root_velocity', torch.float64),
            up('root_angular_velocity', torch.float64), up('local_translation', torch.float32), h['parent_indices'],
            up('length_starts', torch.int32), up('num_frames', torch.int32), up('fps', torch.float64), up('frame_clip', torch.int32),
            h['dof_body_ids'], h['dof_offsets'])


@pytest.mark.parametrize('name', ['a', 'b'])
def test_torch_op_and_repeated_calls_give_the_same_bytes(be, G, name):
    a = _raw(G[name])
    first = be.clip_frames(*a)
    second = be.clip_frames(*a)
    op = torch.ops.ase_hip.clip_frames(*a[:5], *a[6:10], a[5], a[10], a[11])
    torch.cuda.synchronize()
    assert len(first) == len(second) == len(op) == 6
    for x, y, z in zip(first, second, op):
        E.bits_equal(x.cpu(), y.cpu())
        E.bits_equal(x.cpu(), z.cpu())
    with pytest.raises(RuntimeError, match='clip_frames'):
        torch.ops.ase_hip.clip_frames(a[0].float(), *a[1:5], *a[6:10], a[5], a[10], a[11])


def test_launch_writes_only_its_outputs(be, G):
    """Outputs allocated with a guard row before and after: the guards keep their fill, every row between is written."""
    g = G['a']
    a = _raw(g)
    T, B, D = a[0].shape[0], a[0].shape[1], g['dof_offsets'][-1]
    fill = float.fromhex('0x1.fp+100')
    bufs = [torch.full((T + 2,) + s, fill, dtype=torch.float32, device=DEV) for s in ((B, 3), (B, 4), (B, 4), (3,), (3,), (D,))]
    out = be.clip_frames(*a, out=tuple(b[1:-1] for b in bufs))
    plain = be.clip_frames(*a)
    torch.cuda.synchronize()
    for b, o, p in zip(bufs, out, plain):
        assert bool((b[0] == fill).all()) and bool((b[-1] == fill).all())
        assert o.data_ptr() == b[1].data_ptr() and not bool((b[1:-1] == fill).any())
        E.bits_equal(b[1:-1].cpu(), p.cpu())
