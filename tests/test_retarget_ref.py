"""The retargeter without a GPU: the restatement of the reference's pipeline (tests/ref_retarget.py) against
the reference's own recorded outputs (tests/golden/retarget.pt, scripts/make_golden_retarget.py), the emulator of the launches
(tests/emu_retarget.py) under ``ase_amd.retarget.Retargeter`` against the f64 restatement to the GPU bounds, the conditions
the fixture promises, single-term wrong restatements that must fail, and the file / motion-library entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd import lib as L
from ase_amd import retarget as RT
from ase_amd.motion_lib import DeviceMotionLib, read_clip, write_clip
from tests import emu_motion_load as EM
from tests import emu_retarget as E
from tests import ref_retarget as R

CASES = ('cmu', 'sfu', 'global', 'unmapped', 'nohinge', 'topology')
OUTPUTS = ('rotation', 'root_translation', 'global_velocity', 'global_angular_velocity')
RUN_ARGS = (os.path.join(EM.CLIP_DIR, 'amp_humanoid_run.npy'), [1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14],
            [0, 3, 6, 9, 10, 13, 14, 17, 18, 21, 24, 25, 28], [5, 8, 11, 14])


@pytest.fixture(scope='module')
def G():
    return R.load_fixture()


@pytest.fixture(scope='module')
def ref64(G):
    """The f64 restatement of every case, computed once: (stages per clip, |w| of every quat_pos operand, dir0.y per limb)."""
    out = {}
    for name in CASES:
        rec, R.W_LOG = [], []
        try:
            S = R.case_setup(G[name], torch.float64)
            stages = R.pipeline(S, G[name]['clips'], G[name]['trims'], record=rec)
            out[name] = (stages, torch.cat(R.W_LOG), rec, S.last_global)
        finally:
            R.W_LOG = None
    return out


def test_fixture_holds_the_cases_of_the_issue(G):
    assert set(CASES) <= set(G)
    frames = lambda n: [c['rotation'].shape[0] for c in G[n]['clips']]
    assert frames('cmu') == [2, 18, 40] and [c['fps'] for c in G['cmu']['clips']] == [120, 60, 30]
    assert [tuple(t) for t in G['cmu']['trims']] == [(-1, -1), (-1, -1), (5, 33)] and G['cmu']['outputs'][2]['rotation'].shape[0] == 28
    assert frames('sfu') == [3, 17] and frames('global') == [18] and not G['global']['clips'][0]['is_local']
    assert G['cmu']['clips'][0]['rotation'].shape[1] == 38 and G['sfu']['clips'][0]['rotation'].shape[1] == 30
    assert G['unmapped']['outputs'][0]['rotation'].shape[1] == 17 and not G['nohinge']['hinges']
    assert os.path.getsize(os.path.join(EM.GOLDEN, 'retarget.pt')) < 1000 * 1000


def test_restatement_reproduces_the_recording(G):
    """Check 1: the restatement evaluated in f32 is BITWISE the unmodified reference, per stage and per output, on every clip of
    every case - no element is left out."""
    n = 0
    for name in CASES:
        g = G[name]
        out = R.pipeline(R.case_setup(g, torch.float32), g['clips'], g['trims'])
        assert len(out) == len(g['outputs'])
        for o, ref in zip(out, g['outputs']):
            for k in R.STAGES:
                n += EM.bits_equal(o[k].contiguous(), ref[k].contiguous())
    print(f'{n} elements bitwise equal to the recording')
    assert n > 20000


@pytest.mark.parametrize('name', CASES)
def test_emulator_meets_the_gpu_bounds(G, ref64, name):
    """Check 2: Retargeter over the emulated launches against the f64 restatement, to the bounds the kernels are held to."""
    be = E.EmuRetarget()
    out = E.run_case(G[name], be, 'cpu')
    assert be.launches[-(7 if G[name]['hinges'] else 6):] == (
        ['retarget_fk', 'retarget_chain', 'retarget_pose'] + (['retarget_hinge'] if G[name]['hinges'] else []) +
        ['retarget_ground', 'retarget_finish', 'retarget_velocity'])
    check_outputs(out, ref64[name][0], G[name])


def check_outputs(out, ref, g):
    """Every element of every output of every clip against the f64 restatement; -> worst error / bound per output."""
    worst, loose, quats = {}, 0, 0
    assert len(out) == len(ref)
    for c, (o, r) in enumerate(zip(out, ref)):
        fps = g['clips'][c]['fps']
        for k in OUTPUTS:
            got = o[k].detach().cpu()
            assert got.dtype == torch.float32 and got.shape == r[k].shape, (k, got.shape, r[k].shape)
            if k == 'rotation':
                err, n = R.quat_error(got, r[k])
                loose, quats = loose + n, quats + got.shape[0] * got.shape[1]
            else:
                err = (got.double() - r[k]).abs()
            ratio = float((err / R.bound(k, r[k], fps, g['hinges'])).max())
            worst[k] = max(worst.get(k, 0.0), ratio)
            print(f'clip {c} {k}: worst error / bound {ratio:.3f}')
            assert ratio <= 1.0, (c, k, ratio)
        assert o['fps'] == float(fps) and o['is_local'] is True
    assert loose <= 0.05 * quats
    return worst


@pytest.mark.parametrize('name', CASES)
def test_fixture_conditions(G, ref64, name):
    """Check 3, on the f64 restatement alone."""
    stages, w, rec, last_global = ref64[name]
    small = int((w < 1e-3).sum())
    print(f'{name}: {w.numel()} quat_pos operands, {small} with |w| < 1e-3 (min {float(w.min()):.3g})')
    assert small <= 0.05 * w.numel()                      # those are compared up to one common sign (ref_retarget.quat_error)
    if G[name]['hinges']:
        taken, other = 0, 0
        for clip in rec:
            for upper, _, _, _, sense in R.LIMBS:
                y = clip[upper]
                assert float(y.abs().min()) >= 1e-3, (upper, float(y.abs().min()))
                t = int((y <= 0).sum()) if sense < 0 else int((y >= 0).sum())
                taken, other = taken + t, other + y.numel() - t
        frames = sum(s['rotation'].shape[0] for s in stages)
        print(f'{name}: twist branch taken {taken}, not taken {other}; each bend sign on {2 * frames} limb frames')
        assert taken >= 8 and other >= 8 and frames >= 8
    if name in ('unmapped', 'topology'):
        names = R.case_poses(G[name])[1]['node_names']
        for body, ancestor in (('sword', 'right_hand'),) + ((('shield', 'left_lower_arm'),) if name == 'unmapped' else ()):
            EM.bits_equal(last_global[:, names.index(body)].contiguous(), last_global[:, names.index(ancestor)].contiguous())


def test_reference_error_is_reported_not_used(G, ref64):
    """Check 4: e_ref = |recording - f64 restatement| per output - the reference's own f32 arithmetic against its formulas.
    Printed (COVERAGE.md N16 quotes it); no test takes it as an allowance."""
    for name in CASES:
        for k in R.STAGES:
            e = max(float((rec[k].double() - ref[k]).abs().max()) for rec, ref in zip(G[name]['outputs'], ref64[name][0]))
            print(f'e_ref {name} {k}: {e:.3g}')
            assert np.isfinite(e)


WRONG_CASE = {'divide_before_filter': 'cmu', 'filter_wraps': 'cmu', 'central_ends': 'cmu', 'rotation_on_the_right': 'cmu',
              'scale_on_target_root': 'cmu', 'source_tree_recompose': 'topology', 'arm_bend_positive': 'cmu',
              'min_over_all_clips': 'cmu'}


@pytest.mark.parametrize('wrong', R.WRONG)
def test_wrong_restatements_fail(G, ref64, wrong):
    """Check 5: one wrong term - in f32 it no longer reproduces the recording (check 1's bitwise bound), and in f64 it breaks
    a GPU bound against the right restatement.  ``divide_before_filter`` is the exception to the second half: dividing before
    the linear filter is the same real number, only rounded in another order, so it can fail the bitwise bound alone."""
    g = G[WRONG_CASE[wrong]]
    out32 = R.pipeline(R.case_setup(g, torch.float32), g['clips'], g['trims'], wrong=wrong)
    assert any(not torch.equal(o[k], rec[k]) for o, rec in zip(out32, g['outputs']) for k in R.STAGES)
    out64 = R.pipeline(R.case_setup(g, torch.float64), g['clips'], g['trims'], wrong=wrong)
    worst = 0.0
    for c, (o, r) in enumerate(zip(out64, ref64[WRONG_CASE[wrong]][0])):
        for k in R.STAGES:                               # (the hands' rotations and the root's height are overwritten later:
            #                                                some wrong terms show in the stage's own output only)
            err = R.quat_error(o[k], r[k])[0] if k.endswith('rotation') else (o[k] - r[k]).abs()
            worst = max(worst, float((err / R.bound(k, r[k], g['clips'][c]['fps'], g['hinges'])).max()))
    print(f'{wrong}: worst error / bound {worst:.3g}')
    assert worst > 1.0 or wrong == 'divide_before_filter'


def test_filter_taps_are_scipys():
    w = R.gauss_weights()
    assert tuple(float(x) for x in w) == E.GAUSS and abs(2 * w.sum() - w[0] - 1.0) < 1e-15
    ndimage = pytest.importorskip('scipy.ndimage')
    x = np.random.default_rng(3).standard_normal((23, 4, 3)).astype(np.float32)
    for a in (x, x.astype(np.float64), x[:2], x[:3]):
        got, ref = R.gauss_filter(a), ndimage.gaussian_filter1d(a, 2, axis=0, mode='nearest')
        assert got.dtype == ref.dtype and np.array_equal(got, ref)
    assert np.array_equal(R.gradient(x), np.gradient(x, axis=0)) and np.array_equal(R.gradient(x[:2]), np.gradient(x[:2], axis=0))


# ---------------------------------------------------------------------------------------------- files and the motion library
def test_write_clip_round_trips_and_matches_the_shipped_layout(tmp_path):
    src = RUN_ARGS[0]
    x = read_clip(src)
    path = str(tmp_path / 'out.npy')
    write_clip(path, x)
    y = read_clip(path)
    assert list(x) == list(y)
    for k in x:
        if isinstance(x[k], np.ndarray):
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), k
        else:
            assert x[k] == y[k], k
    a, b = np.load(src, allow_pickle=True).item(), np.load(path, allow_pickle=True).item()
    assert type(a) is type(b) and list(a) == list(b) and list(a['skeleton_tree']) == list(b['skeleton_tree'])
    assert a['__name__'] == b['__name__'] == 'SkeletonMotion' and type(a['fps']) is type(b['fps']) and type(a['is_local']) is type(b['is_local'])
    for k in ('rotation', 'root_translation', 'global_velocity', 'global_angular_velocity'):
        assert a[k]['arr'].dtype == b[k]['arr'].dtype and a[k]['context'] == b[k]['context'] and list(a[k]) == list(b[k]), k
    for k in ('parent_indices', 'local_translation'):
        assert a['skeleton_tree'][k]['arr'].dtype == b['skeleton_tree'][k]['arr'].dtype
        assert a['skeleton_tree'][k]['context'] == b['skeleton_tree'][k]['context']
    # torch tensors (what the retargeter returns) write the same file
    t = dict(x, **{k: torch.from_numpy(x[k]).float() for k in ('rotation', 'root_translation', 'global_velocity', 'global_angular_velocity')})
    write_clip(path, t)
    assert np.array_equal(read_clip(path)['rotation'], x['rotation'].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError, match='expected'):
        write_clip(path, dict(x, root_translation=x['root_translation'][:3]))


def test_read_clip_refuses_global_clips_unless_asked(tmp_path):
    x = read_clip(RUN_ARGS[0])
    path = str(tmp_path / 'global.npy')
    write_clip(path, dict(x, is_local=False))
    with pytest.raises(ValueError, match='stores global rotations'):
        read_clip(path)
    y = read_clip(path, allow_global=True)
    assert y['is_local'] is False and x['is_local'] is True and np.array_equal(y['rotation'], x['rotation'])
    with pytest.raises(ValueError, match='global rotations'):
        DeviceMotionLib.from_clips([y], *RUN_ARGS[1:], EM.EmuMotionLoad(), 'cpu')


@pytest.mark.parametrize('motion_file', ['amp_humanoid_run.npy', 'three.yaml'])
def test_from_clips_equals_from_file(motion_file):
    g = EM.load_fixture()['b' if motion_file.endswith('.npy') else 'a']
    args = EM.case_args(g)
    a = DeviceMotionLib.from_file(*args, EM.EmuMotionLoad(), 'cpu')
    from ase_amd.motion_lib import fetch_motion_files
    files, weights = fetch_motion_files(args[0])
    clips = [read_clip(f) for f in files]
    b = DeviceMotionLib.from_clips(clips, *args[1:], EM.EmuMotionLoad(), 'cpu', weights=weights)
    as_torch = [dict(c, **{k: torch.from_numpy(c[k]) for k in ('rotation', 'root_translation', 'global_velocity', 'global_angular_velocity')})
                for c in clips]
    d = DeviceMotionLib.from_clips(as_torch, *args[1:], EM.EmuMotionLoad(), 'cpu', weights=weights)
    for other in (b, d):
        for k in EM.ARRAYS + EM.TABLES:
            assert torch.equal(a.clips[k], other.clips[k]), k
        assert torch.equal(a._motion_weights, other._motion_weights) and torch.equal(a.clip_cdf, other.clip_cdf)
        assert torch.equal(a.fps, other.fps)
    assert a.motion_files == files


def test_retargeted_clips_enter_a_motion_library(G, tmp_path):
    """Retargeter.from_config on the fixture's copies of the reference's files -> write_clip -> from_file equals from_clips."""
    be = E.EmuRetarget()
    r = RT.Retargeter.from_config(os.path.join(R.RETARGET_DIR, 'retarget_sfu_to_amp.json'), R.RETARGET_DIR, be, 'cpu')
    assert r.trim == (0, 100) and r.config['scale'] == 0.01
    clips = r.retarget([dict(c, rotation=c['rotation'].numpy(), root_translation=c['root_translation'].numpy()) for c in G['sfu']['clips']])
    for c, ref in zip(clips, G['sfu']['outputs']):
        assert c['rotation'].shape == ref['rotation'].shape              # trim_frame_end 100 on 3 / 17 frames: the clip's own end
    path = str(tmp_path / 'clip.npy')
    write_clip(path, clips[1])
    a = DeviceMotionLib.from_file(path, *RUN_ARGS[1:], EM.EmuMotionLoad(), 'cpu')
    b = DeviceMotionLib.from_clips(clips[1:], *RUN_ARGS[1:], EM.EmuMotionLoad(), 'cpu')
    for k in EM.ARRAYS + EM.TABLES:
        assert torch.equal(a.clips[k], b.clips[k]), k


def test_refusals(G):
    src, tgt = R.case_poses(G['cmu'])
    g = G['cmu']
    make = lambda **kw: RT.Retargeter(E.EmuRetarget(), 'cpu', kw.pop('source', src), kw.pop('target', tgt),
                                      kw.pop('mapping', g['joint_mapping']), g['rotation'], g['scale'], **kw)
    with pytest.raises(ValueError, match='parent 2 of body 1 does not precede it'):
        RT.tree_table([-1, 2, 0])
    with pytest.raises(ValueError, match='does not precede'):
        make(source=dict(src, parent_indices=np.roll(src['parent_indices'], 1)))
    with pytest.raises(ValueError, match='reduced trees have different sizes'):
        make(mapping=dict(g['joint_mapping'], Neck='no_such_body'))
    with pytest.raises(ValueError, match='root node cannot be dropped'):
        make(mapping={k: v for k, v in g['joint_mapping'].items() if k != 'Hips'})
    big = RT.zero_pose([f'b{i}' for i in range(65)], [-1] + list(range(64)), np.zeros((65, 3)))
    with pytest.raises(ValueError, match=r'65 bodies \(1-64\)'):
        make(source=big)
    with pytest.raises(ValueError, match="no body 'left_elbow'"):
        make(hinges={'limbs': (('left_upper_arm', 'left_elbow', 'left_hand', -1, -1),)})
    r = make()
    clip = dict(g['clips'][1], rotation=g['clips'][1]['rotation'].numpy(), root_translation=g['clips'][1]['root_translation'].numpy())
    with pytest.raises(ValueError, match=r'1 frame\(s\) after trimming 18 to \[4, 5\)'):
        r.retarget([clip], trim=(4, 5))
    with pytest.raises(ValueError, match='2 ranges for 1 clips'):
        r.retarget([clip], trim=[(0, 5), (0, 5)])
    with pytest.raises(ValueError, match='local and in global form'):
        r.retarget([clip, dict(clip, is_local=False)])
    with pytest.raises(ValueError, match='do not describe frames of the 38 source bodies'):
        r.retarget([dict(clip, rotation=clip['rotation'][:, :30])])
    with pytest.raises(ValueError, match="not a 'SkeletonState'"):
        RT.read_tpose(RUN_ARGS[0])


def test_entry_points_refuse_on_the_host():
    """The host-side checks of the ase_hip_retarget_* entries run before any launch, so without a GPU."""
    lib = L.load()
    assert L.ABI_VERSION == 9
    err = lambda: lib.ase_hip_last_error()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fk = lambda **kw: lib.ase_hip_retarget_fk(*{**dict(rotation=p, mode=0, tree=p, tree_ld=3, n_bodies=2, clip_first=p, clip_num_frames=p,
                                                   src_first=p, frame_clip=p, n_clips=1, n_frames=2, n_src_frames=2, out=p,
                                                   stream=None), **kw}.values())
    assert fk(rotation=None) == -1 and b'retarget_fk: null operand' in err()
    assert fk(out=None) == -1 and b'null' in err()
    assert fk(mode=3) == -1 and b'mode 3' in err()
    assert fk(n_bodies=65) == -1 and b'65 bodies (1-64)' in err()
    assert fk(n_frames=0) == -1 and b'frames' in err()
    assert fk(n_clips=3) == -1 and b'bad sizes' in err()
    assert fk(n_src_frames=1) == -1 and b'bad sizes' in err()
    assert fk(tree_ld=70) == -1 and b'tree table' in err()
    assert lib.ase_hip_retarget_chain(p, 2, p, p, p, p, 3, 3, p, 2, p, None) == -1 and b'3 mapped bodies of 2' in err()
    assert lib.ase_hip_retarget_chain(p, 2, None, p, p, p, 3, 2, p, 2, p, None) == -1 and b'retarget_chain: null' in err()
    assert lib.ase_hip_retarget_pose(*([p] * 8), 2, 2, *([p] * 4), 1, 2, 2, p, None, None) == -1 and b'retarget_pose: null' in err()
    assert lib.ase_hip_retarget_hinge(p, p, p, p, 3, None, 2, 2, p, None) == -1 and b'retarget_hinge: null' in err()
    assert lib.ase_hip_retarget_ground(p, p, p, p, 3, 2, p, p, 3, 2, p, None) == -1 and b'bad sizes' in err()
    assert lib.ase_hip_retarget_finish(*([p] * 6), 3, 2, p, 1, 2, p, p, p, None, None) == -1 and b'retarget_finish: null' in err()
    assert lib.ase_hip_retarget_velocity(p, p, 2, p, p, p, p, 2, 3, p, p, None) == -1 and b'a clip has 2 or more' in err()
    for name in ('fk', 'chain', 'pose', 'hinge', 'ground', 'finish', 'velocity'):
        assert f'ase_hip_retarget_{name}' in L.SIGNATURES and hasattr(torch.ops.ase_hip, f'retarget_{name}')
