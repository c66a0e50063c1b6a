"""The clip loader without a GPU: the host reader of ``DeviceMotionLib.from_file`` (file list, tables,
refusals), the f64 restatement of ``ase_hip_clip_frames`` (tests/emu_motion_load.py) against the reference loader's recorded
arrays - BITWISE -, ``from_file`` through the emulated backend, the host-side operand checks of the C entry, and the conditions
the generator of tests/golden/motion_load.pt promises, re-checked on the file."""
import collections
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from ase_amd import lib as L
from ase_amd import motion_lib as ML
from ase_amd.motion_lib import DeviceMotionLib
from tests import emu_motion_load as E

CASES = ['a', 'b', 'c']
REFERENCE = os.environ.get('ASE_REFERENCE', '/root/reference/ase')


@pytest.fixture(scope='module')
def G():
    return E.load_fixture()


@pytest.fixture(scope='module')
def loaded(G):
    """case -> (library loaded from the file through the emulated backend, that backend)."""
    out = {}
    for name in CASES:
        be = E.EmuMotionLoad()
        out[name] = (DeviceMotionLib.from_file(*E.case_args(G[name]), be, 'cpu'), be)
    return out


# ---- host reader ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_host_reader_tables_match_the_reference(G, name):
    g = G[name]
    path, dof_body_ids, dof_offsets, key_body_ids = E.case_args(g)
    h = ML.read_motion_files(path, dof_body_ids, dof_offsets, key_body_ids)
    assert [os.path.basename(f) for f in h['motion_files']] == g['motion_files']
    assert all(os.path.dirname(f) == E.CLIP_DIR for f in h['motion_files'])          # relative to the yaml's directory
    c = g['clips']
    E.bits_equal(torch.tensor(h['lengths'], dtype=torch.float32), c['lengths'])
    E.bits_equal(torch.tensor(h['dt'], dtype=torch.float32), c['dt'])
    E.bits_equal(torch.tensor(h['fps'], dtype=torch.float32), g['fps'])
    E.bits_equal(torch.tensor(h['num_frames']), c['num_frames'])
    E.bits_equal(torch.tensor(h['length_starts']), c['length_starts'])
    w = torch.tensor(h['weights'], dtype=torch.float32)
    E.bits_equal(w / w.sum(), g['weights'])
    T = int(c['num_frames'].sum())
    assert h['rotation'].dtype == np.float64 and h['rotation'].shape == (T,) + tuple(c['lrs'].shape[1:])
    assert h['local_translation'].dtype == np.float32 and h['local_translation'].shape == (len(h['motion_files']), c['lrs'].shape[1], 3)
    assert h['frame_clip'].tolist() == [i for i, n in enumerate(h['num_frames']) for _ in range(n)]
    # the host computes nothing on frames: what it uploads is what the files hold
    f0 = 0
    for f, n in zip(h['motion_files'], h['num_frames']):
        d = np.load(f, allow_pickle=True).item()
        assert np.array_equal(h['rotation'][f0:f0 + n], d['rotation']['arr'])
        assert np.array_equal(h['root_translation'][f0:f0 + n], d['root_translation']['arr'])
        assert np.array_equal(h['root_velocity'][f0:f0 + n], d['global_velocity']['arr'][:, 0])
        assert np.array_equal(h['root_angular_velocity'][f0:f0 + n], d['global_angular_velocity']['arr'][:, 0])
        f0 += n


def test_yaml_and_single_file_forms():
    files, weights = ML.fetch_motion_files(os.path.join(E.CLIP_DIR, 'three.yaml'))
    assert len(files) == 3 and weights == [2.0, 1.0, 0.5]
    single = os.path.join(E.CLIP_DIR, 'amp_humanoid_run.npy')
    assert ML.fetch_motion_files(single) == ([single], [1.0])


def _clip(name='RL_Avatar_TurnLeft90_Motion.npy'):
    return np.load(os.path.join(E.CLIP_DIR, name), allow_pickle=True).item()


def _save(path, d):
    np.save(path, d, allow_pickle=True)
    return str(path)


TABLES_A = ([1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16], [0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31], [5, 10, 13, 16, 6, 9])


def _refused(path, match, tables=TABLES_A):
    with pytest.raises(ValueError, match=match) as e:
        DeviceMotionLib.from_file(str(path), *tables, E.EmuMotionLoad(), 'cpu')
    return str(e.value)


def test_refusals_name_the_file(tmp_path):
    good = os.path.join(E.CLIP_DIR, 'RL_Avatar_TurnLeft90_Motion.npy')
    # a wrong __name__
    d = _clip()
    d['__name__'] = 'SkeletonState'
    p = _save(tmp_path / 'state.npy', d)
    assert 'state.npy' in _refused(p, 'SkeletonMotion')
    # global rotations: refused, with the way out in the message (flag flipped, data untouched)
    d = _clip()
    d['is_local'] = False
    p = _save(tmp_path / 'global.npy', d)
    msg = _refused(p, 'is_local')
    assert 'global.npy' in msg and 're-save' in msg and 'local' in msg
    # fewer than 2 frames
    d = _clip()
    for k in ('rotation', 'root_translation', 'global_velocity', 'global_angular_velocity'):
        d[k] = collections.OrderedDict(arr=d[k]['arr'][:1], context=d[k]['context'])
    p = _save(tmp_path / 'one_frame.npy', d)
    assert 'one_frame.npy' in _refused(p, 'frame')
    # a parent that does not precede its child
    d = _clip()
    par = d['skeleton_tree']['parent_indices']['arr'].copy()
    par[3] = 5
    d['skeleton_tree']['parent_indices'] = collections.OrderedDict(arr=par, context=d['skeleton_tree']['parent_indices']['context'])
    p_bad_parent = _save(tmp_path / 'bad_parent.npy', d)
    assert 'bad_parent.npy' in _refused(p_bad_parent, 'precede')
    # clips of one dataset whose skeletons differ: another body count, other parents
    shutil.copy(good, tmp_path / 'good.npy')
    shutil.copy(os.path.join(E.CLIP_DIR, 'amp_humanoid_run.npy'), tmp_path / 'fifteen.npy')
    (tmp_path / 'mixed.yaml').write_text('motions:\n  - file: good.npy\n    weight: 1\n  - file: fifteen.npy\n    weight: 1\n')
    assert 'fifteen.npy' in _refused(tmp_path / 'mixed.yaml', 'differs')
    d = _clip()
    par = d['skeleton_tree']['parent_indices']['arr'].copy()
    par[6] = 4                                                    # the sword on the lower arm: still ordered, but another tree
    d['skeleton_tree']['parent_indices'] = collections.OrderedDict(arr=par, context=d['skeleton_tree']['parent_indices']['context'])
    _save(tmp_path / 'other_tree.npy', d)
    (tmp_path / 'trees.yaml').write_text('motions:\n  - file: good.npy\n    weight: 1\n  - file: other_tree.npy\n    weight: 1\n')
    assert 'other_tree.npy' in _refused(tmp_path / 'trees.yaml', 'differs')
    # joint sizes other than 1 or 3, ids outside the skeleton
    offs2 = list(TABLES_A[1])
    offs2[12] = 29                                                # joint 11: 2 dofs, joint 12: 2 dofs
    _refused(good, 'dofs', (TABLES_A[0], offs2, TABLES_A[2]))
    assert 'TurnLeft90' in _refused(good, 'dof_body_id 17', (TABLES_A[0][:-1] + [17], TABLES_A[1], TABLES_A[2]))
    assert 'TurnLeft90' in _refused(good, 'key_body_id -1', (TABLES_A[0], TABLES_A[1], [5, -1]))
    # weights
    (tmp_path / 'neg.yaml').write_text('motions:\n  - file: good.npy\n    weight: 1\n  - file: good.npy\n    weight: -0.5\n')
    assert 'neg.yaml' in _refused(tmp_path / 'neg.yaml', 'negative')
    (tmp_path / 'zero.yaml').write_text('motions:\n  - file: good.npy\n    weight: 0\n  - file: good.npy\n    weight: 0.0\n')
    assert 'zero.yaml' in _refused(tmp_path / 'zero.yaml', 'zero')
    # and the files these were made from load
    (tmp_path / 'ok.yaml').write_text('motions:\n  - file: good.npy\n    weight: 0\n  - file: good.npy\n    weight: 3\n')
    ml = DeviceMotionLib.from_file(str(tmp_path / 'ok.yaml'), *TABLES_A, E.EmuMotionLoad(), 'cpu')
    assert ml.num_motions() == 2 and ml._motion_weights.tolist() == [0.0, 1.0]


def test_local_translation_is_uploaded_per_clip(tmp_path):
    """The reference uses each clip's own skeleton offsets: a clip with longer arms next to the original."""
    d = _clip()
    lt = d['skeleton_tree']['local_translation']
    lt2 = lt['arr'].copy()
    lt2[4] *= np.float32(1.25)
    d['skeleton_tree']['local_translation'] = collections.OrderedDict(arr=lt2, context=lt['context'])
    _save(tmp_path / 'long_arm.npy', d)
    shutil.copy(os.path.join(E.CLIP_DIR, 'RL_Avatar_TurnLeft90_Motion.npy'), tmp_path / 'plain.npy')
    (tmp_path / 'two.yaml').write_text('motions:\n  - file: plain.npy\n    weight: 1\n  - file: long_arm.npy\n    weight: 1\n')
    ml = DeviceMotionLib.from_file(str(tmp_path / 'two.yaml'), *TABLES_A, E.EmuMotionLoad(), 'cpu')
    n = int(ml.clips['num_frames'][0])
    gts = ml.clips['gts']
    assert torch.equal(gts[:n, :4], gts[n:, :4]) and not torch.equal(gts[:n, 4], gts[n:, 4])
    for k in ('grs', 'lrs', 'dvs'):
        assert torch.equal(ml.clips[k][:n], ml.clips[k][n:])


# ---- the restatement against the reference loader's arrays ------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_restatement_is_bitwise_equal_to_the_reference_loader(G, loaded, name):
    ml, _ = loaded[name]
    c = G[name]['clips']
    T, B, D = int(c['num_frames'].sum()), c['gts'].shape[1], G[name]['dof_offsets'][-1]
    n = sum(E.bits_equal(ml.clips[k], c[k]) for k in E.ARRAYS)
    assert n == T * (3 * B + 4 * B + 4 * B + 3 + 3 + D)            # no element is left out
    E.bits_equal(ml.clips['lengths'], c['lengths'])
    E.bits_equal(ml.clips['dt'], c['dt'])
    E.bits_equal(ml.clips['num_frames'], c['num_frames'].to(torch.int32))
    E.bits_equal(ml.clips['length_starts'], c['length_starts'].to(torch.int32))
    E.bits_equal(ml._motion_weights, G[name]['weights'])
    E.bits_equal(ml.fps, G[name]['fps'])
    assert [os.path.basename(f) for f in ml.motion_files] == G[name]['motion_files']


def test_first_two_clips_are_those_of_the_motion_state_fixture(G, loaded, golden_dir):
    M = torch.load(os.path.join(golden_dir, 'motion_state.pt'), weights_only=False)['clips']
    ml, _ = loaded['a']
    T2 = M['gts'].shape[0]
    assert T2 == int(M['num_frames'].sum())
    for k in E.ARRAYS:
        E.bits_equal(ml.clips[k][:T2], M[k])
        E.bits_equal(G['a']['clips'][k][:T2], M[k])


@pytest.mark.parametrize('name', CASES)
def test_from_file_equals_from_arrays_and_samples_like_the_reference(G, loaded, name):
    g = G[name]
    ml, be = loaded[name]
    # (the files' own weights: from_arrays normalises what it is given, and normalising twice moves the last bit)
    ref = DeviceMotionLib.from_arrays(E.golden_clips(g), be, 'cpu', weights=ML.fetch_motion_files(E.case_args(g)[0])[1])
    assert set(ml.clips) == set(ref.clips)
    for k in ml.clips:
        if torch.is_tensor(ml.clips[k]):
            E.bits_equal(ml.clips[k], ref.clips[k])
        else:
            assert ml.clips[k] == ref.clips[k], k
    E.bits_equal(ml._motion_weights, ref._motion_weights)
    assert ml.num_motions() == ref.num_motions() and ml.get_total_length() == ref.get_total_length()
    out = ml.get_motion_state(g['motion_ids'], g['times'])
    assert len(out) == len(g['outputs']) == 7
    for k, o in zip(E.OUT_NAMES, out):
        assert o.shape == g['outputs'][k].shape
        assert float((o - g['outputs'][k]).abs().max()) <= 1e-6, k       # test_motion_state_restatement_matches_reference's


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_entry_point_validates_operands_without_gpu():
    """The host-side checks of ase_hip_clip_frames run before any launch: NULL operands, sizes, the kernel's table sizes, joint
    sizes, body ids and the order of the skeleton are refused with the entry's name in the message."""
    lib = L.load()
    assert 'ase_hip_clip_frames' in L.SIGNATURES and L.ABI_VERSION == 9
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()
    i32 = lambda xs: (ctypes.c_int32 * len(xs))(*xs)
    parents = [-1, 0, 1, 1, 3, 4, 5, 1, 7, 8, 8, 0, 11, 12, 0, 14, 15]

    def call(**kw):
        a = dict(rotation=p, root_translation=p, root_velocity=p, root_angular_velocity=p, local_translation=p,
                 parent_indices=i32(parents), n_bodies=17, clip_first=p, clip_num_frames=p, clip_fps=p, frame_clip=p, n_clips=2,
                 n_frames=100, dof_body_ids=i32(TABLES_A[0]), dof_offsets=i32(TABLES_A[1]), n_joints=13, gts=p, grs=p, lrs=p, grvs=p,
                 gravs=p, dvs=p, stream=None)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return lib.ase_hip_clip_frames(*a.values())

    for name in ('rotation', 'root_translation', 'root_velocity', 'root_angular_velocity', 'local_translation', 'parent_indices',
                 'clip_first', 'clip_num_frames', 'clip_fps', 'frame_clip', 'dof_body_ids', 'dof_offsets', 'gts', 'grs', 'lrs', 'grvs',
                 'gravs', 'dvs'):
        assert call(**{name: None}) == -1 and b'clip_frames' in err() and b'null' in err(), name
    assert call(n_frames=0) == -1 and b'clip_frames' in err() and b'sizes' in err()
    assert call(n_clips=0) == -1 and b'sizes' in err()
    assert call(n_frames=3) == -1 and b'sizes' in err()                # two clips of 2 or more frames do not fit 3 rows
    assert call(n_bodies=0) == -1 and b'bodies' in err()
    assert call(n_bodies=33, parent_indices=i32([-1] + list(range(32)))) == -1 and b'clip_frames' in err() and b'bodies' in err()
    assert call(n_joints=0) == -1 and b'joints' in err()
    assert call(n_joints=33) == -1 and b'joints' in err()
    offs2 = list(TABLES_A[1])
    offs2[12] = 29
    assert call(dof_offsets=i32(offs2)) == -1 and b'clip_frames' in err() and b'2 dofs' in err()
    assert call(dof_offsets=i32([1] + TABLES_A[1][1:])) == -1 and b'dof_offsets' in err()
    assert call(dof_body_ids=i32(TABLES_A[0][:-1] + [17])) == -1 and b'body 17' in err()
    assert call(dof_body_ids=i32([-1] + TABLES_A[0][1:])) == -1
    assert call(parent_indices=i32([-1, 0, 1, 5] + parents[4:])) == -1 and b'precede' in err()
    assert call(parent_indices=i32([0] + parents[1:])) == -1 and b'root' in err()
    assert call(parent_indices=i32([-1, -2] + parents[2:])) == -1
    with pytest.raises(L.AseHipError, match='clip_frames'):
        L.check(-1, 'clip_frames')


def test_torch_op_is_registered():
    import ase_amd.ops  # noqa: F401
    assert hasattr(torch.ops.ase_hip, 'clip_frames')
    schema = str(torch.ops.ase_hip.clip_frames.default._schema)
    assert schema.startswith('ase_hip::clip_frames(Tensor rotation, Tensor root_translation,') and 'Int[] dof_offsets)' in schema
    assert schema.endswith('-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)')
    with pytest.raises(NotImplementedError):                     # no CPU kernel: the product has no fallback
        z = torch.zeros(4, 2, 4, dtype=torch.float64)
        v = torch.zeros(4, 3, dtype=torch.float64)
        i = torch.zeros(1, dtype=torch.int32)
        torch.ops.ase_hip.clip_frames(z, v, v, v, torch.zeros(1, 2, 3), i, i, torch.ones(1, dtype=torch.float64),
                                      torch.zeros(4, dtype=torch.int32), [-1, 0], [1], [0, 3])


# ---- the generator's promises, re-checked on the committed files -----------------------------------------------------------
def test_fixture_keeps_its_conditions(G, loaded):
    sizes = set()
    zero_angles = 0
    for name in CASES:
        ml, be = loaded[name]
        g = G[name]
        # the sign flip of quat_pos can go only one way: no product in the chain or in the frame differences has w near 0
        assert be.min_abs_w >= 1e-9, (name, be.min_abs_w)
        zero_angles += be.zero_angles
        sizes |= {b - a for a, b in zip(g['dof_offsets'], g['dof_offsets'][1:])}
        lens = g['clips']['lengths'][g['motion_ids']]
        t = g['times']
        assert t[0] == 0 and t[1] == lens[1] and t[2] > lens[2]                   # start, exact end, past the end
        assert set(g['motion_ids'].tolist()) == set(range(ml.num_motions()))
    assert sizes == {1, 3}
    assert zero_angles >= 1                                                       # a joint with angle == 0 between two frames
    assert loaded['a'][1].min_abs_w < 0.1                                         # (and the margin above is not vacuous)
    a, b = G['a'], G['b']
    assert len(a['motion_files']) == 3 and len(set(a['weights'].tolist())) == 3   # unequal weights
    assert a['clips']['gts'].shape[1] == 17 and b['clips']['gts'].shape[1] == 15 and b['dof_offsets'][-1] == 28
    assert len(set(a['fps'].tolist())) > 1                                        # clips of different frame rates
    total = sum(os.path.getsize(os.path.join(E.CLIP_DIR, f)) for f in os.listdir(E.CLIP_DIR))
    assert total < 512 * 1024 and os.path.getsize(os.path.join(E.GOLDEN, 'motion_load.pt')) < 1024 * 1024


# ---- the whole shipped dataset, when the reference is there ----------------------------------------------------------------
def test_restatement_against_the_reference_loader_on_the_full_dataset():
    data = os.path.join(REFERENCE, 'data', 'motions', 'reallusion_sword_shield', 'dataset_reallusion_sword_shield.yaml')
    if not os.path.exists(data):
        pytest.skip('the reference tree is not mounted')
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the reference's loader in a process of its own (it changes sys.path and torch's JIT state)
    code = ('import sys, torch\n'
            f'sys.path.insert(0, {os.path.join(root, "oracle", "rl_games_shim")!r}); sys.path.insert(0, {REFERENCE!r})\n'
            'from utils.motion_lib import MotionLib\n'
            f'ml = MotionLib(motion_file={data!r}, dof_body_ids={TABLES_A[0]}, dof_offsets={TABLES_A[1]}, key_body_ids={TABLES_A[2]}, device="cpu")\n'
            'torch.save({k: getattr(ml, k) for k in ("gts", "grs", "lrs", "grvs", "gravs", "dvs", "_motion_lengths", "_motion_dt", '
            '"_motion_num_frames", "length_starts", "_motion_weights")}, sys.argv[1])\n')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'ref.pt')
        subprocess.run([sys.executable, '-c', code, out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        ref = torch.load(out, weights_only=False)
    be = E.EmuMotionLoad()
    ml = DeviceMotionLib.from_file(data, *TABLES_A, be, 'cpu')
    assert ml.num_motions() >= 80
    n = sum(E.bits_equal(ml.clips[k], ref[k]) for k in E.ARRAYS)
    assert n == ref['gts'].shape[0] * (11 * 17 + 6 + 31)
    E.bits_equal(ml.clips['lengths'], ref['_motion_lengths'])
    E.bits_equal(ml.clips['dt'], ref['_motion_dt'])
    E.bits_equal(ml.clips['num_frames'], ref['_motion_num_frames'].to(torch.int32))
    E.bits_equal(ml.clips['length_starts'], ref['length_starts'].to(torch.int32))
    E.bits_equal(ml._motion_weights, ref['_motion_weights'])
    assert be.min_abs_w >= 1e-9
