"""The AMP observation / motion sampler reference (tests/ref_amp_obs.py) without a GPU: held to the reference's recordings, the
emulator (oracle/amp_obs.py behind ``EmuBackend``) held to it on every case and bound of tests/test_gpu_amp_obs.py, the
conditions the fixtures promise as assertions (margins, branch counts, no row left out, the share of ill-conditioned
elements), fifteen single-term wrong restatements that must each fail a bound, and the operand refusals of the two C entries."""
import ctypes
import math
import os

import pytest
import torch

from ase_amd import lib as L
from tests import ref_amp_obs as R
from tests.emu_backend import EmuBackend
from tests.helpers import close

EPS24 = R.EPS24


@pytest.fixture(scope='module')
def motion_cases():
    cases = [R.motion_case(n) for n in R.MOTION_N]
    for c in cases:
        R.motion_reference(c)
    return cases


@pytest.fixture(scope='module')
def obs_cases():
    cases = R.obs_plan() + [R.nonfinite_case(f) for f in ((True, True), (False, False))]
    for c in cases:
        R.obs_reference(c)
    return cases


# ---------------------------------------------------------------------------------------------------- the recordings
@pytest.mark.parametrize('local_root,root_h', [(True, True), (True, False), (False, True), (False, False)])
def test_reference_matches_recorded_amp_obs(golden_dir, local_root, root_h):
    G = torch.load(os.path.join(golden_dir, 'amp_obs.pt'), weights_only=False)
    i = G['inputs']
    got, _ = R.build_amp_observations(i['root_pos'], i['root_rot'], i['root_vel'], i['root_ang_vel'], i['dof_pos'], i['dof_vel'],
                                      i['key_body_pos'], local_root, root_h, G['dof_offsets'])
    close(got, G['outputs'][(local_root, root_h)], 1e-5, 3e-6, 'amp obs frame')


def test_reference_matches_recorded_motion_state(golden_dir):
    G = torch.load(os.path.join(golden_dir, 'motion_state.pt'), weights_only=False)
    out, _ = R.get_motion_state(G['clips'], G['motion_ids'], G['times'], torch.float32)
    for k, ref in G['outputs'].items():
        if k in ('root_vel', 'root_ang_vel', 'dof_vel'):
            assert torch.equal(out[k], ref), k
        else:
            close(out[k], ref, 2e-5, 2e-5, 'motion ' + k)


# ---------------------------------------------------------------------------------------------------- the emulator
def test_emulator_motion_state(motion_cases):
    for c in motion_cases:
        R.check_motion(EmuBackend(), 'cpu', c)
    R.check_chain(EmuBackend(), 'cpu', motion_cases[-1])


def test_emulator_build_amp_obs(obs_cases):
    for c in obs_cases:
        R.check_obs(EmuBackend(), 'cpu', c)


def test_reference_backend_passes_its_own_checks(motion_cases, obs_cases):
    for c in motion_cases:
        R.check_motion(R.RefBackend(), 'cpu', c)
    R.check_chain(R.RefBackend(), 'cpu', motion_cases[-1])
    for c in obs_cases:
        R.check_obs(R.RefBackend(), 'cpu', c)


# ---------------------------------------------------------------------------------------------------- fixture conditions
def _planted_joints(ids):
    return torch.tensor([[R.joint_pattern(int(m), j) in R.PLANTED for j in range(R.LIB_J)] for m in ids])


def test_motion_fixture_margins(motion_cases):
    """Every row takes the same decisions in f32 and in f64, and outside the planted groups the f32 decision variable keeps
    its distance from the threshold.  Rows whose frame pair is one frame twice (the i1 clamp) are left out of the slerp
    class comparison alone: c = |q|^2 is 1 within rounding there and every class returns q0."""
    for c in motion_cases:
        o32, d32, o64, d64 = R.motion_reference(c)
        ids = c['ids'].long()
        n = ids.shape[0]
        assert torch.equal(d32['f0'], d64['f0']) and torch.equal(d32['f1'], d64['f1'])
        pair = (d32['f0'] != d32['f1'])
        exact = torch.tensor([k in R.EXACT_KINDS and (k != 'on_frame' or int(m) == 2) for k, m in zip(c['kinds'], ids)])
        var, raw = d32['frame_var'], d32['phase_raw']
        near = var.round()
        inside = ~exact & (raw > 0) & (raw < 1)                                        # clipped phases sit on frame 0 / the last
        assert bool(((var - near).abs() >= R.MARGIN * near.clamp_min(1.0))[inside].all())
        assert bool((torch.minimum(raw.abs(), (raw - 1).abs()) >= R.MARGIN)[~exact].all())
        assert bool((var == near)[~inside].all())                                      # exactly on its frame
        planted_root = torch.tensor([R.ROOT_PATTERN[int(m)] in R.PLANTED for m in ids])
        for who, planted in (('root', planted_root), ('local', _planted_joints(ids))):
            a, b = d32[who], d64[who]
            p = pair if who == 'root' else pair.view(n, 1).expand_as(a['cls'])
            assert torch.equal(a['cls'][p], b['cls'][p]) and torch.equal(a['flip'][p], b['flip'][p]), who
            free = p & ~planted
            cc, s = a['c'][free], a['s'][free]
            assert bool((cc.abs() >= R.MARGIN).all())                                  # the sign flip
            assert bool(((s - 0.001).abs() >= R.MARGIN * 0.001).all())                 # the midpoint
            assert bool((cc.abs() <= 1.0 - 2 * EPS24).all())                           # c >= 1: two ulps below
        assert torch.equal(d32['aa_mask'], d64['aa_mask'])
        free = ~_planted_joints(ids)
        assert bool(((d32['aa_sin'] - 1e-5).abs() >= R.MARGIN * 1e-5)[free].all())
        assert bool((d32['aa_w'].abs() >= R.MARGIN)[free & d32['aa_mask']].all())          # the wrap at angle = pi
        lab = R.motion_labels(c)
        for k, extra in (('root_pos', None), ('root_rot', None), ('key_pos', None), ('dof_pos', d64['acos_allowance'])):
            frac = R.allowance_fraction(o32[k], o64[k], extra)
            print(c['name'], k, 'share of elements with an allowance above 1e-4:', frac)
            assert frac <= 0.05, (c['name'], k, frac)
        assert lab['dof'].shape == o64['dof_pos'].shape                                # no row without a group


def test_motion_branch_counts(motion_cases):
    c = motion_cases[-1]
    _, d, _, _ = R.motion_reference(c)
    t, ids = c['times'], c['ids'].long()
    ln = c['clips']['lengths'][ids]
    both = lambda k: torch.cat([d['root'][k].view(-1, 1), d['local'][k]], 1)
    pair = (d['f0'] != d['f1']).view(-1, 1)
    rows = lambda m: int(m.any(-1).sum()) if m.dim() > 1 else int(m.sum())
    counts = {
        'flip': rows(both('flip') & pair), 'midpoint': rows((both('cls') == R.SLERP_MID) & pair),
        'c >= 1': rows((both('cls') == R.SLERP_ONE) & pair), 'generic': rows((both('cls') == R.SLERP_GENERIC) & pair),
        'sin_theta <= 1e-5': rows(d['aa_sin'] <= 1e-5), 'w > 1': rows(torch.isnan(d['aa_sin'])),
        'w < 0': rows((d['aa_w'] < 0) & d['aa_mask']),
        'second wrap': rows(d['hinge_theta'].abs() > math.pi),                # angle * axis_y past pi before the hinge's wrap
        't < 0': rows(t < 0), 't > length': rows(t > ln), 'i1 clamp': rows(~pair.view(-1)),
        'on a frame': rows((d['frame_var'] == d['frame_var'].round()) & (t >= 0) & (t <= ln)), 'length_starts != 0': rows(ids > 0),
        'midpoint + flip': rows((d['local']['cls'] == R.SLERP_MID) & d['local']['flip'] & pair),
    }
    print(counts)
    assert all(v >= 8 for v in counts.values()), counts


def test_obs_fixture_margins(obs_cases):
    huge = R.HUGE
    for c in obs_cases:
        if c.get('nonfinite'):
            continue
        f32, d32, f64, d64 = R.obs_reference(c)
        jc = c['joint_cls']
        assert torch.equal(d32['em_mask'][jc != huge], d64['em_mask'][jc != huge])
        assert not d32['em_mask'][jc == huge].any()                          # the f32 length overflows: the default
        assert bool(((d32['em_var'].abs() - 1e-5).abs() >= R.MARGIN * 1e-5)[jc != huge].all())
        names = [m[0] for m in R.EXP_MENU]
        for m, nm in enumerate(names):
            assert bool((d32['em_mask'][jc == m] == (nm not in R.EXP_DEFAULT)).all()), nm
        xy = d32['rot_dir'][:, :2].norm(dim=-1)
        assert bool((xy[c['row_cls'] == 0] >= R.MARGIN).all())
        v = d32['rot_dir'][c['row_cls'] == 1]
        assert torch.equal(v, torch.tensor([[0.0, 0.0, 1.0]]).expand_as(v))  # exactly vertical: heading = atan2(0, 0)
        g64 = torch.where((jc == huge).repeat_interleave(6, 1), f32[:, 13:13 + 6 * jc.shape[1]].double(), f64[:, 13:13 + 6 * jc.shape[1]])
        full = f64.clone()
        full[:, 13:13 + 6 * jc.shape[1]] = g64
        extra = torch.zeros_like(full)
        extra[:, 13:13 + 6 * jc.shape[1]] = d64['len_allowance'].repeat_interleave(6, 1)
        frac = R.allowance_fraction(f32, full, extra)
        assert frac <= 0.05, (c['name'], frac)


def test_obs_branch_counts(obs_cases):
    c = next(c for c in obs_cases if c['layout'] == 'humanoid' and c['N'] == 130)
    jc = c['joint_cls']
    counts = {nm: int((jc == m).any(-1).sum()) for m, nm in enumerate(R.JOINT_NAMES)}
    print(counts)
    assert all(v >= 8 for v in counts.values()), counts
    layouts = {c['layout'] for c in obs_cases}
    assert layouts == set(R.LAYOUTS) and R.frame_size('f255') == 255 and R.frame_size('k0') == 29
    assert {(c['S'], c['shift']) for c in obs_cases} >= {(s, sh) for s in (1, 2, 10) for sh in (True, False)}
    assert {c['N'] * R.frame_size(c['layout']) % 256 for c in obs_cases if c['layout'] in ('hinge1', 'f255') and c['S'] == 2} \
        >= {253, 0, 276 - 256}


# ---------------------------------------------------------------------------------------------------- wrong restatements
@pytest.mark.parametrize('name', R.MUTATIONS)
def test_wrong_restatement_fails_a_bound(name, motion_cases, obs_cases):
    """Each single-term wrong restatement, run as the 'device', fails a comparison on these fixtures."""
    failed = []
    with R.mutated(name):
        be = R.RefBackend()
        for c in motion_cases:
            try:
                R.check_motion(be, 'cpu', c)
            except AssertionError as e:
                failed.append((c['name'], str(e)[:120]))
        for c in obs_cases:
            try:
                R.check_obs(be, 'cpu', c)
            except AssertionError as e:
                failed.append((c['name'], str(e)[:120]))
    print(name, len(failed), failed[:1])
    assert failed, name


# ---------------------------------------------------------------------------------------------------- operand refusals
def test_entries_refuse_bad_operands_without_gpu():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()
    ia = lambda *xs: (ctypes.c_int32 * len(xs))(*xs)

    def build(**kw):
        a = dict(root_pos=p, root_rot=p, root_vel=p, root_ang_vel=p, dof_pos=p, dof_vel=p, key=p, n_envs=4, n_dof=4, n_key=1,
                 offs=ia(0, 3, 4), n_joints=2, local=1, height=1, hist=p, n_steps=2, shift=1)
        a.update(kw)
        return lib.ase_hip_build_amp_obs(a['root_pos'], a['root_rot'], a['root_vel'], a['root_ang_vel'], a['dof_pos'], a['dof_vel'],
                                         a['key'], a['n_envs'], a['n_dof'], a['n_key'], a['offs'], a['n_joints'], a['local'],
                                         a['height'], a['hist'], a['n_steps'], a['shift'], None)

    for k in ('root_pos', 'root_rot', 'root_vel', 'root_ang_vel', 'dof_pos', 'dof_vel', 'key', 'hist', 'offs'):
        assert build(**{k: None}) == -1 and b'build_amp_obs: null operand' in err(), k
    # Acceptance is shown WITHOUT a launch (these operands are host memory): the call carries a defect that a LATER check
    # refuses, so the later check's message proves that the earlier one let the operands pass.
    assert build(key=None, n_key=0, offs=ia(0, 3, 6)) == -1 and b'do not cover' in err()      # no key bodies: NULL key_body_pos passes
    assert build(offs=ia(0, 2, 4)) == -1 and b'has 2 dofs' in err()
    assert build(offs=ia(0, 3, 6)) == -1 and b'do not cover' in err()
    assert build(offs=ia(1, 4, 5), n_dof=5) == -1 and b'do not cover' in err()
    assert build(n_joints=0) == -1 and b'bad sizes' in err()
    assert build(n_joints=33, offs=ia(*range(34)), n_dof=33) == -1 and b'bad sizes' in err()
    assert build(n_envs=0) == -1 and build(n_steps=0) == -1 and build(n_key=-1) == -1 and build(n_dof=0) == -1
    # F = 13 + 6 J + D + 3 K.  255 floats are the whole 64 KB tile and pass; 256 are refused.  The tile check precedes the
    # per-joint checks, so a 2-dof joint behind it is reached at F = 255 and not at F = 256 - and nothing is launched.
    two = lambda n: ia(0, 2, *range(3, n + 2))                               # n joints, the first of 2 dofs
    assert build(offs=two(19), n_joints=19, n_dof=20, n_key=36) == -1 and b'has 2 dofs' in err()          # 13 + 114 + 20 + 108 = 255
    assert build(offs=two(20), n_joints=20, n_dof=21, n_key=34) == -1 and b'256 floats' in err()          # 13 + 120 + 21 + 102 = 256
    assert build(offs=two(20), n_joints=20, n_dof=21, n_key=33) == -1 and b'has 2 dofs' in err()          # 253
    assert build(offs=ia(*range(22)), n_joints=21, n_dof=21, n_key=32) == -1 and b'256 floats' in err() and b'staging tile' in err()

    def motion(**kw):
        a = dict(gts=p, grs=p, lrs=p, grvs=p, gravs=p, dvs=p, n_bodies=5, lengths=p, num_frames=p, dt=p, length_starts=p,
                 motion_ids=p, times=p, n=4, dof_body_ids=ia(1, 2), offs=ia(0, 3, 4), n_joints=2, key_ids=ia(4, 0), n_key=2,
                 root_pos=p, root_rot=p, dof_pos=p, root_vel=p, root_ang_vel=p, dof_vel=p, key_pos=p)
        a.update(kw)
        return lib.ase_hip_motion_state(a['gts'], a['grs'], a['lrs'], a['grvs'], a['gravs'], a['dvs'], a['n_bodies'], a['lengths'],
                                        a['num_frames'], a['dt'], a['length_starts'], a['motion_ids'], a['times'], a['n'],
                                        a['dof_body_ids'], a['offs'], a['n_joints'], a['key_ids'], a['n_key'], a['root_pos'],
                                        a['root_rot'], a['dof_pos'], a['root_vel'], a['root_ang_vel'], a['dof_vel'], a['key_pos'], None)

    for k in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'num_frames', 'dt', 'length_starts', 'motion_ids', 'times',
              'dof_body_ids', 'offs', 'root_pos', 'root_rot', 'dof_pos', 'root_vel', 'root_ang_vel', 'dof_vel', 'key_pos', 'key_ids'):
        assert motion(**{k: None}) == -1 and b'motion_state: null operand' in err(), k
    assert motion(key_pos=None, key_ids=None, n_key=0, dof_body_ids=ia(1, 5)) == -1 and b'body 5' in err()    # NULL passes, no launch
    assert motion(offs=ia(0, 2, 4)) == -1 and b'2 dofs' in err()
    assert motion(offs=ia(1, 4, 5)) == -1 and b'do not cover' in err()
    assert motion(n_joints=0) == -1 and b'bad sizes' in err()
    assert motion(n_joints=33, offs=ia(*range(34)), dof_body_ids=ia(*([1] * 33))) == -1 and b'bad sizes' in err()
    assert motion(n_key=33) == -1 and motion(n=0) == -1 and motion(n_bodies=0) == -1
    assert motion(dof_body_ids=ia(1, 5)) == -1 and b'body 5' in err()
    assert motion(dof_body_ids=ia(-1, 2)) == -1
    assert motion(key_ids=ia(4, 5)) == -1 and b'key body 5 out of range' in err()
    assert motion(key_ids=ia(-1, 0)) == -1
