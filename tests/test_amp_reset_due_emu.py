"""Device-drawn HumanoidAMP / HumanoidAMPGetup resets without a GPU: the clip table of the weighted choice, the
logic of the reference plan (tests/ref_amp_reset_due.py) on tests/golden/amp_reset.pt, ``HumanoidAMPTensors.reset_due`` on the
CPU stand-in, and the host-side operand checks of ``ase_hip_amp_reset_due``."""
import ctypes

import numpy as np
import pytest
import torch

from ase_amd import lib as L
from ase_amd.amp_env import HumanoidAMPTensors
from ase_amd.motion_lib import DeviceMotionLib, clip_cdf
from tests import emu_amp_reset as E
from tests import ref_amp_reset_due as R

INITS = ['Default', 'Start', 'Random', 'Hybrid']


@pytest.fixture(scope='module')
def GC():
    return E.load_fixture()


def _cfg(G, state_init, getup):
    return dict(state_init=state_init, hybrid_init_prob=G['hybrid_init_prob'],
                getup=(G['recovery_episode_prob'], G['recovery_steps'], G['fall_init_prob']) if getup else None)


def _ref(G, clips, cfg, reset_buf, seed=R.SEED, offset=0, terminate=None):
    cdf = clip_cdf(torch.ones(clips['lengths'].numel()))
    term = G['buffers']['terminate_buf'] if terminate is None else terminate
    return R.ref_plan(seed, offset, reset_buf.numpy(), term.numpy(), cfg, cdf.numpy(), clips['lengths'].numpy(), G['num_fall_states'])


def _groups(P, N):
    due = P['env_ids'] >= 0
    k, s = P['kind'], P['src_rows']
    return {'recovery': due & (k == L.RESET_FRAME), 'fall': due & (k == L.RESET_TABLE) & (s >= N), 'motion': due & (k == L.RESET_MOTION),
            'default': due & (k == L.RESET_TABLE) & (s < N)}


# ---- the clip table ----------------------------------------------------------------------------------------------------------
def test_clip_cdf_never_draws_a_zero_weight_and_counts_are_the_intervals():
    cdf = clip_cdf([0, 1, 0, 2]).numpy().astype(np.int64)
    assert cdf[-1] == 1 << 24 and cdf.tolist() == [0, 5592405, 5592405, 1 << 24]
    clip = np.searchsorted(cdf, np.arange(1 << 24, dtype=np.int64), side='right')
    counts = np.bincount(clip, minlength=4)
    assert counts.tolist() == np.diff(cdf, prepend=0).tolist() and counts[0] == 0 and counts[2] == 0 and clip.max() == 3


def test_clip_cdf_refuses_a_weight_below_its_resolution():
    with pytest.raises(ValueError, match='clip 4'):
        clip_cdf([0, 1, 0, 2, 1e-9])
    with pytest.raises(ValueError):
        clip_cdf([0.0, 0.0])
    with pytest.raises(ValueError):
        clip_cdf([1.0, -1.0, 2.0])


def test_clip_cdf_equal_weights_and_the_motion_lib_owns_it(GC):
    cdf = clip_cdf([1, 1, 1])
    sizes = np.diff(cdf.numpy().astype(np.int64), prepend=0)
    assert cdf.dtype == torch.int32 and int(cdf[-1]) == 1 << 24 and sizes.max() - sizes.min() <= 1
    _, clips = GC
    ml = DeviceMotionLib.from_arrays(clips, None, 'cpu', weights=[1.0, 3.0])
    assert ml.clip_cdf.tolist() == [1 << 22, 1 << 24]
    with pytest.raises(ValueError, match='clip 1'):
        DeviceMotionLib.from_arrays(clips, None, 'cpu', weights=[1.0, 1e-9])


# ---- the plan's logic on the fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 5])
def test_getup_hybrid_plan_reaches_every_branch(GC, offset):
    G, clips = GC
    N = G['num_envs']
    assert (N, G['recovery_episode_prob'], G['fall_init_prob'], G['hybrid_init_prob'], G['num_fall_states']) == (32, 0.4, 0.3, 0.5, 12)
    reset = R.reset_pattern(N)
    P = _ref(G, clips, _cfg(G, 'Hybrid', True), reset, offset=offset)
    g = _groups(P, N)
    assert all(int(m.sum()) >= 2 for m in g.values()), {k: int(m.sum()) for k, m in g.items()}       # a condition of the seed
    due = P['env_ids'] >= 0
    assert np.array_equal(due, reset.numpy() != 0) and np.array_equal(P['env_ids'][due], np.arange(N)[due])
    assert sum(int(m.sum()) for m in g.values()) == int(due.sum())
    assert (G['buffers']['terminate_buf'].numpy()[g['recovery']] == 1).all()
    assert ((P['src_rows'][g['fall']] >= N) & (P['src_rows'][g['fall']] < N + 12)).all()
    assert np.array_equal(P['src_rows'][g['default']], np.arange(N)[g['default']])
    lengths = clips['lengths'].numpy()
    m = g['motion']
    assert (P['motion_times'][m] < lengths[P['motion_ids'][m]]).all() and (P['motion_times'][m] >= 0).all()
    assert set(P['motion_ids'][m].tolist()) <= {0, 1}
    for k in R.PLAN_KEYS[1:]:
        assert not P[k][~due].any(), k                                   # rows that are not due: -1 and zeros
        assert P[k].dtype == (np.float32 if k == 'motion_times' else np.int32)
    assert (P['env_ids'][~due] == -1).all()
    assert not P['motion_ids'][~m].any() and not P['motion_times'][~m].any() and not P['src_rows'][m | g['recovery']].any()
    # nobody recovers when nothing terminated
    none = _ref(G, clips, _cfg(G, 'Hybrid', True), reset, offset=offset, terminate=torch.zeros(N, dtype=torch.int64))
    assert not _groups(none, N)['recovery'].any()


@pytest.mark.parametrize('state_init', INITS)
@pytest.mark.parametrize('getup', [False, True])
def test_plan_follows_the_state_initialisation(GC, state_init, getup):
    G, clips = GC
    N = G['num_envs']
    reset = R.reset_pattern(N)
    P = _ref(G, clips, _cfg(G, state_init, getup), reset)
    g = _groups(P, N)
    rest = g['motion'] | g['default']
    if not getup:
        assert not g['recovery'].any() and not g['fall'].any()
    if state_init == 'Default':
        assert not g['motion'].any()
    elif state_init == 'Hybrid':
        assert g['motion'].any() and g['default'].any()
    else:
        assert not g['default'].any() and g['motion'].any()
    if state_init == 'Start':
        assert not P['motion_times'].any()                               # exactly 0
    if state_init == 'Random':
        assert (P['motion_times'][g['motion']] > 0).all()
    assert rest.any()
    # the draws are those of the stream: the uniform of element 8 e + 5 times the clip's length, one f32 product
    if state_init in ('Random', 'Hybrid'):
        d = R.draws(R.SEED, 0, N)
        m = g['motion']
        want = d['u5'][m] * clips['lengths'].numpy()[P['motion_ids'][m]]
        assert want.dtype == np.float32 and np.array_equal(P['motion_times'][m], want)


def test_draws_of_a_row_do_not_depend_on_the_other_rows(GC):
    G, clips = GC
    N = G['num_envs']
    cfg = _cfg(G, 'Hybrid', True)
    a, b = R.reset_pattern(N), torch.ones(N, dtype=torch.int64)
    Pa, Pb = _ref(G, clips, cfg, a), _ref(G, clips, cfg, b)
    both = (a != 0).numpy()
    assert both.sum() < N
    for k in R.PLAN_KEYS:
        assert np.array_equal(Pa[k][both], Pb[k][both]), k
    # ... but on the stream position and the seed
    assert not all(np.array_equal(Pb[k], _ref(G, clips, cfg, b, offset=1)[k]) for k in R.PLAN_KEYS)
    assert not all(np.array_equal(Pb[k], _ref(G, clips, cfg, b, seed=R.SEED + 1)[k]) for k in R.PLAN_KEYS)


# ---- the host class on the stand-in ------------------------------------------------------------------------------------------
class Deferred(R.EmuAmpResetDue):
    """Takes the call and runs the stand-in's arithmetic when asked, so that the host class alone runs under the patches."""

    def __init__(self):
        self.calls = []

    def amp_reset_due(self, *a, **kw):
        self.calls.append((a, kw))

    def run(self):
        for a, kw in self.calls:
            R.EmuAmpResetDue.amp_reset_due(self, *a, **kw)
        self.calls = []


def _tensors(G, clips, be, state_init, getup, seed=R.SEED):
    ml = DeviceMotionLib.from_arrays(clips, None, 'cpu')
    kw = {}
    if getup:
        kw.update(recovery_episode_prob=G['recovery_episode_prob'], recovery_steps=G['recovery_steps'], fall_init_prob=G['fall_init_prob'])
    at = HumanoidAMPTensors(be, ml, G['num_envs'], num_amp_obs_steps=G['num_amp_obs_steps'], dt=G['dt'], state_init=state_init,
                            hybrid_init_prob=G['hybrid_init_prob'], local_root_obs=G['local_root_obs'],
                            root_height_obs=G['root_height_obs'], seed=seed, **kw)
    init, fall = E.tables(G)
    at.set_initial_state(*init)
    if getup:
        at.set_fall_states(*fall)
    s, bufs = E.prefill(G)
    at.amp_obs_buf.copy_(s.pop('amp_obs_buf'))
    if getup:
        at.recovery_counter.copy_(bufs['recovery_counter'])
    bufs['reset_buf'] = R.reset_pattern(G['num_envs'])
    return at, s, bufs


@pytest.mark.parametrize('state_init,getup', [('Hybrid', True), ('Random', False), ('Default', False), ('Start', True)])
def test_reset_due_equals_apply_reset_of_the_reference_plan(GC, monkeypatch, state_init, getup):
    G, clips = GC
    N = G['num_envs']
    be = Deferred()
    at, s, bufs = _tensors(G, clips, be, state_init, getup)
    assert at.rng_state.tolist() == [R.SEED, 0] and at.rng_state.dtype == torch.int64
    assert set(at.plan) == set(R.PLAN_KEYS) and all(v.shape == (N,) for v in at.plan.values())
    reset0 = bufs['reset_buf'].clone()

    def refuse(name):
        def f(*a, **kw):
            raise AssertionError(f'{name} called by reset_due')
        return f
    for name in ('nonzero', 'sum', 'bernoulli', 'multinomial'):
        monkeypatch.setattr(torch.Tensor, name, refuse(name))
        monkeypatch.setattr(torch, name, refuse(name))
    be.host_call = refuse('host_call')
    plan = at.reset_due(s, bufs['progress_buf'], bufs['reset_buf'], bufs['terminate_buf'])
    monkeypatch.undo()
    del be.host_call
    assert plan is at.plan and len(be.calls) == 1
    be.run()
    assert at.rng_state.tolist() == [R.SEED, 1]
    # a second copy: apply_reset of the reference plan's due rows
    bt, t, bufs2 = _tensors(G, clips, E.EmuAmpReset(), state_init, getup)
    P = R.plan_tensors(_ref(G, clips, _cfg(G, state_init, getup), reset0))
    for k in R.PLAN_KEYS:
        assert torch.equal(plan[k], P[k]), k
    bt.apply_reset(t, R.due_rows(P), bufs2['progress_buf'], bufs2['reset_buf'], bufs2['terminate_buf'])
    for k in s:
        assert torch.equal(s[k], t[k]), k
    assert torch.equal(at.amp_obs_buf, bt.amp_obs_buf)
    for k in ('progress_buf', 'reset_buf', 'terminate_buf'):
        assert torch.equal(bufs[k], bufs2[k]), k
    due = reset0 != 0
    assert not bufs['reset_buf'].any() and not bufs['progress_buf'][due].any() and bufs['progress_buf'][~due].all()
    if getup:
        assert torch.equal(at.recovery_counter, bt.recovery_counter)
    # advance=False: the same position again
    at.reset_due(s, bufs['progress_buf'], bufs['reset_buf'], bufs['terminate_buf'], advance=False)
    be.run()
    assert at.rng_state.tolist() == [R.SEED, 1] and (at.plan['env_ids'] == -1).all()


def test_reset_due_checks_its_options(GC):
    G, clips = GC
    at, s, bufs = _tensors(G, clips, R.EmuAmpResetDue(), 'Hybrid', True)
    with pytest.raises(ValueError, match='terminate_buf'):
        at.reset_due(s, bufs['progress_buf'], bufs['reset_buf'])
    ml = DeviceMotionLib.from_arrays(clips, None, 'cpu')
    bare = HumanoidAMPTensors(R.EmuAmpResetDue(), ml, G['num_envs'], state_init='Default')
    with pytest.raises(ValueError, match='set_initial_state'):
        bare.reset_due(s, bufs['progress_buf'], bufs['reset_buf'])


# ---- the C entry's operand checks ------------------------------------------------------------------------------------------
def test_entry_point_validates_operands_without_gpu():
    """The host-side checks of ase_hip_amp_reset_due run before any launch: refused with ASE_EINVAL (-1), the entry's name and
    the operand in the message."""
    lib = L.load()
    assert len(L.SIGNATURES['ase_hip_amp_reset_due']) == 56
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()
    offs = (ctypes.c_int32 * 14)(0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31)
    bodies = (ctypes.c_int32 * 13)(1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16)
    keys = (ctypes.c_int32 * 6)(5, 10, 13, 16, 6, 9)

    def call(**kw):
        # Hybrid with the get-up options: every operand is in use.  Only refusals are called (a valid call would launch).
        a = dict(gts=p, grs=p, lrs=p, grvs=p, gravs=p, dvs=p, n_bodies=17, lengths=p, num_frames=p, dt=p, length_starts=p,
                 dof_body_ids=bodies, dof_offsets=offs, n_joints=13, key_body_ids=keys, n_key=6, cdf=p, n_clips=2, tab_root=p,
                 tab_dof_pos=p, tab_dof_vel=p, n_tab=28, state_init=L.INIT_HYBRID, hybrid_init_prob=0.5, getup=1,
                 recovery_episode_prob=0.4, fall_init_prob=0.3, recovery_steps=60, rng_state=p, advance=1, progress_buf=p, reset_buf=p,
                 terminate_buf=p, recovery_counter=p, env_ids_out=p, kind_out=p, motion_ids_out=p, motion_times_out=p, src_rows_out=p,
                 root_states=p, ld_root=13, dof_pos=p, dof_vel=p, ld_dof=31, dof_stride=1, body_pos=p, body_rot=p, body_vel=p,
                 body_ang_vel=p, n_envs=16, local_root_obs=1, root_height_obs=1, env_dt=1.0 / 30.0, hist=p, n_steps=10, stream=None)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return lib.ase_hip_amp_reset_due(*a.values())

    def refused(rc, *words):
        return rc == -1 and b'amp_reset_due' in err() and all(w in err() for w in words)

    assert refused(call(reset_buf=None), b'reset_buf') and refused(call(rng_state=None), b'rng_state')
    assert refused(call(state_init=4), b'state_init') and refused(call(state_init=-1), b'state_init')
    for name in ('tab_root', 'tab_dof_pos', 'tab_dof_vel'):
        assert refused(call(**{name: None}), b'Hybrid', b'tab_root_states'), name
        assert refused(call(**{name: None}, state_init=L.INIT_DEFAULT, getup=0), b'Default', b'tab_root_states'), name
        assert refused(call(**{name: None}, state_init=L.INIT_START), b'fall episodes', b'tab_root_states'), name
    assert refused(call(terminate_buf=None), b'terminate_buf') and refused(call(recovery_counter=None), b'recovery_counter')
    assert refused(call(n_tab=16), b'fall_init_prob', b'n_tab')                    # no fall rows behind the initial state
    assert refused(call(n_tab=15), b'n_tab', b'n_envs') and refused(call(n_tab=15, getup=0), b'n_tab', b'n_envs')
    for init, word in ((L.INIT_START, b'Start'), (L.INIT_RANDOM, b'Random'), (L.INIT_HYBRID, b'Hybrid')):
        for name in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'num_frames', 'dt', 'length_starts', 'dof_body_ids'):
            assert refused(call(**{name: None}, state_init=init), word, b'clip tensors'), (init, name)
        assert refused(call(cdf=None, state_init=init), word, b'cdf') and refused(call(n_clips=0, state_init=init), b'cdf')
    for name in ('env_ids_out', 'kind_out', 'motion_ids_out', 'motion_times_out', 'src_rows_out'):
        assert refused(call(**{name: None}), b'plan export', b'4 of 5'), name
    for name in ('hybrid_init_prob', 'recovery_episode_prob', 'fall_init_prob'):
        for v in (-0.1, 1.5, float('nan')):
            assert refused(call(**{name: v}), name.encode()), (name, v)
    assert refused(call(recovery_steps=-1), b'recovery_steps')
    # the limits amp_reset checks
    for name in ('root_states', 'dof_pos', 'dof_vel', 'body_pos', 'body_rot', 'body_vel', 'body_ang_vel', 'hist', 'dof_offsets',
                 'key_body_ids'):
        assert refused(call(**{name: None}), b'null'), name
    assert refused(call(n_steps=0), b'n_steps') and refused(call(n_steps=65), b'n_steps')
    assert refused(call(n_envs=0), b'envs') and refused(call(n_bodies=0), b'bodies')
    assert refused(call(n_key=33), b'key bodies') and refused(call(n_joints=33), b'joints')
    assert refused(call(dof_stride=3), b'dof_stride') and refused(call(dof_stride=0), b'dof_stride')
    assert refused(call(ld_root=12), b'strides') and refused(call(ld_dof=30), b'strides')
    assert refused(call(ld_dof=60, dof_stride=2), b'strides')
    bad_offs = (ctypes.c_int32 * 14)(0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 29, 31)
    assert refused(call(dof_offsets=bad_offs), b'dofs')
    bad_keys = (ctypes.c_int32 * 6)(5, 10, 13, 17, 6, 9)
    assert refused(call(key_body_ids=bad_keys), b'key body')
    bad_bodies = (ctypes.c_int32 * 13)(1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 17)
    assert refused(call(dof_body_ids=bad_bodies), b'joint 12')
    big = (ctypes.c_int32 * 33)(*range(0, 97, 3))                              # 32 joints of 3 dofs, 32 key bodies, 64 slots
    many = (ctypes.c_int32 * 32)(*range(32))
    assert refused(call(dof_offsets=big, n_joints=32, dof_body_ids=many, key_body_ids=many, n_key=32, n_bodies=33, ld_dof=96,
                        n_steps=64), b'staging tile')
    with pytest.raises(L.AseHipError):
        L.check(-1, 'amp_reset_due')


def test_torch_op_is_registered():
    import ase_amd.ops  # noqa: F401
    assert hasattr(torch.ops.ase_hip, 'amp_reset_due')
    schema = str(torch.ops.ase_hip.amp_reset_due.default._schema)
    for name in ('root_states', 'dof_pos', 'dof_vel', 'hist', 'reset_buf', 'rng_state', 'progress_buf', 'terminate_buf',
                 'recovery_counter', 'env_ids_out', 'kind_out', 'motion_ids_out', 'motion_times_out', 'src_rows_out'):
        assert f'!)? {name}' in schema or f'!) {name}' in schema, (name, schema)
    assert 'Tensor body_pos' in schema and schema.endswith('-> ()') and 'amp_reset_due(' in ase_amd.ops.__doc__
