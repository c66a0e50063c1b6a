"""HumanoidAMP / HumanoidAMPGetup resets without a GPU: the torch restatement and ``HumanoidAMPTensors.apply_reset``
against the reference's recorded buffers, ``draw_reset``, the recovery counter and the PD helpers, the host-side operand checks
of ``ase_hip_amp_reset``, and the conditions the generator of tests/golden/amp_reset.pt promises, re-checked on the file."""
import ctypes
import os

import pytest
import torch

from ase_amd import lib as L
from ase_amd.amp_env import HumanoidAMPTensors, action_to_pd_targets, pd_action_offset_scale
from ase_amd.motion_lib import DeviceMotionLib
from tests import emu_amp_reset as E

SCENARIOS = ['default', 'start', 'random', 'hybrid', 'getup']


@pytest.fixture(scope='module')
def GC():
    return E.load_fixture()


def _tensors(G, clips, sc=None, state_init='Random', getup=False, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    ml = DeviceMotionLib.from_arrays(clips, None, 'cpu', generator=g)
    if sc is not None:
        state_init, getup = sc['state_init'], sc['getup']
    if getup:
        kw.update(recovery_episode_prob=G['recovery_episode_prob'], recovery_steps=G['recovery_steps'], fall_init_prob=G['fall_init_prob'])
    at = HumanoidAMPTensors(E.EmuAmpReset(), ml, G['num_envs'], num_amp_obs_steps=G['num_amp_obs_steps'], dt=G['dt'],
                            state_init=state_init, hybrid_init_prob=G['hybrid_init_prob'], local_root_obs=G['local_root_obs'],
                            root_height_obs=G['root_height_obs'], generator=g, **kw)
    init, fall = E.tables(G)
    at.set_initial_state(*init)
    if getup:
        at.set_fall_states(*fall)
    return at


def _apply(G, clips, sc):
    at = _tensors(G, clips, sc)
    s, bufs = E.prefill(G)
    at.amp_obs_buf.copy_(s.pop('amp_obs_buf'))
    if sc['getup']:
        at.recovery_counter.copy_(bufs['recovery_counter'])
    at.apply_reset(s, E.plan_of(G, sc), bufs['progress_buf'], bufs['reset_buf'], bufs['terminate_buf'])
    s['amp_obs_buf'] = at.amp_obs_buf
    return at, s, bufs


def _rows(sc, kind):
    p = sc['plan']
    return [e for e, k in zip(p['env_ids'], p['kind']) if k == kind]


@pytest.mark.parametrize('name', SCENARIOS)
def test_restatement_reproduces_the_reference_buffers(GC, name):
    G, clips = GC
    sc = G['scenarios'][name]
    at, s, bufs = _apply(G, clips, sc)
    want, ids = sc['f32'], sc['plan']['env_ids']
    before, _ = E.prefill(G)
    init, fall = E.tables(G)
    table = tuple(torch.cat([a, b]) for a, b in zip(init, fall))
    others = [e for e in range(G['num_envs']) if e not in ids]
    rows0, rows1, rows2 = _rows(sc, L.RESET_FRAME), _rows(sc, L.RESET_TABLE), _rows(sc, L.RESET_MOTION)
    hist = s['amp_obs_buf']
    # -- bitwise: what is copied or not touched
    for k in ('humanoid_root_states', 'dof_pos', 'dof_vel'):
        assert torch.equal(s[k][others + rows0], before[k][others + rows0]), k           # rows outside the plan, recovery rows
        assert torch.equal(s[k][rows1], want[k][rows1]), k                                  # table rows
    src = [r for r, k in zip(sc['plan']['src_rows'], sc['plan']['kind']) if k == L.RESET_TABLE]
    assert torch.equal(s['humanoid_root_states'][rows1], table[0][src]) and torch.equal(s['dof_pos'][rows1], table[1][src])
    assert torch.equal(s['humanoid_root_states'][rows2, 7:13], want['humanoid_root_states'][rows2, 7:13])      # velocities: clip rows
    assert torch.equal(s['dof_vel'][rows2], want['dof_vel'][rows2])
    assert torch.equal(hist[others], before['amp_obs_buf'][others])
    assert torch.equal(hist[rows0, 1:], before['amp_obs_buf'][rows0, 1:])                   # a recovery row keeps its history
    assert torch.equal(hist[rows1, 1:], hist[rows1, 0:1].expand(-1, hist.shape[1] - 1, -1))  # default history = slot 0
    for k in ('progress_buf', 'reset_buf', 'terminate_buf'):
        assert torch.equal(bufs[k], want[k]), k
        assert not bufs[k][ids].any()
    if sc['getup']:
        assert torch.equal(at.recovery_counter, want['recovery_counter'])
        assert at.recovery_counter.dtype == torch.int32
    # -- within e_ref of the reference's f32 recording: the rest
    got = dict(s)
    ref = {'humanoid_root_states': want['humanoid_root_states'], 'dof_pos': want['dof_pos'], 'amp_obs_buf': hist.clone()}
    ref['amp_obs_buf'][ids] = want['amp_obs_rows']
    err = E.group_errors(got, ref, rows2, ids)
    print(name, {k: f'{v:.3g}' for k, v in err.items()}, 'e_ref', {k: f'{v:.3g}' for k, v in G['e_ref'].items()})
    for k, v in err.items():
        assert v <= G['e_ref'][k], (name, k, v)
    # ... and the f64 leg within the device bar
    err64 = E.group_errors(got, E.expected_f64(G, clips, sc), rows2, ids)
    for k, v in err64.items():
        assert v <= E.allowance(G, k), (name, k, v)


def test_frame_only_plan_touches_slot_zero_alone(GC):
    G, clips = GC
    at = _tensors(G, clips)
    s, _ = E.prefill(G)
    at.amp_obs_buf.copy_(s.pop('amp_obs_buf'))
    before = {k: v.clone() for k, v in s.items()}
    hist0 = at.amp_obs_buf.clone()
    ids = G['env_ids'][:7]
    at.compute_amp_observations(s, ids)
    for k in before:
        assert torch.equal(s[k], before[k]), k
    others = [e for e in range(G['num_envs']) if e not in ids]
    assert torch.equal(at.amp_obs_buf[others], hist0[others]) and torch.equal(at.amp_obs_buf[ids, 1:], hist0[ids, 1:])
    assert not torch.equal(at.amp_obs_buf[ids, 0], hist0[ids, 0])
    # the same frame as the whole-batch builder computes
    whole = _tensors(G, clips)
    whole.post_physics_step(s)
    # (torch's CPU kernels round sin / cos differently for different batch sizes: ulps, not bits; the device test asks for bits)
    assert float((at.amp_obs_buf[ids, 0] - whole.amp_obs_buf[ids, 0]).abs().max()) <= 2e-6


def test_out_of_range_ids_are_skipped(GC):
    G, clips = GC
    sc = G['scenarios']['hybrid']
    at = _tensors(G, clips, sc)
    s, _ = E.prefill(G)
    at.amp_obs_buf.copy_(s.pop('amp_obs_buf'))
    before = {k: v.clone() for k, v in s.items()}
    hist0 = at.amp_obs_buf.clone()
    p = E.plan_of(G, sc)
    p['env_ids'] = torch.where(torch.arange(p['env_ids'].numel()) % 2 == 0, G['num_envs'] + 5, -3).to(torch.int32)
    at._launch(s, p, L.RESET_HAS_TABLE | L.RESET_HAS_MOTION)
    assert all(torch.equal(s[k], before[k]) for k in before) and torch.equal(at.amp_obs_buf, hist0)


@pytest.mark.parametrize('state_init', ['Default', 'Start', 'Random', 'Hybrid'])
def test_draw_reset_partitions_the_rows(GC, state_init):
    G, clips = GC
    at = _tensors(G, clips, state_init=state_init, seed=3)
    ids = torch.tensor(G['env_ids'])
    plan = at.draw_reset(ids)
    assert set(plan) == {'env_ids', 'kind', 'motion_ids', 'motion_times', 'src_rows'}
    assert plan['env_ids'].dtype == plan['kind'].dtype == plan['motion_ids'].dtype == plan['src_rows'].dtype == torch.int32
    assert plan['motion_times'].dtype == torch.float32 and all(v.numel() == ids.numel() for v in plan.values())
    assert plan['env_ids'].tolist() == G['env_ids']                          # nothing lost, duplicated or reordered
    kind = plan['kind']
    if state_init == 'Default':
        assert (kind == L.RESET_TABLE).all() and plan['src_rows'].tolist() == G['env_ids']
    elif state_init == 'Start':
        assert (kind == L.RESET_MOTION).all() and not plan['motion_times'].any()
    elif state_init == 'Random':
        assert (kind == L.RESET_MOTION).all() and (plan['motion_times'] > 0).all()
        assert (plan['motion_times'] <= clips['lengths'][plan['motion_ids'].long()]).all()
        assert set(plan['motion_ids'].tolist()) == {0, 1}
    else:
        n1, n2 = int((kind == L.RESET_TABLE).sum()), int((kind == L.RESET_MOTION).sum())
        assert n1 + n2 == ids.numel() and n1 >= 4 and n2 >= 4
        t = kind == L.RESET_TABLE
        assert torch.equal(plan['src_rows'][t], plan['env_ids'][t]) and not plan['motion_times'][t].any()
    # reproducible under a seeded generator
    again = _tensors(G, clips, state_init=state_init, seed=3).draw_reset(ids)
    assert all(torch.equal(plan[k], again[k]) for k in plan)
    other = _tensors(G, clips, state_init=state_init, seed=4).draw_reset(ids)
    assert state_init in ('Default', 'Start') or not all(torch.equal(plan[k], other[k]) for k in plan)


def test_draw_reset_getup_split(GC):
    G, clips = GC
    N = G['num_envs']
    ids = torch.tensor(G['env_ids'])
    terminate = G['buffers']['terminate_buf']
    seen = {L.RESET_FRAME: 0, 'fall': 0, L.RESET_MOTION: 0}
    for seed in range(8):
        at = _tensors(G, clips, getup=True, seed=seed)
        plan = at.draw_reset(ids, terminate)
        assert plan['env_ids'].tolist() == G['env_ids']
        kind, src = plan['kind'], plan['src_rows']
        recovery, fall, ref = kind == L.RESET_FRAME, kind == L.RESET_TABLE, kind == L.RESET_MOTION
        assert int(recovery.sum() + fall.sum() + ref.sum()) == ids.numel()
        assert (terminate[ids][recovery] == 1).all()                        # humanoid_amp_getup.py:82-83
        assert ((src[fall] >= N) & (src[fall] < N + G['num_fall_states'])).all()
        seen[L.RESET_FRAME] += int(recovery.sum()); seen['fall'] += int(fall.sum()); seen[L.RESET_MOTION] += int(ref.sum())
        again = _tensors(G, clips, getup=True, seed=seed).draw_reset(ids, terminate)
        assert all(torch.equal(plan[k], again[k]) for k in plan)
        # nobody recovers when nothing terminated
        none = _tensors(G, clips, getup=True, seed=seed).draw_reset(ids, torch.zeros_like(terminate))
        assert not (none['kind'] == L.RESET_FRAME).any()
    assert all(v >= 8 for v in seen.values()), seen
    with pytest.raises(ValueError):
        _tensors(G, clips, getup=True).draw_reset(ids)                       # no terminate_buf


def test_reset_is_draw_plus_apply(GC):
    G, clips = GC
    ids = torch.tensor(G['env_ids'])
    a, b = _tensors(G, clips, state_init='Hybrid', seed=5), _tensors(G, clips, state_init='Hybrid', seed=5)
    sa, ba = E.prefill(G)
    sb, bb = E.prefill(G)
    for at, s in ((a, sa), (b, sb)):
        at.amp_obs_buf.copy_(s.pop('amp_obs_buf'))
    plan = a.reset(sa, ids, ba['progress_buf'], ba['reset_buf'], ba['terminate_buf'])
    b.apply_reset(sb, b.draw_reset(ids), bb['progress_buf'], bb['reset_buf'], bb['terminate_buf'])
    assert torch.equal(a.amp_obs_buf, b.amp_obs_buf) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not ba['progress_buf'][ids].any() and torch.equal(ba['progress_buf'], bb['progress_buf'])
    assert (plan['kind'] > 0).all()


def test_recovery_counter_and_mask(GC):
    G, clips = GC
    sc = G['scenarios']['getup']
    at, s, bufs = _apply(G, clips, sc)
    want = sc['f32']['recovery_counter']
    p = sc['plan']
    steps = G['recovery_steps']
    for e, k, src in zip(p['env_ids'], p['kind'], p['src_rows']):
        assert int(want[e]) == (steps if k == L.RESET_FRAME or (k == L.RESET_TABLE and src >= G['num_envs']) else 0)
    others = [e for e in range(G['num_envs']) if e not in p['env_ids']]
    assert torch.equal(at.recovery_counter[others], G['buffers']['recovery_counter'][others])
    # humanoid_amp_getup.py:136-142
    reset, term = torch.ones(G['num_envs'], dtype=torch.int64), torch.ones(G['num_envs'], dtype=torch.int64)
    at.mask_recovery(reset, term)
    rec = at.recovery_counter > 0
    assert torch.equal(reset, (~rec).long()) and torch.equal(term, (~rec).long()) and rec.any() and not rec.all()
    # humanoid_amp_getup.py:131-134
    c = at.recovery_counter.clone()
    for _ in range(3):
        at.pre_physics_step()
        c = torch.clamp_min(c - 1, 0)
        assert torch.equal(at.recovery_counter, c) and at.recovery_counter.dtype == torch.int32
    assert (at.recovery_counter[others] <= 1).all() and (at.recovery_counter >= 0).all()
    # without the get-up options there is no counter and the mask is the identity
    plain = _tensors(G, clips)
    assert plain.recovery_counter is None
    plain.pre_physics_step()
    assert plain.mask_recovery(reset, term)[0] is reset


def test_pd_helpers_match_the_reference(GC):
    G, _ = GC
    pd = G['pd']
    offs = E.load_fixture()[1]['dof_offsets']
    lower, upper = pd['dof_limits_lower'].clone(), pd['dof_limits_upper'].clone()
    offset, scale = pd_action_offset_scale(lower, upper, offs)
    assert torch.equal(offset, pd['pd_action_offset']) and torch.equal(scale, pd['pd_action_scale'])
    assert torch.equal(lower, pd['dof_limits_lower']) and torch.equal(upper, pd['dof_limits_upper'])       # the limits stay
    assert torch.equal(action_to_pd_targets(pd['actions'], offset, scale), pd['pd_targets'])
    assert float(scale.max()) == pytest.approx(3.14159265, abs=1e-6)          # a 3-dof joint takes the cap


def test_post_physics_step_then_reset_follows_the_reference_sequence(GC):
    """shift, current frame for everybody, then the reset rows (humanoid_amp.py:50-59,132-139)."""
    G, clips = GC
    sc = G['scenarios']['hybrid']
    at = _tensors(G, clips, sc)
    s, bufs = E.prefill(G)
    hist0 = s.pop('amp_obs_buf')
    at.amp_obs_buf.copy_(hist0)
    flat = at.post_physics_step(s)
    assert flat.shape == (G['num_envs'], at.get_num_amp_obs()) and flat.data_ptr() == at.amp_obs_buf.data_ptr()
    assert at.get_num_amp_obs() == G['num_amp_obs_steps'] * G['num_amp_obs_per_step']
    assert torch.equal(at.amp_obs_buf[:, 1:], hist0[:, :-1])
    stepped = at.amp_obs_buf.clone()
    at.apply_reset(s, E.plan_of(G, sc))
    ids = sc['plan']['env_ids']
    others = [e for e in range(G['num_envs']) if e not in ids]
    assert torch.equal(at.amp_obs_buf[others], stepped[others])
    # the reset rows do not depend on the history they had
    _, s2, _ = _apply(G, clips, sc)
    assert torch.equal(at.amp_obs_buf[ids], s2['amp_obs_buf'][ids])


def test_options_are_checked(GC):
    G, clips = GC
    ml = DeviceMotionLib.from_arrays(clips, None, 'cpu')
    with pytest.raises(ValueError):
        HumanoidAMPTensors(E.EmuAmpReset(), ml, 4, state_init='Sometimes')
    with pytest.raises(ValueError):
        HumanoidAMPTensors(E.EmuAmpReset(), ml, 4, recovery_steps=60)
    at = HumanoidAMPTensors(E.EmuAmpReset(), ml, 4, state_init='Default')
    with pytest.raises(ValueError):
        at.draw_reset([0, 1])                                                # no initial state
    with pytest.raises(ValueError):
        at.set_initial_state(torch.zeros(3, 13), torch.zeros(3, 31), torch.zeros(3, 31))
    with pytest.raises(ValueError):
        at.set_fall_states(torch.zeros(3, 13), torch.zeros(3, 31), torch.zeros(3, 31))
    assert at.amp_obs_buf.shape == (4, 10, 140) and at.get_num_amp_obs() == 1400


def test_entry_point_validates_operands_without_gpu():
    """The host-side checks of ase_hip_amp_reset run before any launch: NULL operands, sizes, table sizes of the kernel,
    the dof stride and operands missing for an announced kind are refused with the entry's name in the message."""
    lib = L.load()
    assert 'ase_hip_amp_reset' in L.SIGNATURES and L.ABI_VERSION == 9
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ase_hip_last_error()
    offs = (ctypes.c_int32 * 14)(0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 28, 31)
    bodies = (ctypes.c_int32 * 13)(1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16)
    keys = (ctypes.c_int32 * 6)(5, 10, 13, 16, 6, 9)

    def call(**kw):
        a = dict(gts=p, grs=p, lrs=p, grvs=p, gravs=p, dvs=p, n_bodies=17, lengths=p, num_frames=p, dt=p, length_starts=p,
                 dof_body_ids=bodies, dof_offsets=offs, n_joints=13, key_body_ids=keys, n_key=6, env_ids=p, kind=p, motion_ids=p,
                 motion_times=p, src_rows=p, n_ids=8, kinds=3, tab_root=p, tab_dof_pos=p, tab_dof_vel=p, n_tab=4, root_states=p,
                 ld_root=13, dof_pos=p, dof_vel=p, ld_dof=31, dof_stride=1, body_pos=p, body_rot=p, body_vel=p, body_ang_vel=p,
                 n_envs=16, local_root_obs=1, root_height_obs=1, env_dt=1.0 / 30.0, hist=p, n_steps=10, stream=None)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return lib.ase_hip_amp_reset(*a.values())

    for name in ('env_ids', 'kind', 'root_states', 'dof_pos', 'dof_vel', 'body_pos', 'body_rot', 'body_vel', 'body_ang_vel', 'hist',
                 'dof_offsets', 'key_body_ids'):
        assert call(**{name: None}) == -1 and b'amp_reset' in err() and b'null' in err(), name
    assert call(n_steps=0) == -1 and b'n_steps' in err()
    assert call(n_steps=65) == -1 and b'n_steps' in err()
    assert call(n_ids=-1) == -1 and call(n_envs=0) == -1 and call(n_bodies=0) == -1
    assert call(n_key=33) == -1 and b'key bodies' in err()
    assert call(n_joints=33) == -1 and b'joints' in err()
    assert call(dof_stride=3) == -1 and b'dof_stride' in err()
    assert call(dof_stride=0) == -1
    assert call(kinds=4) == -1 and b'kinds' in err()
    assert call(ld_root=12) == -1 and b'strides' in err()
    assert call(ld_dof=30) == -1
    # a null table / null clips only together with the host flag that says no row is of that kind
    for name in ('tab_root', 'tab_dof_pos', 'tab_dof_vel', 'src_rows'):
        assert call(**{name: None}) == -1 and b'kind 1' in err(), name
    assert call(n_tab=0) == -1
    for name in ('gts', 'grs', 'lrs', 'grvs', 'gravs', 'dvs', 'lengths', 'num_frames', 'dt', 'length_starts', 'dof_body_ids',
                 'motion_ids', 'motion_times'):
        assert call(**{name: None}) == -1 and b'kind 2' in err(), name
    bad_offs = (ctypes.c_int32 * 14)(0, 3, 6, 9, 10, 13, 16, 17, 20, 21, 24, 27, 29, 31)
    assert call(dof_offsets=bad_offs) == -1 and b'dofs' in err()
    bad_keys = (ctypes.c_int32 * 6)(5, 10, 13, 17, 6, 9)
    assert call(key_body_ids=bad_keys) == -1 and b'key body' in err()
    bad_bodies = (ctypes.c_int32 * 13)(1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 17)
    assert call(dof_body_ids=bad_bodies) == -1
    # an empty plan is valid and launches nothing - with and without the optional operands
    assert call(n_ids=0) == 0
    assert call(n_ids=0, kinds=0, tab_root=None, tab_dof_pos=None, tab_dof_vel=None, src_rows=None, n_tab=0, gts=None, grs=None,
                lrs=None, grvs=None, gravs=None, dvs=None, lengths=None, num_frames=None, dt=None, length_starts=None,
                dof_body_ids=None, motion_ids=None, motion_times=None) == 0
    assert call(n_ids=0, ld_dof=61, dof_stride=2) == 0 and call(n_ids=0, ld_dof=60, dof_stride=2) == -1
    with pytest.raises(L.AseHipError):
        L.check(-1, 'amp_reset')


def test_torch_op_is_registered():
    import ase_amd.ops  # noqa: F401
    assert hasattr(torch.ops.ase_hip, 'amp_reset')
    schema = str(torch.ops.ase_hip.amp_reset.default._schema)
    assert 'Tensor(a0!) root_states' in schema and 'Tensor(a3!) hist' in schema and schema.endswith('-> ()')


# ---- the generator's promises, re-checked on the committed file --------------------------------------------------------
def test_fixture_keeps_its_conditions(GC):
    G, clips = GC
    N, S = G['num_envs'], G['num_amp_obs_steps']
    assert 32 <= N <= 48 and S == 10 and G['num_amp_obs_per_step'] == 140 and G['margin'] == 1e-3
    ids = G['env_ids']
    assert len(set(ids)) == len(ids) and N // 2 < len(ids) < N and ids != sorted(ids)          # most, not all, shuffled
    assert set(G['scenarios']) == set(SCENARIOS)
    fall_root = G['tables']['fall'][0]
    assert len({tuple(r.tolist()) for r in fall_root}) == fall_root.shape[0]                   # pairwise distinct
    nf, ln = clips['num_frames'].double(), clips['lengths'].double()
    for name, sc in G['scenarios'].items():
        p = sc['plan']
        assert p['env_ids'] == ids
        worst, negative = 1.0, 0
        for i, k in enumerate(p['kind']):
            if k != L.RESET_MOTION:
                continue
            m = p['motion_ids'][i]
            t = p['motion_times'][i].double() + (-G['dt']) * torch.arange(0, S).double()
            negative += bool((t < 0).any())
            phase = t / ln[m]
            pos = (phase * (nf[m] - 1))[(phase > 0) & (phase < 1)]
            if pos.numel():
                worst = min(worst, float((pos - pos.round()).abs().min()))
        assert worst >= G['margin'], (name, worst)
        assert worst == sc['frame_margin'] and negative == sc['negative_time_rows']
        g = sc['groups']
        assert g == {'default': sum(k == 1 and s < N for k, s in zip(p['kind'], p['src_rows'])), 'ref': p['kind'].count(2),
                     'fall': sum(k == 1 and s >= N for k, s in zip(p['kind'], p['src_rows'])), 'recovery': p['kind'].count(0)}
        if name == 'hybrid':
            assert min(g['default'], g['ref']) >= 4
        if name == 'getup':
            assert min(g['recovery'], g['fall'], g['ref']) >= 4
        if name == 'random':
            assert negative >= 3
        if name == 'start':
            assert not p['motion_times'].any()
    # the allowance is the reference's own error, capped
    caps = {'root': 1e-4, 'dof_pos': 1e-4, 'frame0': 1e-4, 'hist': 5e-4}
    assert G['e_ref_max'] == caps
    worst = {k: 0.0 for k in caps}
    for name, sc in G['scenarios'].items():
        p = sc['plan']
        want = sc['f32']
        ref = E.expected_f64(G, clips, sc)
        got = {'humanoid_root_states': want['humanoid_root_states'], 'dof_pos': want['dof_pos'], 'amp_obs_buf': ref['amp_obs_buf'].clone()}
        got['amp_obs_buf'][p['env_ids']] = want['amp_obs_rows'].double()
        for k, v in E.group_errors(got, ref, _rows(sc, L.RESET_MOTION), p['env_ids']).items():
            worst[k] = max(worst[k], v)
    for k in caps:
        assert worst[k] == pytest.approx(G['e_ref'][k], rel=1e-6, abs=1e-12) and 0 < G['e_ref'][k] <= caps[k], (k, worst[k], G['e_ref'][k])
    assert os.path.getsize(os.path.join(E.GOLDEN, 'amp_reset.pt')) < 1024 * 1024
