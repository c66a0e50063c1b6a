"""HumanoidAMP / HumanoidAMPGetup resets on the MI355X: ``ase_hip_amp_reset`` through ``HipBackend``,
``HumanoidAMPTensors`` and ``torch.ops.ase_hip.amp_reset`` against tests/golden/amp_reset.pt - floats within 2 e_ref + 1e-7 of
the f64 result, copied quantities and everything outside the plan bitwise."""
import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd import lib as L
from ase_amd.amp_env import HumanoidAMPTensors
from ase_amd.motion_lib import DeviceMotionLib
from tests import emu_amp_reset as E

pytestmark = pytest.mark.gpu

SCENARIOS = ['default', 'start', 'random', 'hybrid', 'getup']
DEV = 'cuda:0'
STATE_KEYS = ('humanoid_root_states', 'dof_pos', 'dof_vel')


@pytest.fixture(scope='module')
def GC():
    return E.load_fixture()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(DEV)


def _tensors(be, G, clips, sc=None, state_init='Random', getup=False, seed=0, steps=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ml = DeviceMotionLib.from_arrays(clips, be, DEV, generator=g)
    kw = {}
    if sc is not None:
        state_init, getup = sc['state_init'], sc['getup']
    if getup:
        kw.update(recovery_episode_prob=G['recovery_episode_prob'], recovery_steps=G['recovery_steps'], fall_init_prob=G['fall_init_prob'])
    at = HumanoidAMPTensors(be, ml, G['num_envs'], num_amp_obs_steps=steps or G['num_amp_obs_steps'], dt=G['dt'], state_init=state_init,
                            hybrid_init_prob=G['hybrid_init_prob'], local_root_obs=G['local_root_obs'],
                            root_height_obs=G['root_height_obs'], generator=g, **kw)
    init, fall = E.tables(G, device=DEV)
    at.set_initial_state(*init)
    if getup:
        at.set_fall_states(*fall)
    return at


def _start(be, G, clips, sc=None, **kw):
    at = _tensors(be, G, clips, sc, **kw)
    s, bufs = E.prefill(G, device=DEV)
    s.pop('amp_obs_buf')
    at.amp_obs_buf.copy_(E.hist_pattern(*at.amp_obs_buf.shape))
    if at.getup:
        at.recovery_counter.copy_(bufs['recovery_counter'])
    return at, s, bufs


def _rows(sc, kind):
    p = sc['plan']
    return [e for e, k in zip(p['env_ids'], p['kind']) if k == kind]


def _check_scenario(G, clips, sc, s, hist, what):
    """State and history of a scenario after the reset: floats against f64, copies and untouched rows bitwise."""
    ids = sc['plan']['env_ids']
    before, _ = E.prefill(G)
    init, fall = E.tables(G)
    table = tuple(torch.cat([a, b]) for a, b in zip(init, fall))
    others = [e for e in range(G['num_envs']) if e not in ids]
    rows0, rows1, rows2 = _rows(sc, L.RESET_FRAME), _rows(sc, L.RESET_TABLE), _rows(sc, L.RESET_MOTION)
    got = {k: s[k].cpu() for k in STATE_KEYS}
    got['amp_obs_buf'] = hist.cpu()
    want = sc['f32']
    h = got['amp_obs_buf']
    for k in STATE_KEYS:
        assert torch.equal(got[k][others + rows0], before[k][others + rows0]), (what, k)
    src = [r for r, k in zip(sc['plan']['src_rows'], sc['plan']['kind']) if k == L.RESET_TABLE]
    for k, t in zip(STATE_KEYS, table):
        assert torch.equal(got[k][rows1], t[src]), (what, k)
    assert torch.equal(got['humanoid_root_states'][rows2, 7:13], want['humanoid_root_states'][rows2, 7:13]), what     # clip rows
    assert torch.equal(got['dof_vel'][rows2], want['dof_vel'][rows2]), what
    assert torch.equal(h[others], before['amp_obs_buf'][others]), what
    assert torch.equal(h[rows0, 1:], before['amp_obs_buf'][rows0, 1:]), what
    assert torch.equal(h[rows1, 1:], h[rows1, 0:1].expand(-1, h.shape[1] - 1, -1)), what
    od = 13 + 6 * (len(clips['dof_offsets']) - 1)
    assert torch.equal(h[ids, 0, od:od + G['num_dof']], got['dof_vel'][ids]), what                # the frame's dof velocities: a copy
    err = E.group_errors(got, E.expected_f64(G, clips, sc), rows2, ids)
    print(what, 'max |hip - f64|', {k: f'{v:.3g}' for k, v in err.items()}, 'allowance', {k: f'{E.allowance(G, k):.3g}' for k in err})
    for k, v in err.items():
        assert v <= E.allowance(G, k), (what, k, v, E.allowance(G, k))
    return got


@pytest.mark.parametrize('name', SCENARIOS)
def test_scenarios_match_the_reference(be, GC, name):
    G, clips = GC
    sc = G['scenarios'][name]
    at, s, bufs = _start(be, G, clips, sc)
    at.apply_reset(s, E.plan_of(G, sc, DEV), bufs['progress_buf'], bufs['reset_buf'], bufs['terminate_buf'])
    torch.cuda.synchronize()
    _check_scenario(G, clips, sc, s, at.amp_obs_buf, name)
    for k in ('progress_buf', 'reset_buf', 'terminate_buf'):
        assert torch.equal(bufs[k].cpu(), sc['f32'][k]), k
    if sc['getup']:
        assert torch.equal(at.recovery_counter.cpu(), sc['f32']['recovery_counter'])
    for k in ('rigid_body_pos', 'rigid_body_rot', 'rigid_body_vel', 'rigid_body_ang_vel'):       # inputs stay inputs
        assert torch.equal(s[k].cpu(), G['inputs'][k]), k


def test_out_of_range_ids_and_unknown_kinds_are_skipped(be, GC):
    G, clips = GC
    sc = G['scenarios']['hybrid']
    at, s, _ = _start(be, G, clips, sc)
    before = {k: v.clone() for k, v in s.items()}
    hist0 = at.amp_obs_buf.clone()
    p = E.plan_of(G, sc, DEV)
    n = p['env_ids'].numel()
    odd = torch.arange(n, device=DEV) % 2 == 1
    bad = p['env_ids'].clone()
    bad[odd] = torch.where(torch.arange(n, device=DEV) % 4 == 1, G['num_envs'], -1).to(torch.int32)[odd]
    q = dict(p, env_ids=bad)
    q['kind'] = p['kind'].clone()
    q['kind'][0] = 3                                           # row 0 (a valid id): not a kind -> skipped as well
    at._launch(s, q, L.RESET_HAS_TABLE | L.RESET_HAS_MOTION)
    torch.cuda.synchronize()
    live = [e for i, e in enumerate(sc['plan']['env_ids']) if i % 2 == 0 and i != 0]
    dead = [e for e in range(G['num_envs']) if e not in live]
    for k in STATE_KEYS:
        assert torch.equal(s[k][dead], before[k][dead]), k
    assert torch.equal(at.amp_obs_buf[dead], hist0[dead])
    # the rows that stayed are the rows of the full plan
    full, s2, _ = _start(be, G, clips, sc)
    full._launch(s2, p, L.RESET_HAS_TABLE | L.RESET_HAS_MOTION)
    torch.cuda.synchronize()
    assert torch.equal(at.amp_obs_buf[live], full.amp_obs_buf[live]) and all(torch.equal(s[k][live], s2[k][live]) for k in STATE_KEYS)
    # a kind that the host mask does not announce is skipped too (its operands may be missing)
    at3, s3, _ = _start(be, G, clips, sc)
    at3._launch(s3, {'env_ids': p['env_ids'], 'kind': p['kind']}, 0)
    torch.cuda.synchronize()
    assert all(torch.equal(s3[k], before[k]) for k in STATE_KEYS) and torch.equal(at3.amp_obs_buf, hist0)


def test_strided_simulator_tensors(be, GC):
    """dof_stride = 2 on the interleaved [N, D, 2] dof state and ld_root > 13: the contiguous result, gaps untouched."""
    G, clips = GC
    sc = G['scenarios']['getup']
    N, D = G['num_envs'], G['num_dof']
    ref, s, _ = _start(be, G, clips, sc)
    ref.apply_reset(s, E.plan_of(G, sc, DEV))
    at, t, _ = _start(be, G, clips, sc)
    dof_state = torch.full((N, D + 2, 2), 7.25, device=DEV)    # two spare dofs per row: ld_dof = 2 D + 4
    dof_state[:, :D, 0], dof_state[:, :D, 1] = t['dof_pos'], t['dof_vel']
    actors = torch.full((N, 3, 13), -3.5, device=DEV)          # the humanoid is actor 0 of 3 per environment: ld_root = 39
    actors[:, 0] = t['humanoid_root_states']
    t.update(dof_pos=dof_state[:, :D, 0], dof_vel=dof_state[:, :D, 1], humanoid_root_states=actors[:, 0])
    assert t['dof_pos'].stride() == (2 * D + 4, 2) and t['humanoid_root_states'].stride() == (39, 1)
    at.apply_reset(t, E.plan_of(G, sc, DEV))
    torch.cuda.synchronize()
    for k in STATE_KEYS:
        assert torch.equal(t[k], s[k]), k
    assert torch.equal(at.amp_obs_buf, ref.amp_obs_buf)
    assert (dof_state[:, D:] == 7.25).all() and (actors[:, 1:] == -3.5).all()


@pytest.mark.parametrize('S', [10, 1, 3, 40])
def test_motion_rows_equal_the_existing_entries_composed(be, GC, S):
    """kind 2 = be.motion_state, then be.build_amp_obs(shift=False), then indexed writes - for the fixture's 10 history slots,
    none, a few, and more slots than a block's usual share of items (a row then has a block of its own)."""
    G, clips = GC
    sc = G['scenarios']['random']
    at, s, _ = _start(be, G, clips, sc, steps=S)
    p = E.plan_of(G, sc, DEV)
    at.apply_reset(s, p)
    c = at._motion_lib.clips
    F, n = G['num_amp_obs_per_step'], p['env_ids'].numel()
    ids = p['env_ids'].long()
    _, t, _ = _start(be, G, clips, sc, steps=S)
    rp, rq, dp, rv, rw, dv, _ = be.motion_state(c, p['motion_ids'], p['motion_times'])
    t['humanoid_root_states'][ids] = torch.cat([rp, rq, rv, rw], -1)
    t['dof_pos'][ids], t['dof_vel'][ids] = dp, dv
    hist = E.hist_pattern(G['num_envs'], S, F).to(DEV)
    cur = torch.zeros(n, 1, F, device=DEV)
    kb = c['key_body_ids']
    be.build_amp_obs(t['rigid_body_pos'][ids][:, 0].contiguous(), t['rigid_body_rot'][ids][:, 0].contiguous(),
                     t['rigid_body_vel'][ids][:, 0].contiguous(), t['rigid_body_ang_vel'][ids][:, 0].contiguous(), t['dof_pos'][ids],
                     t['dof_vel'][ids], t['rigid_body_pos'][ids][:, kb].contiguous(), c['dof_offsets'], G['local_root_obs'],
                     G['root_height_obs'], cur, shift=False)
    hist[ids, 0] = cur[:, 0]
    if S > 1:
        steps = -G['dt'] * (torch.arange(0, S - 1, device=DEV) + 1)
        times = (p['motion_times'].unsqueeze(-1) + steps).reshape(-1)
        mids = p['motion_ids'].view(-1, 1).expand(n, S - 1).reshape(-1).contiguous()
        st = be.motion_state(c, mids, times)
        past = torch.zeros(n * (S - 1), 1, F, device=DEV)
        be.build_amp_obs(st[0], st[1], st[3], st[4], st[2], st[5], st[6], c['dof_offsets'], G['local_root_obs'], G['root_height_obs'],
                         past, shift=False)
        hist[ids, 1:] = past.view(n, S - 1, F)
    torch.cuda.synchronize()
    rows = sc['plan']['env_ids']
    got = {k: s[k] for k in STATE_KEYS}
    got['amp_obs_buf'] = at.amp_obs_buf
    want = {k: t[k] for k in STATE_KEYS}
    want['amp_obs_buf'] = hist
    err = E.group_errors(got, want, rows, rows)
    print('fused against composed', {k: f'{v:.3g}' for k, v in err.items()})
    for k, v in err.items():
        assert v <= E.allowance(G, k), (k, v)
    # the same device functions run in both: the state rows and the current frame are the same bits
    assert all(torch.equal(got[k], want[k]) for k in STATE_KEYS) and torch.equal(got['amp_obs_buf'][:, 0], hist[:, 0])
    others = [e for e in range(G['num_envs']) if e not in rows]
    assert torch.equal(at.amp_obs_buf[others], E.hist_pattern(G['num_envs'], S, F).to(DEV)[others])


def test_frame_only_rows_equal_the_whole_batch_builder(be, GC):
    G, clips = GC
    at, s, _ = _start(be, G, clips)
    hist0 = at.amp_obs_buf.clone()
    before = {k: v.clone() for k, v in s.items()}
    ids = G['env_ids'][:9]
    at.compute_amp_observations(s, ids)
    whole, s2, _ = _start(be, G, clips)
    flat = whole.post_physics_step(s2)
    torch.cuda.synchronize()
    assert flat.shape == (G['num_envs'], whole.get_num_amp_obs())
    others = [e for e in range(G['num_envs']) if e not in ids]
    assert torch.equal(at.amp_obs_buf[ids, 0], whole.amp_obs_buf[ids, 0])                    # bits
    assert torch.equal(at.amp_obs_buf[ids, 1:], hist0[ids, 1:]) and torch.equal(at.amp_obs_buf[others], hist0[others])
    assert all(torch.equal(s[k], before[k]) for k in before)
    assert torch.equal(whole.amp_obs_buf[:, 1:], hist0[:, :-1])


def test_apply_reset_in_a_launch_program_follows_the_plan(be, GC):
    """Recorded once; the plan's tensors are read at replay time."""
    G, clips = GC
    sc_a, sc_b = G['scenarios']['getup'], G['scenarios']['random']
    at, s, bufs = _start(be, G, clips, sc_a)
    plan = E.plan_of(G, sc_a, DEV)
    s0 = {k: v.clone() for k, v in s.items()}
    hist0, counter0 = at.amp_obs_buf.clone(), at.recovery_counter.clone()
    prog = be.prog_create()
    be.prog_begin(prog)
    at.apply_reset(s, plan, bufs['progress_buf'], bufs['reset_buf'], bufs['terminate_buf'])
    be.prog_end(prog)
    torch.cuda.synchronize()
    assert be.prog_size(prog) >= 1
    assert torch.equal(at.amp_obs_buf, hist0) and all(torch.equal(s[k], s0[k]) for k in s0)    # recorded, not executed
    assert bufs['progress_buf'].all()
    be.prog_launch(prog)
    torch.cuda.synchronize()
    _check_scenario(G, clips, sc_a, s, at.amp_obs_buf, 'replay, recorded plan')
    assert torch.equal(at.recovery_counter.cpu(), sc_a['f32']['recovery_counter'])
    assert torch.equal(bufs['progress_buf'].cpu(), sc_a['f32']['progress_buf'])
    # new contents in place (another draw, its rows in reverse order: every row now names another environment, motion and
    # time), buffers back to the start, replay
    for k, v in E.plan_of(G, sc_b, DEV).items():
        plan[k].copy_(v.flip(0))
    assert plan['env_ids'].tolist() == sc_a['plan']['env_ids'][::-1]
    for k in s0:
        s[k].copy_(s0[k])
    at.amp_obs_buf.copy_(hist0)
    at.recovery_counter.copy_(counter0)
    be.prog_launch(prog)
    torch.cuda.synchronize()
    _check_scenario(G, clips, sc_b, s, at.amp_obs_buf, 'replay, rewritten plan')
    assert not at.recovery_counter[plan['env_ids'].long()].any()                               # motion rows: counter 0
    be.prog_destroy(prog)


def test_torch_op_equals_the_backend_call(be, GC):
    G, clips = GC
    sc = G['scenarios']['getup']
    at, s, _ = _start(be, G, clips, sc)
    p = E.plan_of(G, sc, DEV)
    at.apply_reset(s, p)
    other, t, _ = _start(be, G, clips, sc)
    c, tab = other._motion_lib.clips, other._table
    out = torch.ops.ase_hip.amp_reset(t['humanoid_root_states'], t['dof_pos'], t['dof_vel'], other.amp_obs_buf, t['rigid_body_pos'],
                                      t['rigid_body_rot'], t['rigid_body_vel'], t['rigid_body_ang_vel'], p['env_ids'], p['kind'],
                                      p['motion_ids'], p['motion_times'], p['src_rows'], c['gts'], c['grs'], c['lrs'], c['grvs'],
                                      c['gravs'], c['dvs'], c['lengths'], c['num_frames'], c['dt'], c['length_starts'], tab[0], tab[1],
                                      tab[2], c['dof_body_ids'], c['dof_offsets'], c['key_body_ids'], G['local_root_obs'],
                                      G['root_height_obs'], G['dt'])
    torch.cuda.synchronize()
    assert out is None
    assert torch.equal(other.amp_obs_buf, at.amp_obs_buf) and all(torch.equal(t[k], s[k]) for k in STATE_KEYS)
    # frame-only rows need neither clips nor a table
    hist = other.amp_obs_buf.clone()
    ids = p['env_ids'][:5].contiguous()
    t['dof_pos'].mul_(0.5)
    torch.ops.ase_hip.amp_reset(t['humanoid_root_states'], t['dof_pos'], t['dof_vel'], other.amp_obs_buf, t['rigid_body_pos'],
                                t['rigid_body_rot'], t['rigid_body_vel'], t['rigid_body_ang_vel'], ids, torch.zeros_like(ids), None, None,
                                None, None, None, None, None, None, None, None, None, None, None, None, None, None, c['dof_body_ids'],
                                c['dof_offsets'], c['key_body_ids'], G['local_root_obs'], G['root_height_obs'], G['dt'])
    torch.cuda.synchronize()
    assert torch.equal(other.amp_obs_buf[:, 1:], hist[:, 1:]) and not torch.equal(other.amp_obs_buf[ids.long(), 0], hist[ids.long(), 0])
    with pytest.raises(RuntimeError):
        torch.ops.ase_hip.amp_reset(t['humanoid_root_states'], t['dof_pos'], t['dof_vel'], other.amp_obs_buf, t['rigid_body_pos'],
                                    t['rigid_body_rot'], t['rigid_body_vel'], t['rigid_body_ang_vel'], ids, torch.zeros_like(ids), None,
                                    None, None, c['gts'], None, None, None, None, None, None, None, None, None, None, None, None,
                                    c['dof_body_ids'], c['dof_offsets'], c['key_body_ids'], True, True, G['dt'])


def test_post_physics_step_then_reset_follows_the_reference_sequence(be, GC):
    """shift, current frame for everybody, then the reset rows (humanoid_amp.py:50-59,132-139) of a scenario."""
    G, clips = GC
    sc = G['scenarios']['hybrid']
    at, s, bufs = _start(be, G, clips, sc)
    hist0 = at.amp_obs_buf.clone()
    at.post_physics_step(s)
    stepped = at.amp_obs_buf.clone()
    at.apply_reset(s, E.plan_of(G, sc, DEV), bufs['progress_buf'], bufs['reset_buf'], bufs['terminate_buf'])
    torch.cuda.synchronize()
    ids = sc['plan']['env_ids']
    others = [e for e in range(G['num_envs']) if e not in ids]
    assert torch.equal(stepped[:, 1:], hist0[:, :-1])
    assert torch.equal(at.amp_obs_buf[others], stepped[others])                                # not reset: shifted + current frame
    # the reset rows are the scenario's, whatever history they had: compare them on the scenario's own start
    h = E.hist_pattern(G['num_envs'], G['num_amp_obs_steps'], G['num_amp_obs_per_step'])
    h[ids] = at.amp_obs_buf[ids].cpu()
    _check_scenario(G, clips, sc, s, h, 'post_physics_step + reset')
    # reset() = draw + apply, on the device generator
    a, sa, ba = _start(be, G, clips, state_init='Hybrid', seed=11)
    b, sb, _ = _start(be, G, clips, state_init='Hybrid', seed=11)
    ids_t = torch.tensor(ids, device=DEV)
    plan = a.reset(sa, ids_t, ba['progress_buf'], ba['reset_buf'], ba['terminate_buf'])
    b.apply_reset(sb, b.draw_reset(ids_t))
    torch.cuda.synchronize()
    assert torch.equal(a.amp_obs_buf, b.amp_obs_buf) and all(torch.equal(sa[k], sb[k]) for k in STATE_KEYS)
    assert set(plan['kind'].tolist()) == {L.RESET_TABLE, L.RESET_MOTION} and not ba['progress_buf'][ids_t].any()
