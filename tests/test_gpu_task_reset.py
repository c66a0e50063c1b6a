"""Target resets of the four tasks on the MI355X: ``ase_hip_task_reset`` through ``HipBackend``,
``HumanoidTensors`` and ``torch.ops.ase_hip.task_reset`` against tests/golden/task_reset.pt - floats within 2 e_ref + 1e-7 of the
f64 result, change steps, constants, device draws against passed-in draws and everything outside the selected rows bitwise.

Shapes beyond the fixture have no recorded e_ref; there the allowance takes the cap the generator holds every e_ref to, 16 f32
roundings of the group's largest output (scripts/make_golden_task_reset.py), in its place: 2 * 16 * 2^-24 * max |f64| + 1e-7."""
import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd import lib as L
from ase_amd.env_tensors import HumanoidTensors
from tests import emu_task_reset as E

pytestmark = pytest.mark.gpu

SCENARIOS = ('heading', 'heading_fixed', 'location', 'reach', 'strike')
TIMED = ('heading', 'location', 'reach')                 # the tasks with change steps
DEV = 'cuda:0'
SEED = (1 << 33) + 12345                                  # above 2^32: both key words of the stream are in use
OFFSETS = (0, (1 << 32) + 7)


@pytest.fixture(scope='module')
def G():
    return E.load_fixture()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(DEV)


def _rng(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _ids(ids):
    return torch.as_tensor(ids, dtype=torch.int32, device=DEV)


def _cpu(outs):
    return {g: v.cpu() for g, v in outs.items()}


def _equal(a, b):
    return set(a) == set(b) and all(torch.equal(a[g], b[g]) for g in a)


def _case(n, task, seed=5):
    """A state of n environments for shapes beyond the fixture: (G-like dict, scenario-like dict of the default parameters)."""
    g = torch.Generator().manual_seed(seed + n)
    root = torch.randn(n, 13, generator=g)
    root[:, 3:7] = root[:, 3:7] / root[:, 3:7].norm(dim=-1, keepdim=True)
    return {'num_envs': n, 'root_states': root, 'progress_buf': torch.randint(0, 300, (n,), generator=g)}


def _check_against_f64(task, got, f64, before, ids, bar, what):
    """Floats of the rows ids within bar(group) of f64, the exact groups equal, every other row the prefill."""
    n = before[next(iter(before))].shape[0]
    others = [e for e in range(n) if e not in ids]
    for g, v in got.items():
        assert torch.equal(v[others], before[g][others]), (what, g, 'a row outside the selection changed')
        if g in E.FLOAT_GROUPS[task]:
            err = float((v[ids].double() - f64[g][ids]).abs().max()) if ids else 0.0
            print(f'{what}: max |hip - f64| {g} {err:.3g} (allowed {bar(g):.3g})')
            assert err <= bar(g), (what, g, err, bar(g))
        else:
            assert torch.equal(v[ids], f64[g][ids].to(v.dtype)), (what, g)


# ---- 1. passed-in draws against the recording ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SCENARIOS)
def test_passed_in_draws_match_the_recording(be, G, name):
    sc = G['scenarios'][name]
    task, ids = sc['task'], G['env_ids']
    s, progress, change = E.prefill(G, task, device=DEV)
    p = E.plan_of(G, sc, DEV)
    be.task_reset(E.KIND[task], env_ids=p['env_ids'], u=p['u'], steps=p['steps'], **E.operands(task, s, progress, change), **E.params_of(sc))
    torch.cuda.synchronize()
    got = _cpu(E.outputs(task, s, change))
    s0, _, change0 = E.prefill(G, task)
    _check_against_f64(task, got, E.expected(G, sc), E.outputs(task, s0, change0), ids, lambda g: E.allowance(G, name, g), name)
    assert torch.equal(s['humanoid_root_states'].cpu(), G['root_states']) and torch.equal(progress.cpu(), G['progress_buf'])
    for g in set(got) - set(E.FLOAT_GROUPS[task]):           # change steps; strike's height, velocities: the reference's own
        assert torch.equal(got[g], sc['f32'][g]), (name, g)
    if name == 'heading_fixed':
        for g in ('tar_dir', 'tar_facing_dir'):
            assert torch.equal(got[g][ids], torch.tensor([1.0, 0.0]).expand(len(ids), 2)), g
    if task == 'strike':
        # the near / far choice: a near row lies within near_dist of its root, and the rows agree with the reference's
        # choice through their distance (a wrong choice moves a row by up to tar_dist_max - near_dist)
        near = sc['u'][:, 0] < sc['params']['near_prob']
        dist = (got['target_pos'][ids] - G['root_states'][ids, 0:2]).norm(dim=-1)
        want = (sc['f32']['target_pos'][ids] - G['root_states'][ids, 0:2]).norm(dim=-1)
        assert bool((dist[near] <= sc['params']['near_dist'] + 1e-5).all()) and float((dist - want).abs().max()) < 1e-4
        assert bool((got['target_rest'][ids, 0] == torch.tensor(0.9, dtype=torch.float32)).all()) and not got['target_rest'][ids, 1:].any()


# ---- 2. device draws equal passed-in draws --------------------------------------------------------------------------------------
@pytest.mark.parametrize('task', E.TASKS)
def test_device_draws_equal_passed_in_draws(be, G, task):
    """u / steps stated on the host from tests/ref_rollout.py (elements 4 e + j) and passed in give bitwise what the kernel
    gives on its own draws; the stream position moves by exactly one, or not at all with advance off."""
    sc = G['scenarios'][task]
    ids, kw = G['env_ids'], E.params_of(sc)
    for offset in OFFSETS:
        u, steps = E.device_draws(E.KIND[task], ids, SEED, offset, kw.get('steps_low', 0), kw.get('steps_high', 1))
        assert bool(((u >= 0) & (u < 1)).all())
        sa, progress, ca = E.prefill(G, task, device=DEV)
        be.task_reset(E.KIND[task], env_ids=_ids(ids), u=u.to(DEV), steps=None if task == 'strike' else steps.to(DEV),
                      **E.operands(task, sa, progress, ca), **kw)
        for advance in (True, False):
            sb, _, cb = E.prefill(G, task, device=DEV)
            st = _rng(SEED, offset)
            be.task_reset(E.KIND[task], env_ids=_ids(ids), rng_state=st, advance=advance, **E.operands(task, sb, progress, cb), **kw)
            torch.cuda.synchronize()
            assert _equal(_cpu(E.outputs(task, sb, cb)), _cpu(E.outputs(task, sa, ca))), (task, offset, advance)
            assert st.tolist() == [SEED, offset + int(advance)]
        if task != 'strike':
            assert torch.equal(ca.cpu()[ids], G['progress_buf'][ids] + steps)
    # the draws of an environment do not depend on its position in env_ids or on the other rows
    sub = ids[7:3:-1]
    sc_, _, cc = E.prefill(G, task, device=DEV)
    be.task_reset(E.KIND[task], env_ids=_ids(sub), rng_state=_rng(SEED, OFFSETS[-1]), **E.operands(task, sc_, progress, cc), **kw)
    torch.cuda.synchronize()
    for g, v in _cpu(E.outputs(task, sc_, cc)).items():
        assert torch.equal(v[sub], E.outputs(task, sb, cb)[g].cpu()[sub]), (task, g)


# ---- 3. due mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('task', TIMED)
def test_due_mode_is_ids_mode_on_the_due_rows(be, G, task):
    sc = G['scenarios'][task]
    kw, N = E.params_of(sc), G['num_envs']
    progress = G['progress_buf'].clone().to(DEV)
    change0 = progress.cpu() + (torch.arange(N) % 3 - 1)                  # rows above, equal to and below their change steps
    mask = progress.cpu() >= change0
    due = mask.nonzero().flatten().tolist()
    assert 0 < len(due) < N and bool((progress.cpu() == change0).any()) and bool((progress.cpu() > change0).any())
    sa, _, _ = E.prefill(G, task, device=DEV)
    sb, _, _ = E.prefill(G, task, device=DEV)
    ca, cb = change0.clone().to(DEV), change0.clone().to(DEV)
    ra, rb = _rng(SEED, 3), _rng(SEED, 3)
    be.task_reset(E.KIND[task], rng_state=ra, **E.operands(task, sa, progress, ca), **kw)
    be.task_reset(E.KIND[task], env_ids=_ids(due), rng_state=rb, **E.operands(task, sb, progress, cb), **kw)
    torch.cuda.synchronize()
    got = _cpu(E.outputs(task, sa, ca))
    assert _equal(got, _cpu(E.outputs(task, sb, cb))) and ra.tolist() == rb.tolist() == [SEED, 4]
    s0, _, _ = E.prefill(G, task)
    before = E.outputs(task, s0, change0)
    for g, v in got.items():
        assert torch.equal(v[~mask], before[g][~mask]) and not torch.equal(v[mask], before[g][mask]), (task, g)
    assert bool((got['change_steps'][mask] > G['progress_buf'][mask]).all())
    # nothing due: nothing is written, the stream position still moves
    sn, _, _ = E.prefill(G, task, device=DEV)
    cn, rn = (progress + 1).clone(), _rng(SEED, 3)
    be.task_reset(E.KIND[task], rng_state=rn, **E.operands(task, sn, progress, cn), **kw)
    torch.cuda.synchronize()
    assert _equal(_cpu(E.outputs(task, sn, cn)), E.outputs(task, s0, G['progress_buf'] + 1)) and rn.tolist() == [SEED, 4]


# ---- 4. shapes where it can go wrong ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 70, 257))
@pytest.mark.parametrize('task', E.TASKS)
def test_partial_waves_and_blocks_and_ids_outside_the_range(be, G, task, n):
    """n_envs of a partial wave, a wave and a bit, four blocks and a bit; env_ids shuffled with ids outside [0, n) among them
    (skipped, never dereferenced); due mode on the same grids."""
    sc = dict(G['scenarios'][task])
    C = _case(n, task)
    kw = E.params_of(sc)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).tolist()
    valid = perm[:max(1, (3 * n) // 4)]
    ids = []
    for i, e in enumerate(valid):
        ids.append(e)
        if i % 5 == 0:
            ids.append((-1, n, n + 5, -(1 << 31), (1 << 31) - 1)[(i // 5) % 5])
    s, progress, change = E.prefill(C, task, device=DEV)
    st = _rng(SEED, 9)
    be.task_reset(E.KIND[task], env_ids=_ids(ids), rng_state=st, **E.operands(task, s, progress, change), **kw)
    torch.cuda.synchronize()
    # the f64 result on the host statement of the same draws
    u, steps = E.device_draws(E.KIND[task], valid, SEED, 9, kw.get('steps_low', 0), kw.get('steps_high', 1))
    f, pf, cf = E.prefill(C, task, torch.float64)
    E.EmuTaskReset().task_reset(E.KIND[task], env_ids=torch.tensor(valid), u=u, steps=None if task == 'strike' else steps,
                                **E.operands(task, f, pf, cf), **kw)
    f64 = E.outputs(task, f, cf)
    s0, _, c0 = E.prefill(C, task)
    bar = lambda g: 2.0 * G['roundings'] * 2.0 ** -24 * float(f64[g][valid].abs().max()) + 1e-7
    _check_against_f64(task, _cpu(E.outputs(task, s, change)), f64, E.outputs(task, s0, c0), valid, bar, f'{task} n={n}')
    if task != 'strike':
        sa, _, ca = E.prefill(C, task, device=DEV)
        sb, _, cb = E.prefill(C, task, device=DEV)
        due = (progress >= ca).nonzero().flatten()
        be.task_reset(E.KIND[task], rng_state=_rng(SEED, 9), **E.operands(task, sa, progress, ca), **kw)
        be.task_reset(E.KIND[task], env_ids=due.to(torch.int32), rng_state=_rng(SEED, 9), **E.operands(task, sb, progress, cb), **kw)
        torch.cuda.synchronize()
        assert _equal(_cpu(E.outputs(task, sa, ca)), _cpu(E.outputs(task, sb, cb))), (task, n)


@pytest.mark.parametrize('task', ('location', 'strike'))
def test_strided_simulator_tensors(be, G, task):
    """root_states / target_states as the views [:, 0] / [:, 1] of the simulator's [N, 2, 13] root tensor: the contiguous
    result, the other actor's rows untouched."""
    sc = G['scenarios'][task]
    kw, N, ids = E.params_of(sc), G['num_envs'], G['env_ids']
    s, progress, change = E.prefill(G, task, device=DEV)
    sim = E.pattern(N, 2, 13).to(DEV)
    sim[:, 0] = s['humanoid_root_states']
    if task == 'strike':
        sim[:, 1] = s['target_states']
    sim0 = sim.clone()
    t = dict(s, humanoid_root_states=sim[:, 0])
    if task == 'strike':
        t['target_states'] = sim[:, 1]
    else:
        t['tar_pos'] = s['tar_pos'].clone()
    c2 = None if change is None else change.clone()
    be.task_reset(E.KIND[task], env_ids=_ids(ids), rng_state=_rng(SEED, 1), **E.operands(task, t, progress, c2), **kw)
    be.task_reset(E.KIND[task], env_ids=_ids(ids), rng_state=_rng(SEED, 1), **E.operands(task, s, progress, change), **kw)
    torch.cuda.synchronize()
    assert torch.equal(sim[:, 0], sim0[:, 0])
    if task == 'strike':
        others = [e for e in range(N) if e not in ids]
        assert torch.equal(sim[:, 1], s['target_states']) and torch.equal(sim[others, 1], sim0[others, 1])
        assert not torch.equal(sim[ids, 1], sim0[ids, 1])
    else:
        assert torch.equal(sim, sim0) and torch.equal(t['tar_pos'], s['tar_pos']) and torch.equal(c2, change)


def test_one_id(be, G):
    sc = G['scenarios']['reach']
    s, progress, change = E.prefill(G, 'reach', device=DEV)
    be.task_reset(L.TASK_REACH, env_ids=_ids([13]), rng_state=_rng(SEED, 0), **E.operands('reach', s, progress, change), **E.params_of(sc))
    torch.cuda.synchronize()
    s0, _, c0 = E.prefill(G, 'reach')
    keep = torch.arange(G['num_envs']) != 13
    assert torch.equal(s['tar_pos'].cpu()[keep], s0['tar_pos'][keep]) and torch.equal(change.cpu()[keep], c0[keep])
    u, steps = E.device_draws(L.TASK_REACH, [13], SEED, 0, 50, 100)
    assert int(change[13]) == int(G['progress_buf'][13]) + int(steps[0]) and not torch.equal(s['tar_pos'].cpu()[13], s0['tar_pos'][13])


# ---- 5. launch program --------------------------------------------------------------------------------------------------------
def _heading_tensors(be, G, seed):
    ht = HumanoidTensors(be, G['num_envs'], 17, task='heading', seed=seed, **G['scenarios']['heading']['params'])
    s, progress, change = E.prefill(G, 'heading', device=DEV)
    ht.change_steps.copy_(change)
    return ht, s, progress


def test_update_task_replays_in_a_launch_program(be, G):
    """update_task recorded once, replayed twice with progress_buf advanced in between: each replay resets what is due by the
    progress_buf it finds, on the stream position it finds; recording executes nothing."""
    ht, s, progress = _heading_tensors(be, G, SEED)
    twin, s2, _ = _heading_tensors(be, G, SEED)
    s0 = {k: v.clone() for k, v in s.items()}
    change0 = ht.change_steps.clone()
    prog = be.prog_create()
    be.prog_begin(prog)
    ht.update_task(s, progress)
    be.prog_end(prog)
    torch.cuda.synchronize()
    assert be.prog_size(prog) >= 1
    assert all(torch.equal(s[k], s0[k]) for k in s0) and torch.equal(ht.change_steps, change0) and ht.rng_state.tolist() == [SEED, 0]
    sizes = []
    for replay in range(2):
        due = (progress >= twin.change_steps).nonzero().flatten()
        sizes.append(due.numel())
        twin.reset_task(s2, due, progress)                                 # eager, ids mode: what the replay has to give
        be.prog_launch(prog)
        torch.cuda.synchronize()
        assert all(torch.equal(s[k], s2[k]) for k in s) and torch.equal(ht.change_steps, twin.change_steps), replay
        assert ht.rng_state.tolist() == twin.rng_state.tolist() == [SEED, replay + 1]
        progress += 120                                                    # the simulator's steps between two updates
    assert 0 < sizes[0] < G['num_envs'] and sizes[1] > 0
    be.prog_destroy(prog)


# ---- 6. the torch op ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SCENARIOS)
def test_torch_op_equals_the_backend_call(be, G, name):
    sc = G['scenarios'][name]
    task, kw = sc['task'], E.params_of(sc)
    ranges = [kw[k] for k in ase_amd.ops._RESET_RANGES[task]]
    p = E.plan_of(G, sc, DEV)
    for mode in ('passed in', 'device', 'due'):
        if mode == 'due' and task == 'strike':
            continue
        sa, progress, ca = E.prefill(G, task, device=DEV)
        sb, _, cb = E.prefill(G, task, device=DEV)
        ra, rb = _rng(SEED, 2), _rng(SEED, 2)
        draws = dict(env_ids=p['env_ids'], u=p['u'], steps=p['steps']) if mode == 'passed in' else \
            dict(env_ids=p['env_ids'] if mode == 'device' else None, rng_state=ra)
        be.task_reset(E.KIND[task], **draws, **E.operands(task, sa, progress, ca), **kw)
        o = E.operands(task, sb, progress, cb)
        d = dict(draws, rng_state=rb) if 'rng_state' in draws else draws
        torch.ops.ase_hip.task_reset(task, ranges, kw.get('steps_low', 0), kw.get('steps_high', 0), kw.get('enable_rand_heading', True),
                                     o.get('progress_buf'), o.get('change_steps'), o.get('root_states'), o.get('tar_a'), o.get('tar_b'),
                                     o.get('tar_speed'), o.get('tar_states'), d.get('env_ids'), d.get('u'), d.get('steps'),
                                     d.get('rng_state'))
        torch.cuda.synchronize()
        assert _equal(_cpu(E.outputs(task, sa, ca)), _cpu(E.outputs(task, sb, cb))) and ra.tolist() == rb.tolist(), (name, mode)
    with pytest.raises(RuntimeError):
        torch.ops.ase_hip.task_reset(task, ranges + [1.0], 0, 1, True, torch.zeros(4, dtype=torch.int64, device=DEV), *([None] * 10))


# ---- 7. through HumanoidTensors -------------------------------------------------------------------------------------------------
def _body_state(G, root):
    N, B = G['num_envs'], 17
    g = torch.Generator().manual_seed(31)
    r = lambda *shape: torch.randn(*shape, generator=g)
    rot = r(N, B, 4)
    s = {'rigid_body_pos': r(N, B, 3), 'rigid_body_rot': rot / rot.norm(dim=-1, keepdim=True), 'rigid_body_vel': r(N, B, 3),
         'rigid_body_ang_vel': r(N, B, 3)}
    s['rigid_body_pos'][:, 0], s['rigid_body_rot'][:, 0] = root[:, 0:3], root[:, 3:7]
    return {k: v.contiguous().to(DEV) for k, v in s.items()}


@pytest.mark.parametrize('task', TIMED)
def test_reset_task_then_observations(be, G, task):
    """reset_task, then compute_observations: the task columns are task_obs on the targets the reset wrote, and those targets
    are the f64 result on the host statement of the draws."""
    sc = G['scenarios'][task]
    extra = dict(reach_body_id=5) if task == 'reach' else {}
    ht = HumanoidTensors(be, G['num_envs'], 17, task=task, seed=SEED, **extra, **sc['params'])
    s, progress, change = E.prefill(G, task, device=DEV)
    ht.change_steps.copy_(change)
    s.update(_body_state(G, G['root_states']))
    ids = G['env_ids']
    ht.reset_task(s, ids, progress)
    obs = ht.compute_observations(s)
    torch.cuda.synchronize()
    kw = E.params_of(sc)
    u, steps = E.device_draws(E.KIND[task], ids, SEED, 0, kw['steps_low'], kw['steps_high'])
    f64 = E.expected(G, dict(sc, u=u, steps=steps))
    s0, _, c0 = E.prefill(G, task)
    bar = lambda g: 2.0 * G['roundings'] * 2.0 ** -24 * float(f64[g][ids].abs().max()) + 1e-7
    _check_against_f64(task, _cpu(E.outputs(task, s, ht.change_steps)), f64, E.outputs(task, s0, c0), ids, bar, f'HumanoidTensors {task}')
    tk = {'heading': dict(tar_a=s.get('tar_dir'), tar_b=s.get('tar_facing_dir'), tar_speed=s.get('tar_speed'))}.get(task, dict(tar_a=s.get('tar_pos')))
    want = torch.ops.ase_hip.task_obs(task, s['humanoid_root_states'], **tk)
    assert obs.shape == (G['num_envs'], 253 + L.TASK_OBS_COLS[E.KIND[task]]) and torch.equal(obs[:, 253:], want)
    assert ht.rng_state.tolist() == [SEED, 1]
    ht.update_task(s, progress)                                            # and the per-step call on the same object
    torch.cuda.synchronize()
    assert ht.rng_state.tolist() == [SEED, 2]


def test_strike_target_follows_the_root_of_the_actor_reset(be, G):
    """The reference calls _reset_target after the actor reset (humanoid_strike.py:103-106): reset_task behind
    HumanoidAMPTensors.apply_reset places the target relative to the root that reset wrote, not the one before it."""
    from ase_amd.amp_env import HumanoidAMPTensors
    from ase_amd.motion_lib import DeviceMotionLib
    from tests import emu_amp_reset as A
    GA, clips = A.load_fixture()
    assert GA['num_envs'] == G['num_envs']
    sa = GA['scenarios']['random']
    ml = DeviceMotionLib.from_arrays(clips, be, DEV)
    at = HumanoidAMPTensors(be, ml, GA['num_envs'], num_amp_obs_steps=GA['num_amp_obs_steps'], dt=GA['dt'], state_init='Random')
    s, _ = A.prefill(GA, device=DEV)
    s.pop('amp_obs_buf')
    s['target_states'] = E.pattern(G['num_envs'], 13).to(DEV)
    root_before = s['humanoid_root_states'].clone()
    plan = A.plan_of(GA, sa, DEV)
    ids = plan['env_ids'].tolist()
    sc = G['scenarios']['strike']
    ht = HumanoidTensors(be, G['num_envs'], 17, task='strike', strike_body_ids=[5], seed=SEED, **sc['params'])
    at.apply_reset(s, plan)
    ht.reset_task(s, plan['env_ids'])
    obs = ht.compute_observations(s)
    torch.cuda.synchronize()
    root = s['humanoid_root_states'].cpu()
    assert not torch.equal(root[ids, 0:2], root_before.cpu()[ids, 0:2])
    u, _ = E.device_draws(L.TASK_STRIKE, ids, SEED, 0)
    f = {'humanoid_root_states': root.double(), 'target_states': E.pattern(G['num_envs'], 13).double()}
    E.EmuTaskReset().task_reset(L.TASK_STRIKE, env_ids=torch.tensor(ids), u=u, steps=None, **E.operands('strike', f, None, None),
                                **E.params_of(sc))
    f64 = E.outputs('strike', f, None)
    bar = lambda g: 2.0 * G['roundings'] * 2.0 ** -24 * float(f64[g][ids].abs().max()) + 1e-7
    _check_against_f64('strike', _cpu(E.outputs('strike', s, None)), f64, E.outputs('strike', {'target_states': E.pattern(G['num_envs'], 13)}, None),
                       ids, bar, 'strike behind the actor reset')
    moved = (root[ids, 0:2] - root_before.cpu()[ids, 0:2]).norm(dim=-1)
    assert float(moved.min()) > 1e-3                   # every root moved by far more than the bar: the old root fails the check above
    dist = (s['target_states'].cpu()[ids, 0:2] - root[ids, 0:2]).norm(dim=-1)
    assert bool(((dist >= sc['params']['tar_dist_min'] - 1e-4) & (dist <= sc['params']['tar_dist_max'] + 1e-4)).all())
    want = torch.ops.ase_hip.task_obs('strike', s['humanoid_root_states'], tar_states=s['target_states'])
    assert torch.equal(obs[:, 253:], want) and ht.rng_state.tolist() == [SEED, 1]
