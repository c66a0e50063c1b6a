"""The environment kernels at the branch edges and on non-finite state, on the GPU: ``humanoid_obs_max``,
``humanoid_reset``, ``task_obs`` and ``task_reward`` through ``HipBackend`` and ``torch.ops.ase_hip.*`` on every group of
tests/golden/env_edges.pt (recorded from the unmodified reference by scripts/make_golden_env_edges.py), and every group once
more through ``ase_hip_env_post_step`` on packed simulator state.  The cases, operands and comparisons are those of
tests/env_edge_cases.py, shared with the CPU stand-ins (tests/test_env_edges_emu.py):

    floats   |hip - ref_f64| <= 2 e_ref + 2^-23 max |ref| + 1e-7 per group and output; tie rows against the f32 run
    NaN/inf  at the positions of the reference's f32 run
    exact    resets, terminates, copies, untouched rows, every guard word of the NaN-free sentinel frames

Set ASE_ENV_EDGES_REPORT=<path> to get, per group and output, the observed max |hip - f64|, e_ref, the allowance, the elements
and tie elements compared and the guard words checked, as one JSON document."""
import json
import math
import os

import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from tests import env_edge_cases as EC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
STATS = EC.Stats()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    path = os.environ.get('ASE_ENV_EDGES_REPORT')
    if path:
        total = {k: sum(s[k] for s in STATS.values()) for k in ('elements', 'tie_elements', 'guard_words', 'exact_elements')}
        with open(path, 'w') as f:
            json.dump({'total': total, 'outputs': STATS}, f, indent=1)


@pytest.mark.parametrize('name', EC.names('reset'))
def test_reset_group_is_exact(be, name):
    EC.run_reset_group(be, name, EC.group(name), DEV, STATS)


@pytest.mark.parametrize('task', EC.TASKS)
def test_task_obs_and_reward(be, task):
    EC.run_task(be, 'tasks', EC.group('tasks'), DEV, STATS, task)


@pytest.mark.parametrize('name', EC.names('obs'))
def test_obs_group(be, name):
    EC.run_obs_group(be, name, EC.group(name), DEV, STATS)


@pytest.mark.parametrize('name', EC.names())
def test_post_step_on_every_group(be, name):
    grp = EC.group(name)
    for task in EC.post_step_tasks(grp):
        EC.run_post_step(be, name, grp, DEV, STATS, task, 0, math.inf, False)
        EC.run_post_step(be, name, grp, DEV, STATS, task, 1, 5.0, True, local_root=False)


def _ids(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('name', ['obs_n1_b1', 'obs_n33_b5', 'obs_n17_b64'])
def test_obs_env_ids_with_duplicates_strangers_and_nothing(be, name):
    grp = EC.group(name)
    i = EC.to(grp['inputs'], DEV)
    n, F = grp['n'], 15 * grp['B'] - 2
    state = (i['body_pos'], i['body_rot'], i['body_vel'], i['body_ang_vel'])
    full = torch.zeros(n, F, device=DEV)
    be.humanoid_obs_max(*state, True, True, full)
    for ids, written in EC.env_id_lists(n):
        g = EC.Guarded(n, F, device=DEV, left=2, right=3)
        be.humanoid_obs_max(*state, True, True, g.rows_view, 2, _ids(ids))
        torch.cuda.synchronize()
        words = g.check(written)
        assert EC.same_bits(g.view[written], full[written])
        STATS.add(name, grp, 'env_ids', guards=words, exact=len(written) * F)


@pytest.mark.parametrize('task', EC.TASKS)
def test_task_obs_env_ids_with_duplicates_strangers_and_nothing(be, task):
    grp = EC.group('tasks')
    i = EC.to(EC.full_state(grp), DEV)
    n, k = grp['n'], EC.KIND[task]
    cols = EC.L.TASK_OBS_COLS[k]
    kw = EC.task_operands(grp, i, task, 'obs')
    full = torch.zeros(n, cols, device=DEV)
    be.task_obs(k, full, **kw)
    for ids, written in EC.env_id_lists(n):
        g = EC.Guarded(n, cols, device=DEV, left=2, right=3)
        be.task_obs(k, g.rows_view, 2, _ids(ids), **kw)
        torch.cuda.synchronize()
        words = g.check(written)
        assert EC.same_bits(g.view[written], full[written])
        STATS.add('tasks', grp, 'env_ids', guards=words, exact=len(written) * cols)


def test_torch_ops_forms_give_the_same_bits(be):
    ops = torch.ops.ase_hip
    grp = EC.group('obs_n17_b64')
    i = EC.to(grp['inputs'], DEV)
    state = (i['body_pos'], i['body_rot'], i['body_vel'], i['body_ang_vel'])
    want = torch.zeros(grp['n'], 15 * grp['B'] - 2, device=DEV)
    be.humanoid_obs_max(*state, False, True, want)
    assert EC.same_bits(ops.humanoid_obs_max(*state, False, True), want)
    grp = EC.group('reset_ties')
    i = EC.to(grp['inputs'], DEV)
    for form in ('plain', 'strike'):
        r, t = ops.humanoid_reset(*EC.reset_args(grp, i, True), **EC.strike_kw(grp, i, form))
        w_r, w_t = EC.reset_want(grp, 'f32', form, True)
        assert torch.equal(r.cpu(), w_r) and torch.equal(t.cpu(), w_t)
    grp = EC.group('tasks')
    i = EC.to(EC.full_state(grp), DEV)
    for task in EC.TASKS:
        k = EC.KIND[task]
        kw = EC.task_operands(grp, i, task, 'obs')
        want = torch.zeros(grp['n'], EC.L.TASK_OBS_COLS[k], device=DEV)
        be.task_obs(k, want, **kw)
        assert EC.same_bits(ops.task_obs(task, **kw), want)
        kw = EC.task_operands(grp, i, task, 'rew')
        rew = torch.zeros(grp['n'], device=DEV)
        be.task_reward(k, rew, **kw)
        okw = {('tar_speed_scalar' if key == 'tar_speed' and not torch.is_tensor(v) else key): v for key, v in kw.items()}
        assert EC.same_bits(ops.task_reward(task, grp['n'], **okw), rew)
        r = EC.check_float(rew, grp['f32'][f'{task}_rew'], grp['f64'][f'{task}_rew'], EC.allowance(grp, f'{task}_rew'),
                           grp['tie_rows'] if task == 'strike' else (), f'torch.ops {task}_rew')
        STATS.add('tasks', grp, f'{task}_rew', r)


@pytest.mark.parametrize('task,what', [('strike', 'NaN target rotation w'), ('strike', 'NaN target rotation z'),
                                       ('heading', 'NaN tar_face_dir y'), ('location', 'NaN previous root position x'),
                                       ('strike', 'NaN previous root position y')])
def test_a_nan_operand_gives_a_nan_reward(be, task, what):
    """The cases the clamps of task_reward_row dropped while they were fmaxf: the reference's reward is NaN, a finite reward
    would tell the agent that a blown-up state is an ordinary one."""
    grp = EC.group('tasks')
    row = {w: r for r, w in grp['planted']}['non-finite: ' + what]
    i = EC.to(EC.full_state(grp), DEV)
    rew = torch.zeros(grp['n'], device=DEV)
    be.task_reward(EC.KIND[task], rew, **EC.task_operands(grp, i, task, 'rew'))
    assert math.isnan(float(grp['f32'][f'{task}_rew'][row])) and math.isnan(float(grp['f64'][f'{task}_rew'][row]))
    assert math.isnan(float(rew[row])), f'{task} reward with a {what}: {float(rew[row])} where the reference has NaN'
