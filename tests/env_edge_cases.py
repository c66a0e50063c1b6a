"""Shared loader of tests/test_env_edges_emu.py and tests/test_gpu_env_edges.py: the groups of tests/golden/env_edges.pt
(scripts/make_golden_env_edges.py), operand builders for the C entries and for ``env_post_step``'s packed simulator layout, the
allowance, guarded output windows and the comparisons.  TEST INFRASTRUCTURE ONLY; it never reads the reference tree.

The float bar, per group and per output, against the reference's f64 run (rows a7, a10, N2 of COVERAGE.md):

    |x - ref_f64| <= 2 e_ref + 2^-23 max |ref_f64| + 1e-7

e_ref = max |ref_f32 - ref_f64| of the reference itself, stored with the group.  NaN and infinity positions are those of the
reference's f32 run; tie rows are compared with the f32 run (f64 may take the other branch); resets, terminates, copies,
untouched rows and guard words are exact."""
import math
import os

import torch

from ase_amd import lib as L
from tests import env_step_cases as CS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'env_edges.pt')
FLAGS = [(True, True), (True, False), (False, True), (False, False)]
TASKS = ['heading', 'location', 'reach', 'strike']
KIND = {'heading': L.TASK_HEADING, 'location': L.TASK_LOCATION, 'reach': L.TASK_REACH, 'strike': L.TASK_STRIKE}
RESET_KEYS = [('reset', form, early) for form in ('plain', 'strike') for early in (True, False)]
SENT, ISENT = -4321.5, -99
_CACHE = {}


def load():
    if 'G' not in _CACHE:
        _CACHE['G'] = torch.load(GOLDEN, weights_only=False)
    return _CACHE['G']


def groups(kind=None):
    G = load()
    return [(name, G['groups'][name]) for name in G['order'] if kind is None or G['groups'][name]['kind'] == kind]


def names(kind=None):
    return [name for name, _ in groups(kind)]


def group(name):
    return load()['groups'][name]


def allowance(grp, name):
    return 2.0 * grp['e_ref'][name] + 2.0 ** -23 * grp['max_ref'][name] + 1e-7


def mask(grp, name):
    G = load()
    return grp['masks'][G['reset_masks' if grp['kind'] == 'reset' else 'task_masks'].index(name)]


def reset_want(grp, tag, form, early):
    """(reset, terminated) of the reference's run `tag`, int64."""
    o = grp[tag][RESET_KEYS.index(('reset', form, early))].to(torch.int64)
    return o[0], o[1]


def obs_want(grp, tag, local_root, root_h):
    out = grp[tag]['obs_max'].clone()
    out[:, grp['obs_max_flag_cols']] = grp[tag]['obs_max_flag_cols'][(local_root, root_h)]
    return out


# ---- operands ----------------------------------------------------------------------------------------------------------------
def full_state(grp):
    """Every tensor a whole environment step reads, [n, B, ...]: the group's recorded inputs, and seeded filler (quiet forces,
    unit rotations) for what its reference functions did not consume."""
    n, B = grp['n'], grp['B']
    g = torch.Generator().manual_seed(1000 * n + B)
    q = torch.randn(n, B, 4, generator=g)
    i = {'body_pos': torch.randn(n, B, 3, generator=g) + torch.tensor([0.0, 0.0, 2.0]), 'body_rot': q / q.norm(dim=-1, keepdim=True),
         'body_vel': torch.randn(n, B, 3, generator=g), 'body_ang_vel': torch.randn(n, B, 3, generator=g),
         'contact_forces': (torch.rand(n, B, 3, generator=g) - 0.5) * 0.1, 'tar_contact_forces': torch.rand(n, 3, generator=g) - 0.5,
         'termination_heights': torch.full((B,), 0.15), 'progress_buf': torch.randint(0, 300, (n,), generator=g)}
    rec = {k: v.clone() for k, v in grp['inputs'].items()}
    if grp['kind'] == 'task':
        rs = rec['root_states']
        i['body_pos'][:, 0], i['body_rot'][:, 0], i['body_vel'][:, 0], i['body_ang_vel'][:, 0] = rs[:, 0:3], rs[:, 3:7], rs[:, 7:10], rs[:, 10:13]
        i['body_pos'][:, grp['reach_body_id']] = rec.pop('reach_body_pos')
    i.update(rec)
    if 'root_states' not in i:
        i['root_states'] = torch.cat([i['body_pos'][:, 0], i['body_rot'][:, 0], i['body_vel'][:, 0], i['body_ang_vel'][:, 0]], -1)
    if 'tar_states' not in i:
        i['tar_states'] = torch.randn(n, 13, generator=g)
    if 'prev_root_pos' not in i:
        i['prev_root_pos'] = i['body_pos'][:, 0] - 0.01 * torch.randn(n, 3, generator=g)
    return i


def to(i, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in i.items()}


def task_operands(grp, i, task, what):
    """Keyword operands of task_obs / task_reward for a task of the task group (the form of tests.emu_env_tensors)."""
    from tests.emu_env_tensors import task_operands as ops
    return ops(grp, i, task, what)


def reset_args(grp, i, early):
    return (i['progress_buf'], i['contact_forces'], i['body_pos'], i['termination_heights'], grp['contact_body_ids'],
            grp['max_episode_length'], early)


def strike_kw(grp, i, form):
    """The strike form's operands; the entry needs at least one strike body, a group without a list has the plain form only."""
    if form == 'plain':
        return {}
    return dict(tar_contact_forces=i['tar_contact_forces'], strike_body_ids=grp['strike_body_ids'])


def forms(grp):
    return ('plain', 'strike') if grp['strike_body_ids'] else ('plain',)


def packed(i, extra_body, D=3):
    """The state in the simulator's layout (env_step_cases.packed) with `extra_body` more bodies per environment, and the
    windows of it that env_post_step reads in place."""
    return CS.packed(i, CS.dof_state(i['body_pos'].shape[0], D), extra_body=bool(extra_body))


def packed_views(p, B, extra_body, i):
    rb, cf = p['rigid_body_state'], p['contact_forces']
    return dict(body_pos=rb[:, :B, 0:3], body_rot=rb[:, :B, 3:7], body_vel=rb[:, :B, 7:10], body_ang_vel=rb[:, :B, 10:13],
                contact_forces=cf[:, :B], root_states=p['root_states'][:, 0], tar_states=p['root_states'][:, 1],
                tar_contact_forces=cf[:, B] if extra_body else i['tar_contact_forces'])


# ---- guarded outputs ---------------------------------------------------------------------------------------------------------
class Guarded:
    """A window [lead : lead + rows, left : left + cols] of a sentinel-filled allocation: a wider pitch, a column offset, rows in
    front and behind.  ``rows_view`` is what an entry with a leading dimension takes (with ``left`` as its column offset);
    ``check`` asserts that every word outside the window - and inside it, outside the rows named - still holds the sentinel
    bit for bit, and returns how many words that were."""

    def __init__(self, rows, cols=None, dtype=torch.float32, device='cpu', lead=2, left=0, right=0):
        self.rows, self.cols, self.lead, self.left = rows, cols, lead, left
        self.fill = SENT if dtype.is_floating_point else ISENT
        shape = (rows + 2 * lead,) + (() if cols is None else (left + cols + right,))
        self.whole = torch.full(shape, self.fill, dtype=dtype, device=device)
        self.rows_view = self.whole[lead:lead + rows]
        self.view = self.rows_view if cols is None else self.rows_view[:, left:left + cols]

    def check(self, written_rows=None):
        own = torch.zeros(self.whole.shape, dtype=torch.bool, device=self.whole.device)
        rows = torch.arange(self.rows) if written_rows is None else torch.as_tensor(sorted(set(written_rows)), dtype=torch.long)
        if self.cols is None:
            own[self.lead + rows] = True
        else:
            own[self.lead + rows, self.left:self.left + self.cols] = True
        guard = self.whole[~own]
        assert bool((guard == self.fill).all()), 'a guard word was overwritten'
        return int(guard.numel())


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def check_float(got, want32, want64, allow, tie_rows=(), what=''):
    """got against the reference: the NaN / +-infinity positions of the f32 run, the finite elements within `allow` of the f64
    run - of the f32 run on the tie rows.  -> dict(err, elements, tie_elements)."""
    got = got.detach().cpu()
    assert got.shape == want32.shape, (what, got.shape, want32.shape)
    for f, label in ((torch.isnan, 'NaN'), (torch.isposinf, '+inf'), (torch.isneginf, '-inf')):
        assert torch.equal(f(got), f(want32)), f'{what}: {label} positions differ from the reference f32 run in rows ' \
            f'{sorted(set(torch.nonzero(f(got) != f(want32))[:, 0].tolist()))}'
    tie = torch.zeros(got.shape[0], dtype=torch.bool)
    tie[list(tie_rows)] = True
    ref = torch.where(tie.view(-1, *([1] * (got.dim() - 1))), want32.double(), want64)
    fin = torch.isfinite(want32) & torch.isfinite(ref)
    d = (got.double() - ref).abs()
    d[~fin] = 0
    err = float(d.max()) if d.numel() else 0.0
    assert err <= allow, f'{what}: max |x - reference| = {err:.3g} above the allowance {allow:.3g} (row {int(d.view(d.shape[0], -1).amax(1).argmax())})'
    per_row = got[0].numel() if got.shape[0] else 0
    return dict(err=err, elements=int(fin.sum()), tie_elements=int(tie.sum()) * per_row)


def same_bits(a, b):
    """Equality bit for bit of two float tensors (-0 is not +0); a NaN matches a NaN, whatever its sign and payload."""
    if a.shape != b.shape:
        return False
    a, b = a.contiguous(), b.contiguous()
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | both_nan).all())


def differing(a, b, k=4):
    """The first few elements in which two tensors differ, for a message."""
    bad = torch.nonzero(~((a == b) | (torch.isnan(a) & torch.isnan(b))))[:k]
    return [(tuple(ix.tolist()), float(a[tuple(ix)]), float(b[tuple(ix)])) for ix in bad]


def clamp_keep_nan(x, c):
    return x if c == math.inf else torch.clamp(x, -c, c)


def env_id_lists(n):
    """Subsets for the env_ids argument: duplicates, ids outside the range, an empty list -> [(list, rows written)]."""
    inside = sorted({0, n - 1, n // 2})
    dup = inside + inside[:1] + [-1, n, 1 << 20, -(1 << 30)]
    return [(dup, inside), ([], []), ([n + 5, -3], [])]


# ---- the cases, for any backend with HipBackend's signatures (the emulators on the CPU, HipBackend on the device) ---------------
class Stats(dict):
    """(group, output) -> observed max error, e_ref, allowance, elements / tie elements compared, guard words checked."""

    def add(self, grp_name, grp, out, r=None, guards=0, exact=0):
        s = self.setdefault(f'{grp_name}:{out}', dict(err=0.0, e_ref=grp['e_ref'].get(out), allowance=allowance(grp, out) if out in grp['e_ref'] else 0.0,
                                                      elements=0, tie_elements=0, guard_words=0, exact_elements=0))
        if r is not None:
            s['err'] = max(s['err'], r['err'])
            s['elements'] += r['elements']
            s['tie_elements'] += r['tie_elements']
        s['guard_words'] += guards
        s['exact_elements'] += exact


def _sync(device):
    if str(device).startswith('cuda'):
        torch.cuda.synchronize()


def run_reset_group(be, name, grp, device, stats):
    i = to(grp['inputs'], device)
    n = grp['n']
    for form in forms(grp):
        for early in (True, False):
            reset, term = Guarded(n, dtype=torch.int64, device=device), Guarded(n, dtype=torch.int64, device=device)
            be.humanoid_reset(*reset_args(grp, i, early), reset.view, term.view, **strike_kw(grp, i, form))
            _sync(device)
            words = reset.check() + term.check()
            w_reset, w_term = reset_want(grp, 'f32', form, early)
            bad = torch.nonzero((reset.view.cpu() != w_reset) | (term.view.cpu() != w_term)).view(-1).tolist()
            assert not bad, f'{name} {form} early={early}: rows {bad} differ from the reference: ' \
                f'{[w for r, w in grp["planted"] if r in bad][:4]}'
            stats.add(name, grp, f'reset_{form}', guards=words, exact=2 * n)


def run_task(be, name, grp, device, stats, task):
    i = to(full_state(grp), device)
    n, k = grp['n'], KIND[task]
    cols = L.TASK_OBS_COLS[k]
    obs = Guarded(n, cols, device=device, left=3, right=4)
    be.task_obs(k, obs.rows_view, 3, None, **task_operands(grp, i, task, 'obs'))
    _sync(device)
    words = obs.check()
    r = check_float(obs.view, grp['f32'][f'{task}_obs'], grp['f64'][f'{task}_obs'], allowance(grp, f'{task}_obs'), (), f'{name} {task}_obs')
    if task == 'heading':
        assert same_bits(obs.view[:, 2], i['tar_speed'])                              # a pure copy
    stats.add(name, grp, f'{task}_obs', r, words)
    rew = Guarded(n, device=device)
    be.task_reward(k, rew.view, **task_operands(grp, i, task, 'rew'))
    _sync(device)
    words = rew.check()
    r = check_float(rew.view, grp['f32'][f'{task}_rew'], grp['f64'][f'{task}_rew'], allowance(grp, f'{task}_rew'),
                    grp['tie_rows'] if task == 'strike' else (), f'{name} {task}_rew')
    stats.add(name, grp, f'{task}_rew', r, words)
    return obs.view, rew.view


def run_obs_group(be, name, grp, device, stats):
    i = to(grp['inputs'], device)
    n, F = grp['n'], 15 * grp['B'] - 2
    for local_root, root_h in FLAGS:
        obs = Guarded(n, F, device=device, left=3, right=6)
        be.humanoid_obs_max(i['body_pos'], i['body_rot'], i['body_vel'], i['body_ang_vel'], local_root, root_h, obs.rows_view, 3)
        _sync(device)
        words = obs.check()
        r = check_float(obs.view, obs_want(grp, 'f32', local_root, root_h), obs_want(grp, 'f64', local_root, root_h),
                        allowance(grp, 'obs_max'), (), f'{name} obs_max local_root={local_root} root_h={root_h}')
        if root_h:
            assert same_bits(obs.view[:, 0], i['body_pos'][:, 0, 2])                   # a pure copy
        else:
            assert not obs.view[:, 0].any()
        stats.add(name, grp, 'obs_max', r, words)


def post_step_tasks(grp):
    if grp['kind'] == 'task':
        return TASKS
    return [None] + (['strike'] if grp['kind'] == 'reset' and grp['strike_body_ids'] else [])


def run_post_step(be, name, grp, device, stats, task, extra_body, clip, with_counter, local_root=True):
    """The group once through env_post_step on packed state (progress one less: the launch increments first) -> bitwise the
    separate entries on contiguous copies; reset / terminate the recording's; the clipped observation clamp(reference)."""
    i = full_state(grp)
    n, B = grp['n'], grp['B']
    dt = grp.get('dt', 1.0 / 30.0)
    c = to(i, device)
    p = to(packed(i, extra_body), device)
    v = packed_views(p, B, extra_body, c)
    F = 15 * B - 2
    kind = None if task is None else KIND[task]
    tcols = 0 if task is None else L.TASK_OBS_COLS[kind]
    off = 3
    obs = Guarded(n, F + tcols, device=device, left=off, right=5)
    rew = Guarded(n, device=device)
    reset, term, prog = (Guarded(n, dtype=torch.int64, device=device) for _ in range(3))
    prog.view.copy_(c['progress_buf'] - 1)
    kw = dict(task_kind=kind, enable_task_obs=True)
    G2 = dict(grp, dt=dt, tar_speed=grp.get('tar_speed', 1.0), reach_body_id=grp.get('reach_body_id', 0))
    if task is not None:
        iv = dict(c)
        iv.update(root_states=v['root_states'], tar_states=v['tar_states'], body_pos=v['body_pos'])
        if grp['kind'] == 'task':
            ops = dict(task_operands(G2, iv, task, 'rew'))
            ops.update(task_operands(G2, iv, task, 'obs'))
        else:
            ops = dict(root_states=iv['root_states'], tar_states=iv['tar_states'], prev_root_pos=c['prev_root_pos'], dt=dt)
        if 'body_pos' in ops:
            ops.pop('body_pos')
            kw['reach_body_id'] = ops.pop('body_id')
        kw.update(ops)
    strike = task == 'strike'
    if strike:
        kw.update(tar_contact_forces=v['tar_contact_forces'], strike_body_ids=grp['strike_body_ids'])
    counter = None
    if with_counter:
        counter = ((torch.arange(n) % 3 == 1).to(torch.int32) * 2).to(device)
        kw['recovery_counter'] = counter
    be.env_post_step(v['body_pos'], v['body_rot'], v['body_vel'], v['body_ang_vel'], v['contact_forces'], prog.view, obs.rows_view,
                     rew.view, reset.view, term.view, c['termination_heights'], grp['contact_body_ids'], grp['max_episode_length'], True,
                     local_root, True, col_offset=off, clip_obs=clip, **kw)
    _sync(device)
    words = obs.check() + rew.check() + reset.check() + term.check() + prog.check()
    assert torch.equal(prog.view, c['progress_buf'])
    # ---- the separate entries on contiguous copies
    want = torch.full((n, F + tcols), SENT, device=device)
    be.humanoid_obs_max(c['body_pos'], c['body_rot'], c['body_vel'], c['body_ang_vel'], local_root, True, want, 0)
    w_rew = torch.ones(n, device=device)
    if task is not None:
        if grp['kind'] == 'task':
            o_ops, r_ops = task_operands(G2, c, task, 'obs'), task_operands(G2, c, task, 'rew')
        else:
            o_ops = dict(root_states=c['root_states'], tar_states=c['tar_states'])
            r_ops = dict(o_ops, prev_root_pos=c['prev_root_pos'], dt=dt)
        be.task_obs(kind, want, F, None, **o_ops)
        be.task_reward(kind, w_rew, **r_ops)
    w_reset, w_term = torch.zeros_like(reset.view), torch.zeros_like(term.view)
    be.humanoid_reset(c['progress_buf'], c['contact_forces'], c['body_pos'], c['termination_heights'], grp['contact_body_ids'],
                      grp['max_episode_length'], True, w_reset, w_term, **strike_kw(grp, c, 'strike' if strike else 'plain'))
    _sync(device)
    assert same_bits(obs.view, clamp_keep_nan(want, clip)), \
        f'{name} {task}: the observation is not the separate entries, bit for bit: {differing(obs.view, clamp_keep_nan(want, clip))}'
    assert same_bits(rew.view, w_rew), f'{name} {task}: the reward is not the separate entry, bit for bit'
    rec = torch.zeros(n, dtype=torch.bool, device=device) if counter is None else counter > 0
    assert torch.equal(reset.view, w_reset.masked_fill(rec, 0)) and torch.equal(term.view, w_term.masked_fill(rec, 0))
    exact = obs.view.numel() + 4 * n
    # ---- the recording
    if grp['kind'] == 'reset':
        r_reset, r_term = reset_want(grp, 'f32', 'strike' if strike else 'plain', True)
        assert torch.equal(reset.view.cpu(), r_reset.masked_fill(rec.cpu(), 0)) and torch.equal(term.view.cpu(), r_term.masked_fill(rec.cpu(), 0)), \
            f'{name} {task}: reset / terminate differ from the reference'
        exact += 2 * n
    if grp['kind'] == 'obs':
        r = check_float(obs.view, clamp_keep_nan(obs_want(grp, 'f32', local_root, True), clip), clamp_keep_nan(obs_want(grp, 'f64', local_root, True), clip),
                        allowance(grp, 'obs_max'), (), f'{name} post_step clip {clip}')
        stats.add(name, grp, 'obs_max', r)
    elif grp['kind'] == 'task':
        for what, got in ((f'{task}_obs', obs.view[:, F:]), (f'{task}_rew', rew.view)):
            r = check_float(got, clamp_keep_nan(grp['f32'][what], clip if what.endswith('obs') else math.inf),
                            clamp_keep_nan(grp['f64'][what], clip if what.endswith('obs') else math.inf), allowance(grp, what),
                            grp['tie_rows'] if what == 'strike_rew' else (), f'{name} post_step {what}')
            stats.add(name, grp, what, r)
    stats.add(name, grp, 'post_step', guards=words, exact=exact)
