"""Device-drawn HumanoidAMP / HumanoidAMPGetup resets on the MI355X: ``ase_hip_amp_reset_due`` through
``HipBackend``, ``HumanoidAMPTensors.reset_due`` and ``torch.ops.ase_hip.amp_reset_due``.  Every comparison is bitwise: the
exported plan against the numpy statement of the draws (tests/ref_amp_reset_due.py), everything the launch writes against a
second copy on which ``ase_hip_amp_reset`` (pinned to the reference by tests/test_gpu_amp_reset.py) applied that plan and the
host did the book-keeping.  State, history, buffers and plan live in longer NaN- / sentinel-filled allocations, so untouched
rows and gaps are part of every comparison."""
import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd import lib as L
from ase_amd.amp_env import HumanoidAMPTensors
from ase_amd.env_tensors import HumanoidTensors
from ase_amd.motion_lib import DeviceMotionLib
from tests import emu_amp_reset as E
from tests import ref_amp_reset_due as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 3                      # spare rows behind every allocation
SENTINEL = -77
STATE_KEYS = ('humanoid_root_states', 'dof_pos', 'dof_vel')
BODY_KEYS = ('rigid_body_pos', 'rigid_body_rot', 'rigid_body_vel', 'rigid_body_ang_vel')
COUNTS = {'cases': 0, 'elements': 0, 'unequal': 0}


@pytest.fixture(scope='module')
def GC():
    return E.load_fixture()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(DEV)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\namp_reset_due: comparisons', COUNTS)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    """Bitwise equality of two whole allocations (NaN fill included), counted."""
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = int((a != b).sum())
    COUNTS['cases'] += 1
    COUNTS['elements'] += a.numel()
    COUNTS['unequal'] += bad
    assert bad == 0, (what, bad)


def _padded(rows, fill):
    """rows [N, ...] at the front of an allocation of N + PAD rows filled with `fill` -> (allocation, view of the N rows)."""
    big = torch.full((rows.shape[0] + PAD,) + tuple(rows.shape[1:]), fill, dtype=rows.dtype, device=DEV)
    big[:rows.shape[0]] = rows.to(DEV)
    return big, big[:rows.shape[0]]


class Copy:
    """One copy of everything a reset touches, N environments whose rows repeat the fixture's."""

    def __init__(self, be, G, clips, N=32, S=10, state_init='Hybrid', getup=True, seed=R.SEED, offset=0, reset=None, strided=False):
        self.N, self.getup, self.state_init = N, getup, state_init
        idx = torch.arange(N) % G['num_envs']
        ml = DeviceMotionLib.from_arrays(clips, be, DEV)
        kw = {}
        if getup:
            kw.update(recovery_episode_prob=G['recovery_episode_prob'], recovery_steps=G['recovery_steps'], fall_init_prob=G['fall_init_prob'])
        at = HumanoidAMPTensors(be, ml, N, num_amp_obs_steps=S, dt=G['dt'], state_init=state_init, hybrid_init_prob=G['hybrid_init_prob'],
                                local_root_obs=G['local_root_obs'], root_height_obs=G['root_height_obs'], seed=seed, **kw)
        at.rng_state[1] = offset
        init, fall = E.tables(G)
        at.set_initial_state(*[t[idx] for t in init])
        if getup:
            at.set_fall_states(*fall)
        s0, b0 = E.prefill(G)
        nan = float('nan')
        self.alloc, s = {}, {}
        D = G['num_dof']
        if strided:                                            # the simulator's interleaved dof state and actor-major root states
            dof_state = torch.full((N + PAD, D + 2, 2), nan, device=DEV)
            dof_state[:N, :D, 0], dof_state[:N, :D, 1] = s0['dof_pos'][idx].to(DEV), s0['dof_vel'][idx].to(DEV)
            actors = torch.full((N + PAD, 3, 13), nan, device=DEV)
            actors[:N, 0] = s0['humanoid_root_states'][idx].to(DEV)
            self.alloc.update(dof_state=dof_state, actors=actors)
            s.update(dof_pos=dof_state[:N, :D, 0], dof_vel=dof_state[:N, :D, 1], humanoid_root_states=actors[:N, 0])
        else:
            for k in STATE_KEYS:
                self.alloc[k], s[k] = _padded(s0[k][idx], nan)
        for k in BODY_KEYS:
            s[k] = s0[k][idx].contiguous().to(DEV)
        self.alloc['hist'], at.amp_obs_buf = _padded(E.hist_pattern(N, S, G['num_amp_obs_per_step']), nan)
        self.bufs = {}
        b0 = dict(b0, reset_buf=R.reset_pattern(G['num_envs']))
        for k in ('progress_buf', 'reset_buf', 'terminate_buf'):
            self.alloc[k], self.bufs[k] = _padded(b0[k][idx], SENTINEL)
        if reset is not None:
            self.bufs['reset_buf'].copy_(reset)
        if getup:
            self.alloc['recovery_counter'], at.recovery_counter = _padded(b0['recovery_counter'][idx], SENTINEL)
        for k in R.PLAN_KEYS:
            self.alloc['plan_' + k], at.plan[k] = _padded(torch.full((N,), 5, dtype=at.plan[k].dtype), SENTINEL)
        self.alloc['rng_state'] = at.rng_state
        self.at, self.s, self.body0 = at, s, {k: s[k].clone() for k in BODY_KEYS}
        self.cfg = dict(state_init=state_init, hybrid_init_prob=G['hybrid_init_prob'],
                        getup=(G['recovery_episode_prob'], G['recovery_steps'], G['fall_init_prob']) if getup else None)
        self.n_fall = G['num_fall_states'] if getup else 0

    def ref_plan(self):
        """The numpy statement of the plan at the copy's current buffers and stream position -> device tensors."""
        rng = self.at.rng_state.tolist()
        ml = self.at._motion_lib
        P = R.ref_plan(rng[0], rng[1], self.bufs['reset_buf'].cpu().numpy(), self.bufs['terminate_buf'].cpu().numpy(), self.cfg,
                       ml.clip_cdf.cpu().numpy(), ml.clips['lengths'].cpu().numpy(), self.n_fall)
        return R.plan_tensors(P, DEV)

    def reset_due(self, advance=True):
        b = self.bufs
        return self.at.reset_due(self.s, b['progress_buf'], b['reset_buf'], b['terminate_buf'], advance=advance)

    def apply_full_plan(self, plan, advance=True):
        """ase_hip_amp_reset (ids mode) on a full-length plan, rows -1 included, then the host's book-keeping."""
        at, b = self.at, self.bufs
        for k in R.PLAN_KEYS:
            at.plan[k].copy_(plan[k])
        at._launch(self.s, at.plan, L.RESET_HAS_MOTION | (L.RESET_HAS_TABLE if at._table is not None else 0))
        R.bookkeeping(at.plan, self.N, b['progress_buf'], b['reset_buf'], b['terminate_buf'], at.recovery_counter, self.cfg['getup'])
        if advance:
            at.rng_state[1] += 1


def _compare(a, b, what):
    assert set(a.alloc) == set(b.alloc)
    for k in a.alloc:
        _same(a.alloc[k], b.alloc[k], (what, k))
    for k in BODY_KEYS:                                        # inputs stay inputs
        _same(a.s[k], a.body0[k], (what, k))


def _run(be, G, clips, what, advance=True, **kw):
    """reset_due on one copy: the exported plan is the numpy plan, and everything equals the ids-mode kernel on that plan."""
    a, b = Copy(be, G, clips, **kw), Copy(be, G, clips, **kw)
    want = a.ref_plan()
    seed0, off0 = a.at.rng_state.tolist()
    plan = a.reset_due(advance=advance)
    torch.cuda.synchronize()
    for k in R.PLAN_KEYS:
        _same(plan[k], want[k], (what, 'plan', k))
    assert a.at.rng_state.tolist() == [seed0, off0 + int(advance)], what
    b.apply_full_plan(want, advance=advance)
    torch.cuda.synchronize()
    _compare(a, b, what)
    due = want['env_ids'] >= 0
    assert not a.bufs['reset_buf'].any() and not a.bufs['progress_buf'][due].any() and a.bufs['progress_buf'][~due].all(), what
    return a, want


def _groups(P, N):
    due = P['env_ids'] >= 0
    k, s = P['kind'], P['src_rows']
    return {'recovery': due & (k == L.RESET_FRAME), 'fall': due & (k == L.RESET_TABLE) & (s >= N), 'motion': due & (k == L.RESET_MOTION),
            'default': due & (k == L.RESET_TABLE) & (s < N)}


@pytest.mark.parametrize('getup', [False, True])
@pytest.mark.parametrize('state_init', ['Default', 'Start', 'Random', 'Hybrid'])
def test_plan_and_apply(be, GC, state_init, getup):
    G, clips = GC
    a, want = _run(be, G, clips, (state_init, getup), state_init=state_init, getup=getup)
    g = _groups(want, a.N)
    if state_init == 'Hybrid' and getup:
        assert all(int(m.sum()) >= 2 for m in g.values()), {k: int(m.sum()) for k, m in g.items()}
    if getup:
        counted = g['recovery'] | g['fall']
        assert (a.at.recovery_counter[counted] == G['recovery_steps']).all() and not a.at.recovery_counter[g['motion'] | g['default']].any()


@pytest.mark.parametrize('offset,advance', [(5, True), ((1 << 32) + 7, True), (5, False)])
def test_stream_positions(be, GC, offset, advance):
    G, clips = GC
    a, want = _run(be, G, clips, ('offset', offset, advance), offset=offset, advance=advance)
    other = Copy(be, G, clips, offset=0).ref_plan()
    assert not all(torch.equal(want[k], other[k]) for k in R.PLAN_KEYS)          # another position: other draws
    assert R.SEED > 1 << 32


@pytest.mark.parametrize('N,S,pattern', [(1, 10, 'all'), (70, 10, 'blocks'), (70, 1, 'blocks'), (32, 40, 'two_in_three'),
                                         (70, 3, 'blocks'), (32, 10, 'none'), (70, 10, 'all')])
def test_block_mappings(be, GC, N, S, pattern):
    """S = 10: 3 rows per block (70 rows: the last block holds one); S = 1: 32 rows per block; S = 40: a row per block.  Blocks
    without a due row, with only their last or only their first row due, every row due and no row due."""
    G, clips = GC
    rows_per_block = 1 if S >= 32 else 32 // S
    reset = {'all': torch.ones(N, dtype=torch.int64), 'none': torch.zeros(N, dtype=torch.int64),
             'blocks': R.block_pattern(N, rows_per_block), 'two_in_three': R.reset_pattern(N)}[pattern].to(DEV)
    if pattern == 'blocks':
        per_block = [int(reset[i:i + rows_per_block].sum()) for i in range(0, N, rows_per_block)]
        assert 0 in per_block and 1 in per_block and max(per_block) > 1 and per_block[1] == 1 and int(reset[2 * rows_per_block - 1]) == 1
    a, want = _run(be, G, clips, (N, S, pattern), N=N, S=S, reset=reset)
    if pattern == 'none':                                      # nothing written but the plan's -1s, and the offset moved
        assert (want['env_ids'] == -1).all() and a.at.rng_state.tolist() == [R.SEED, 1]
        fresh = Copy(be, G, clips, N=N, S=S, reset=reset)
        for k in a.alloc:
            if not k.startswith('plan_') and k != 'rng_state':
                _same(a.alloc[k], fresh.alloc[k], ('none due', k))
    if pattern == 'all':
        assert (want['env_ids'] == torch.arange(N, device=DEV)).all()


def test_strided_simulator_tensors(be, GC):
    """dof_stride = 2 on the interleaved [N, D, 2] dof state and ld_root = 39: the contiguous result, gaps untouched."""
    G, clips = GC
    a, _ = _run(be, G, clips, 'strided', strided=True)
    D = G['num_dof']
    assert a.s['dof_pos'].stride() == (2 * D + 4, 2) and a.s['humanoid_root_states'].stride() == (39, 1)
    c = Copy(be, G, clips)
    c.reset_due()
    torch.cuda.synchronize()
    for k in STATE_KEYS:
        _same(a.s[k].contiguous(), c.s[k].contiguous(), ('strided against plain', k))
    _same(a.alloc['hist'], c.alloc['hist'], 'strided against plain, hist')
    assert a.alloc['dof_state'][:, D:].isnan().all() and a.alloc['actors'][:, 1:].isnan().all()


def test_reset_due_in_a_launch_program_follows_the_buffers(be, GC):
    """Recorded once, replayed three times with reset_buf rewritten: each replay equals an eager call at the same position."""
    G, clips = GC
    N = G['num_envs']
    a, b = Copy(be, G, clips), Copy(be, G, clips)
    before = {k: v.clone() for k, v in a.alloc.items()}
    prog = be.prog_create()
    be.prog_begin(prog)
    a.reset_due()
    be.prog_end(prog)
    torch.cuda.synchronize()
    assert be.prog_size(prog) == 2                             # the reset and the stream position
    for k in a.alloc:
        _same(a.alloc[k], before[k], ('recorded, not executed', k))
    resets = [R.reset_pattern(N), (torch.arange(N) % 5 == 2).to(torch.int64), torch.ones(N, dtype=torch.int64)]
    for i, reset in enumerate(resets):
        for c in (a, b):
            c.bufs['reset_buf'].copy_(reset)
            c.bufs['terminate_buf'].copy_((torch.arange(N) + i) % 2)
        want = b.ref_plan()
        be.prog_launch(prog)
        b.reset_due()
        torch.cuda.synchronize()
        assert a.at.rng_state.tolist() == [R.SEED, i + 1]
        for k in R.PLAN_KEYS:
            _same(a.at.plan[k], want[k], ('replay', i, k))
        _compare(a, b, ('replay', i))
    be.prog_destroy(prog)


def test_torch_op_equals_the_backend_call(be, GC):
    G, clips = GC
    a, b = Copy(be, G, clips), Copy(be, G, clips)
    a.reset_due()
    at, s, bufs = b.at, b.s, b.bufs
    c, tab, p = at._motion_lib.clips, at._table, at.plan
    out = torch.ops.ase_hip.amp_reset_due(s['humanoid_root_states'], s['dof_pos'], s['dof_vel'], at.amp_obs_buf, s['rigid_body_pos'],
                                          s['rigid_body_rot'], s['rigid_body_vel'], s['rigid_body_ang_vel'], bufs['reset_buf'],
                                          at.rng_state, bufs['progress_buf'], bufs['terminate_buf'], at.recovery_counter, p['env_ids'],
                                          p['kind'], p['motion_ids'], p['motion_times'], p['src_rows'], c['gts'], c['grs'], c['lrs'],
                                          c['grvs'], c['gravs'], c['dvs'], c['lengths'], c['num_frames'], c['dt'], c['length_starts'],
                                          at._motion_lib.clip_cdf, tab[0], tab[1], tab[2], c['dof_body_ids'], c['dof_offsets'],
                                          c['key_body_ids'], 'Hybrid', G['hybrid_init_prob'], True, G['recovery_episode_prob'],
                                          G['recovery_steps'], G['fall_init_prob'], G['local_root_obs'], G['root_height_obs'], G['dt'])
    torch.cuda.synchronize()
    assert out is None
    _compare(a, b, 'torch op')
    with pytest.raises(RuntimeError):                          # a plan export given in part
        torch.ops.ase_hip.amp_reset_due(s['humanoid_root_states'], s['dof_pos'], s['dof_vel'], at.amp_obs_buf, s['rigid_body_pos'],
                                        s['rigid_body_rot'], s['rigid_body_vel'], s['rigid_body_ang_vel'], bufs['reset_buf'],
                                        at.rng_state, bufs['progress_buf'], bufs['terminate_buf'], at.recovery_counter, p['env_ids'],
                                        None, p['motion_ids'], p['motion_times'], p['src_rows'], c['gts'], c['grs'], c['lrs'],
                                        c['grvs'], c['gravs'], c['dvs'], c['lengths'], c['num_frames'], c['dt'], c['length_starts'],
                                        at._motion_lib.clip_cdf, tab[0], tab[1], tab[2], c['dof_body_ids'], c['dof_offsets'],
                                        c['key_body_ids'], 'Hybrid', G['hybrid_init_prob'], True, G['recovery_episode_prob'],
                                        G['recovery_steps'], G['fall_init_prob'], G['local_root_obs'], G['root_height_obs'], G['dt'])


def test_reset_sequence_without_nonzero(be, GC, monkeypatch):
    """reset_due, then reset_task and latent_renew on the exported id list, under a Tensor.nonzero that raises - against
    apply_reset, reset_task and latent_renew given nonzero(reset_buf) as ids on a second copy."""
    G, clips = GC
    N, dim = G['num_envs'], 64
    copies = []
    for _ in range(2):
        c = Copy(be, G, clips)
        c.ht = HumanoidTensors(be, N, G['num_bodies'], task='heading', device=DEV, seed=R.SEED + 1)
        c.s.update(tar_dir=torch.full((N, 2), 0.25, device=DEV), tar_facing_dir=torch.full((N, 2), -0.5, device=DEV),
                   tar_speed=torch.full((N,), 3.0, device=DEV))
        c.latents = torch.full((N, dim), 0.125, device=DEV)
        c.latent_steps = torch.full((N,), 9, dtype=torch.int32, device=DEV)
        c.latent_rng = torch.tensor([R.SEED + 2, 4], dtype=torch.int64, device=DEV)
        copies.append(c)
    a, b = copies
    reset0 = a.bufs['reset_buf'].clone()
    want = b.ref_plan()

    def no_nonzero(*args, **kw):
        raise AssertionError('nonzero called in the device reset sequence')
    monkeypatch.setattr(torch.Tensor, 'nonzero', no_nonzero)
    plan = a.reset_due()
    a.ht.reset_task(a.s, plan['env_ids'], a.bufs['progress_buf'])
    be.latent_renew(a.latents, env_ids=plan['env_ids'], rng_state=a.latent_rng, reset_steps=a.latent_steps, steps_low=1, steps_high=150)
    monkeypatch.undo()
    ids = torch.nonzero(reset0).flatten().to(torch.int32)
    assert 0 < ids.numel() < N
    b.at.apply_reset(b.s, {k: v[ids.long()].contiguous() for k, v in want.items()}, b.bufs['progress_buf'], b.bufs['reset_buf'],
                     b.bufs['terminate_buf'])
    b.at.rng_state[1] += 1
    for k in R.PLAN_KEYS:
        b.at.plan[k].copy_(want[k])
    b.ht.reset_task(b.s, ids, b.bufs['progress_buf'])
    be.latent_renew(b.latents, env_ids=ids, rng_state=b.latent_rng, reset_steps=b.latent_steps, steps_low=1, steps_high=150)
    torch.cuda.synchronize()
    _compare(a, b, 'sequence')
    for k in ('tar_dir', 'tar_facing_dir', 'tar_speed'):
        _same(a.s[k], b.s[k], ('sequence', k))
    _same(a.ht.change_steps, b.ht.change_steps, 'change_steps')
    _same(a.latents, b.latents, 'latents')
    _same(a.latent_steps, b.latent_steps, 'latent steps')
    assert a.ht.rng_state.tolist() == b.ht.rng_state.tolist() == [R.SEED + 1, 1] and a.latent_rng.tolist() == b.latent_rng.tolist()
    due = reset0 != 0
    assert (a.s['tar_speed'][~due] == 3.0).all() and (a.s['tar_speed'][due] != 3.0).all()
    assert (a.latents[~due] == 0.125).all() and (a.latents[due] != 0.125).any(dim=-1).all()
