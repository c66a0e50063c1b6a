"""The projectile launches of the perturbation task on the MI355X: ``ase_hip_proj_launch`` through
``HipBackend``, ``ProjectileLauncher``, ``torch.ops.ase_hip.proj_launch`` and ``HumanoidEnv(perturb=True)`` against
tests/golden/perturb.pt and the f64 restatement tests/emu_perturb.py.

Every operand and output is a window of a NaN- / sentinel-filled allocation with wider strides; every guard word is checked
after each launch.  Floats are held to 2 e_ref + 2^-23 max |ref| + 1e-7 against f64 per group (position, velocity), e_ref =
what the reference's own f32 run loses: recorded in the fixture, and for shapes beyond it taken from the f32 stand-in (bitwise
the reference on the fixture) under the generator's cap of 16 f32 roundings of the group's largest output.  The constant
columns, untouched slots, actors and rows and the progress buffer are bitwise."""
import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd.perturb import ProjectileLauncher
from tests import emu_perturb as E
from tests import env_step_cases as CS
from tests import ref_perturb as RP
from tests import ref_rollout as RR

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENT, ISENT = -4321.5, -99
NAN, INF = float('nan'), float('inf')
SEED = (1 << 33) + 12345                                  # above 2^32: both key words of the stream are in use
OFFSETS = (0, (1 << 32) + 7)
PAD = 16                                                  # floats per root-state row of the allocation (13 used)


@pytest.fixture(scope='module')
def G():
    return E.load_fixture()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend(DEV)


@pytest.fixture(scope='module')
def fx():
    return CS.load()


class Case:
    """The operands of one launch sequence as windows of wider allocations on the device, and their host copies."""

    def __init__(self, n, K, A, B, root, body_pos, body_vel, packed=None, tar_body=1):
        self.n, self.K, self.A, self.B, self.tar_body = n, K, A, B, tar_body
        host = E.pattern(n + 2, A, PAD)
        if packed is not None:
            host[1:n + 1, :, :13] = packed.view(n, A, 13)
        host[1:n + 1, 0, :13] = root
        self.whole = host.to(DEV)
        self.win = self.whole[1:n + 1, :, :13]
        self.root, self.proj = self.win[:, 0], self.win[:, A - K:]
        self.bodies = {}
        for k, v in (('pos', body_pos), ('vel', body_vel)):
            w = torch.full((n + 2, B + 1, 5), NAN)
            w[1:n + 1, :B, :3] = v
            self.bodies[k] = w.to(DEV)
        self.body_pos, self.body_vel = (self.bodies[k][1:n + 1, :B, :3] for k in ('pos', 'vel'))
        self.progress_whole = torch.full((n + 2,), ISENT, dtype=torch.int64, device=DEV)
        self.progress = self.progress_whole[1:n + 1]
        self.slot_whole = torch.full((3,), ISENT, dtype=torch.int32, device=DEV)
        self.ids_whole = torch.full((n + 2,), ISENT, dtype=torch.int32, device=DEV)
        self.draws_whole = torch.full((n + 2, 7), SENT, device=DEV)
        self.slot_out, self.ids_out, self.draws_out = self.slot_whole[1:2], self.ids_whole[1:n + 1], self.draws_whole[1:n + 1]
        self.snapshot()

    def snapshot(self):
        self.before = self.whole.cpu().clone()
        self.bodies0 = {k: v.cpu().clone() for k, v in self.bodies.items()}
        self.progress0 = self.progress_whole.cpu().clone()

    def operands(self):
        return self.root, self.body_pos, self.body_vel, self.proj

    def exports(self):
        return dict(slot_out=self.slot_out, ids_out=self.ids_out, draws_out=self.draws_out)

    def draws_window(self, draws):
        """u [rows, 4] / eps [rows, 3] as windows of sentinel-framed allocations."""
        u, eps = RP.split(draws)
        out = []
        for t in (u, eps):
            w = torch.full((t.shape[0] + 2, t.shape[1]), SENT)
            w[1:-1] = t
            out.append(w.to(DEV)[1:-1])
        return out

    def guards_ok(self):
        n = self.n
        ok = bool((self.slot_whole[[0, 2]] == ISENT).all()) and bool((self.ids_whole[[0, n + 1]] == ISENT).all())
        ok = ok and bool((self.draws_whole[[0, n + 1]] == SENT).all())
        ok = ok and torch.equal(self.progress_whole.cpu(), self.progress0)            # the progress buffer is only read
        for k, v in self.bodies.items():
            ok = ok and torch.equal(torch.nan_to_num(v.cpu(), nan=7.0), torch.nan_to_num(self.bodies0[k], nan=7.0))
        return ok

    def expected(self, slot, ids, draws, dtype):
        """The stand-in on the host copies -> the projectile window [n, K, 13] after the launch, in dtype."""
        host = self.before.clone().to(dtype)
        win = host[1:self.n + 1, :, :13]
        bp, bv = (self.bodies0[k][1:self.n + 1, :self.B, :3] for k in ('pos', 'vel'))
        u, eps = RP.split(draws)
        E.EmuProjLaunch().proj_launch(win[:, 0], bp, bv, win[:, self.A - self.K:], slot=slot, u=u, eps=eps, tar_body=self.tar_body,
                                      env_ids=None if ids is None else torch.tensor(ids, dtype=torch.int32))
        return host

    def check(self, slot, ids, draws, what, e_ref=None):
        """The device result of one launch since the last snapshot: the written rows within the bar of f64, NaN / inf as the f32
        reference run has them, everything else - other slots, actors, rows, pad columns, the frame - bitwise the snapshot."""
        torch.cuda.synchronize()
        got = self.whole.cpu()
        n, K, A = self.n, self.K, self.A
        rows = list(range(n)) if ids is None else [e for e in ids if 0 <= e < n]
        if slot < 0:
            rows = []
        mask = torch.zeros(n + 2, A, PAD, dtype=torch.bool)
        for e in rows:
            mask[1 + e, A - K + slot, :13] = True
        same = torch.equal(torch.nan_to_num(got[~mask], nan=7.0), torch.nan_to_num(self.before[~mask], nan=7.0))
        assert same, (what, 'an element outside the launched rows changed')
        assert self.guards_ok(), (what, 'a guard word or a read-only operand changed')
        if not rows:
            return
        r32, r64 = self.expected(slot, ids, draws, torch.float32), self.expected(slot, ids, draws, torch.float64)
        g = got[1:n + 1, A - K + slot, :13][rows]
        a32, a64 = r32[1:n + 1, A - K + slot, :13][rows], r64[1:n + 1, A - K + slot, :13][rows]
        assert torch.equal(g[:, E.CONSTANT_COLS], E.CONSTANT.expand(len(rows), 7)), (what, 'constant columns')
        for name, cols in E.GROUPS.items():
            x, y32, y64 = g[:, cols].double(), a32[:, cols].double(), a64[:, cols]
            assert torch.equal(torch.isnan(x), torch.isnan(y32)) and torch.equal(torch.isnan(y32), torch.isnan(y64)), (what, name, 'NaN pattern')
            inf = torch.isinf(y64)
            assert torch.equal(x[inf], y64[inf]) and torch.equal(torch.isinf(x), inf), (what, name, 'infinite entries')
            fin = torch.isfinite(y64)
            if not fin.any():
                continue
            top = float(y64[fin].abs().max())
            own = float((y32[fin] - y64[fin]).abs().max())
            assert own <= 16 * 2.0 ** -24 * top, (what, name, 'the f32 restatement itself is beyond the cap')
            e = own if e_ref is None else e_ref[name]
            bar = 2.0 * e + 2.0 ** -23 * top + 1e-7
            err = float((x[fin] - y64[fin]).abs().max())
            print(f'{what}: max |hip - f64| {name} {err:.3g} (e_ref {e:.3g}, allowed {bar:.3g})')
            assert err <= bar, (what, name, err, bar)


def _inputs(n, B, seed=0):
    g = torch.Generator().manual_seed(1000 * n + B + seed)
    root = torch.randn(n, 13, generator=g)
    root[:, 0:3] = root[:, 0:3] * torch.tensor([3.0, 3.0, 0.1]) + torch.tensor([0.0, 0.0, 0.9])
    body_pos = root[:, None, 0:3] + 0.3 * torch.randn(n, B, 3, generator=g)
    return root, body_pos, 2.0 * torch.randn(n, B, 3, generator=g)


def _rng(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _ts(G):
    return E.timesteps_of(G).to(DEV)


# ---- 1. due mode on the recorded progress values --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('A14', 'A15'))
def test_due_mode_on_the_recorded_progress_values(be, G, name):
    case = G['cases'][name]
    A, n = case['actors'], G['num_envs']
    c = Case(n, 13, A, G['num_bodies'], G['root_states'], G['body_pos'], G['body_vel'], E.packed_before(G, A), G['tar_body'])
    for st in case['chain']:
        c.progress.fill_(st['progress'])
        c.slot_out.fill_(ISENT)
        c.ids_out.fill_(ISENT)
        c.snapshot()
        draws = st['draws'] if st['draws'] is not None else torch.full((n, 7), 0.5)
        u, eps = c.draws_window(draws)
        be.proj_launch(*c.operands(), progress_buf=c.progress, timesteps=_ts(G), u=u, eps=eps, tar_body=G['tar_body'],
                       slot_out=c.slot_out, ids_out=c.ids_out, **G['params'])
        c.check(st['slot'], None, draws, f'{name} progress {st["progress"]}', st['e_ref'])
        assert int(c.slot_out) == st['slot'] and c.ids_out.tolist() == ([-1] * n if st['slot'] < 0 else list(range(n)))
    # the tensor after the chain against the reference's own: the same bar, with the recorded e_ref
    got = c.win.cpu().reshape(n * A, 13)
    _, pg = E.views(G, got, A)
    _, pr = E.views(G, case['after'], A)
    _, p64 = E.views(G, E.replay(G, case, torch.float64), A)
    for st in case['chain']:
        if st['slot'] >= 0:
            for g, cols in E.GROUPS.items():
                ref64 = p64[:, st['slot'], cols]
                assert float((pg[:, st['slot'], cols].double() - ref64).abs().max()) <= E.allowance(st, g, ref64)
            assert torch.equal(pg[:, st['slot'], E.CONSTANT_COLS], pr[:, st['slot'], E.CONSTANT_COLS])
    others = [k for k in range(13) if k not in [st['slot'] for st in case['chain']]]
    assert torch.equal(pg[:, others], pr[:, others]) and torch.equal(got.view(n, A, 13)[:, :A - 13], case['after'].view(n, A, 13)[:, :A - 13])


def test_environment_zero_decides_for_all(be, G):
    n = 65
    c = Case(n, 13, 14, 3, *_inputs(n, 3))
    draws = RP.device_draws(range(n), SEED, 5)
    for p0, rest, want in ((60, 59, 0), (59, 60, -1), (489 + 128, 0, 10), (0, 488, -1)):
        c.progress.fill_(rest)
        c.progress[0] = p0
        c.snapshot()
        st = _rng(SEED, 5)
        be.proj_launch(*c.operands(), progress_buf=c.progress, timesteps=_ts(G), rng_state=st, **c.exports())
        c.check(want, None, draws, f'progress[0] {p0}, others {rest}')
        assert int(c.slot_out) == want and c.ids_out.tolist() == ([-1] * n if want < 0 else list(range(n))) and st.tolist() == [SEED, 6]


# ---- 2. shapes where it can go wrong --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', (1, 2))
@pytest.mark.parametrize('K', (1, 13))
@pytest.mark.parametrize('n', (1, 63, 64, 65, 130))
def test_every_slot_on_partial_waves_and_blocks(be, n, K, extra):
    """n of a lane, a wave less one, a wave, a wave and a lane, three blocks; one projectile and thirteen; one and two actors in
    front of them.  Every slot once on device draws, then an env_ids list with ids outside [0, n) (skipped, never
    dereferenced)."""
    A, B = K + extra, 4
    c = Case(n, K, A, B, *_inputs(n, B), tar_body=2)
    for slot in range(K):
        c.snapshot()
        st = _rng(SEED, slot)
        be.proj_launch(*c.operands(), slot=slot, rng_state=st, tar_body=2, **c.exports())
        c.check(slot, None, RP.device_draws(range(n), SEED, slot), f'n {n} K {K} A {A} slot {slot}')
        assert int(c.slot_out) == slot and c.ids_out.tolist() == list(range(n)) and st.tolist() == [SEED, slot + 1]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).tolist()
    ids = []
    for i, e in enumerate(perm[:max(1, (3 * n) // 4)]):
        ids.append(e)
        if i % 5 == 0:
            ids.append((-1, n, n + 5, -(1 << 31), (1 << 31) - 1)[(i // 5) % 5])
    c.snapshot()
    c.slot_out.fill_(ISENT)
    be.proj_launch(*c.operands(), slot=K - 1, env_ids=torch.tensor(ids, dtype=torch.int32, device=DEV), rng_state=_rng(SEED, 77), tar_body=2,
                   slot_out=c.slot_out)
    valid = [e if 0 <= e < n else 0 for e in ids]
    c.check(K - 1, ids, RP.device_draws(valid, SEED, 77), f'n {n} K {K} A {A} env_ids')
    assert int(c.slot_out) == K - 1


# ---- 3. device draws ------------------------------------------------------------------------------------------------------------
def test_device_draws_are_the_table_and_equal_a_passed_in_launch(be):
    n = 130
    for offset in OFFSETS:
        c = Case(n, 13, 14, 3, *_inputs(n, 3))
        st = _rng(SEED, offset)
        be.proj_launch(*c.operands(), slot=4, rng_state=st, **c.exports())
        torch.cuda.synchronize()
        d = c.draws_out.cpu()
        want32, want64 = RP.device_draws(range(n), SEED, offset), RP.device_draws(range(n), SEED, offset, torch.float64)
        assert torch.equal(d[:, list(RP.UNIFORM_J)], want32[:, list(RP.UNIFORM_J)]), offset          # uniforms: bitwise the table
        RR.within(d[:, list(RP.NORMAL_J)], want64[:, list(RP.NORMAL_J)], want32[:, list(RP.NORMAL_J)], f'normals offset {offset}')
        assert st.tolist() == [SEED, offset + 1] and c.guards_ok()
        # the same launch on the exported draws, passed in: the same bits; advance off leaves the stream position
        for advance in (None, False):
            t = Case(n, 13, 14, 3, *_inputs(n, 3))
            if advance is None:
                u, eps = t.draws_window(d)
                be.proj_launch(*t.operands(), slot=4, u=u, eps=eps, **t.exports())
            else:
                st2 = _rng(SEED, offset)
                be.proj_launch(*t.operands(), slot=4, rng_state=st2, advance=False, **t.exports())
                assert st2.tolist() == [SEED, offset]
            torch.cuda.synchronize()
            assert torch.equal(t.whole, c.whole) and torch.equal(t.draws_whole, c.draws_whole) and t.guards_ok()
        c.check(4, None, d, f'device draws offset {offset}')


# ---- 4. planted rows, NaN and inf -----------------------------------------------------------------------------------------------
def test_target_exactly_on_the_drawn_position_gives_the_body_velocity(be):
    """theta = 0, distance 4.5, height 1.125 are exact in f32 (cos 0 = 1, sin 0 = 0): with the target body there and zero noise
    the direction is 0 / max(0, 1e-12) = 0, so the velocity is the body's xy velocity and 0 in z."""
    n = 5
    root, bp, bv = _inputs(n, 3)
    root[:, 0] = torch.round(root[:, 0] * 4) / 4               # root x + 4.5 is then exact in f32, and so in f64
    draws = torch.zeros(n, 7)
    draws[:, 1], draws[:, 2], draws[:, 6] = 0.5, 0.5, 0.25
    bp[:, 1, 0], bp[:, 1, 1], bp[:, 1, 2] = root[:, 0] + 4.5, root[:, 1], 1.125
    c = Case(n, 2, 3, 3, root, bp, bv)
    u, eps = c.draws_window(draws)
    be.proj_launch(*c.operands(), slot=1, u=u, eps=eps, **c.exports())
    c.check(1, None, draws, 'planted row')
    row = c.proj.cpu()[:, 1]
    assert torch.equal(row[:, 0:3], bp[:, 1]) and torch.equal(row[:, 7:9], bv[:, 1, 0:2]) and not row[:, 9].any()


def test_nan_and_inf_operands_as_the_reference_has_them(be):
    n = 24
    root, bp, bv = _inputs(n, 3)
    vals = (NAN, INF, -INF)
    for i, v in enumerate(vals):
        root[i, 0], root[3 + i, 1], root[6 + i, 2] = v, v, v            # (root z is not read: those rows stay finite)
        bp[9 + i, 1, 0], bp[12 + i, 1, 2] = v, v
        bv[15 + i, 1, 0], bv[18 + i, 1, 2] = v, v                        # (the body's z velocity is not read)
        bp[21 + i, 0, 1], bv[21 + i, 2, 0] = v, v                        # another body: not read
    c = Case(n, 2, 3, 3, root, bp, bv)
    draws = RP.device_draws(range(n), SEED, 1)
    u, eps = c.draws_window(draws)
    be.proj_launch(*c.operands(), slot=0, u=u, eps=eps, **c.exports())
    c.check(0, None, draws, 'NaN / inf operands')
    row = c.proj.cpu()[:, 0]
    assert bool(torch.isnan(row[0, [0, 7, 8, 9]]).all()) and bool(torch.isfinite(row[0, [1, 2]]).all())     # NaN root x: x and the velocity
    assert bool(torch.isnan(row[1, 7:10]).any()) and float(row[1, 0]) == INF                                # inf / inf
    assert bool(torch.isfinite(row[6:9]).all()) and bool(torch.isfinite(row[18:24]).all())
    assert bool(torch.isnan(row[15, 7])) and bool(torch.isfinite(row[15, [8, 9]]).all()) and float(row[16, 7]) == INF


# ---- 5. the torch op and the launcher -------------------------------------------------------------------------------------------
def test_torch_op_equals_the_backend_call(be, G):
    n = 65
    p = G['params']
    ranges = [p[k] for k in ('dist_min', 'dist_max', 'h_min', 'h_max', 'speed_min', 'speed_max')]
    draws = RP.device_draws(range(n), SEED, 3)
    for mode in ('due', 'explicit passed in', 'ids'):
        a, b = Case(n, 13, 15, 3, *_inputs(n, 3)), Case(n, 13, 15, 3, *_inputs(n, 3))
        ra, rb = _rng(SEED, 2), _rng(SEED, 2)
        ids = torch.tensor([5, 64, -1, 0, 99], dtype=torch.int32, device=DEV)
        for c, r, op in ((a, ra, False), (b, rb, True)):
            c.progress.fill_(77)
            c.snapshot()
            u, eps = c.draws_window(draws)
            kw = dict(due=dict(progress_buf=c.progress, timesteps=_ts(G), slot=-1, rng_state=r),
                      ids=dict(slot=3, env_ids=ids, rng_state=r, ids_out=None))
            kw['explicit passed in'] = dict(slot=12, u=u, eps=eps)
            k = dict(dict(progress_buf=None, timesteps=None, env_ids=None, u=None, eps=None, rng_state=None), **c.exports())
            k.update(kw[mode])
            if op:
                torch.ops.ase_hip.proj_launch(*c.operands(), k['progress_buf'], k['timesteps'], k['slot'], k['env_ids'], k['u'], k['eps'],
                                              k['rng_state'], True, 1, ranges, p['noise'], k['slot_out'], k['ids_out'], k['draws_out'])
            else:
                be.proj_launch(*c.operands(), tar_body=1, **k, **p)
        torch.cuda.synchronize()
        assert torch.equal(a.whole, b.whole) and torch.equal(a.draws_whole, b.draws_whole) and torch.equal(a.ids_whole, b.ids_whole), mode
        assert torch.equal(a.slot_whole, b.slot_whole) and ra.tolist() == rb.tolist() and not torch.equal(a.whole.cpu(), a.before), mode
        assert a.guards_ok() and b.guards_ok()
    with pytest.raises(RuntimeError):
        torch.ops.ase_hip.proj_launch(*a.operands(), None, None, 0, None, None, None, ra, True, 1, ranges[:5], 0.1, None, None, None)
    with pytest.raises(NotImplementedError):
        torch.ops.ase_hip.proj_launch(*[t.cpu() for t in a.operands()], None, None, 0, None, None, None, ra.cpu(), True, 1, ranges, 0.1, None, None, None)


def test_backend_refuses_foreign_and_strided_tensors(be, G):
    c = Case(8, 2, 3, 3, *_inputs(8, 3))
    with pytest.raises(AssertionError, match='root_states must be a tensor on'):
        be.proj_launch(c.root.cpu(), c.body_pos, c.body_vel, c.proj, slot=0, rng_state=_rng(1, 0))
    with pytest.raises(AssertionError, match='rng_state must be a tensor on'):
        be.proj_launch(*c.operands(), slot=0, rng_state=_rng(1, 0).cpu())
    with pytest.raises(AssertionError, match='unit stride'):
        be.proj_launch(c.root, c.body_pos, c.body_vel, c.whole[1:9, 1:, 0:26:2], slot=0, rng_state=_rng(1, 0))
    with pytest.raises(AssertionError, match='beyond the 2 projectiles'):
        be.proj_launch(*c.operands(), slot=2, rng_state=_rng(1, 0))
    torch.cuda.synchronize()
    assert torch.equal(c.whole.cpu(), c.before)


def test_update_replays_in_a_launch_program(be, G):
    """update recorded once, replayed with progress_buf[0] rewritten in between: each replay launches what is due by the word
    it finds, on the stream position it finds; recording executes nothing."""
    n = 65
    a, b = Case(n, 13, 14, 3, *_inputs(n, 3)), Case(n, 13, 14, 3, *_inputs(n, 3))
    la, lb = ProjectileLauncher(be, n, seed=SEED), ProjectileLauncher(be, n, seed=SEED)
    state = lambda c: dict(humanoid_root_states=c.root, rigid_body_pos=c.body_pos, rigid_body_vel=c.body_vel, proj_states=c.proj)
    a.progress.fill_(60)
    prog = be.prog_create()
    be.prog_begin(prog)
    la.update(state(a), a.progress)
    be.prog_end(prog)
    torch.cuda.synchronize()
    try:
        assert 1 <= be.prog_size(prog) <= 2 and torch.equal(a.whole.cpu(), a.before) and la.rng_state.tolist() == [SEED, 0] and int(la.slot_word) == -1
        for k, (p0, want) in enumerate(((59, -1), (60, 0), (489 + 67, 1), (61, -1), (488, 12))):
            for c in (a, b):
                c.progress.fill_(3)
                c.progress[0] = p0
            a.snapshot()
            be.prog_launch(prog)
            lb.update(state(b), b.progress)
            torch.cuda.synchronize()
            assert int(la.slot_word) == int(lb.slot_word) == want and torch.equal(la.launch_ids, lb.launch_ids)
            assert la.rng_state.tolist() == lb.rng_state.tolist() == [SEED, k + 1] and torch.equal(a.whole, b.whole)
            a.check(want, None, RP.device_draws(range(n), SEED, k), f'replay {k}')
    finally:
        be.prog_destroy(prog)


# ---- 6. the environment and an agent --------------------------------------------------------------------------------------------
def test_env_fused_and_unfused_steps_agree_on_the_device(be, fx):
    Genv, clips, _ = fx
    runs = [E.run_env(E.make_env(be, 'cuda', Genv, clips, fused, n=64), 12, device='cuda') for fused in (True, False)]
    for k, (x, y) in enumerate(zip(*runs)):
        for key in x:
            same = torch.equal(torch.nan_to_num(x[key], nan=12345.0), torch.nan_to_num(y[key], nan=12345.0)) if x[key].dtype.is_floating_point \
                else torch.equal(x[key], y[key])
            assert same, f'step {k}: {key} differs between the fused and the unfused step'
    recs = runs[0]
    assert [int(r['slot']) for r in recs] == [-1] * 6 + [0] + [-1] * 5 and recs[-1]['rng'].tolist() == [6, 12]
    assert sum(int(r['dones'].sum()) for r in recs) >= 16 and not any(bool(r['terminate'].any()) for r in recs)
    # the launched rows against the host statement of the draws, on the state the launch read
    proj = recs[6]['proj'].cpu()
    assert not torch.equal(proj[:, 0], recs[5]['proj'].cpu()[:, 0]) and torch.equal(proj[:, 1:], recs[5]['proj'].cpu()[:, 1:])
    assert torch.equal(proj[:, 0, E.CONSTANT_COLS], E.CONSTANT.expand(64, 7)) and bool(torch.isfinite(proj).all())
    speed = (proj[:, 0, 7:10]).norm(dim=-1)
    assert bool((speed > 20).all()) and bool((speed < 60).all())


@pytest.fixture
def boundary(monkeypatch):
    import tests.test_boundary_emu as T
    from ase_amd.backend import HipBackend
    monkeypatch.setattr(T, '_DEV', 'cuda:0')
    monkeypatch.setattr(T, '_BE', lambda: HipBackend('cuda:0'))
    return T


def test_agent_epoch_on_the_perturbed_environment(be, fx, boundary, golden_dir):
    """64 environments, horizon 4, the tiny ASE nets with the device rollout: one train_epoch across a due step with finite
    losses; the projectile that came due is in flight in every environment."""
    T = boundary
    Genv, clips, _ = fx
    Gk = T._load(golden_dir, 'ase')
    Gk = dict(Gk, spec=dict(Gk['spec'], num_envs=64), cfg=dict(Gk['cfg'], horizon_length=4))
    env = E.make_env(be, 'cuda', Genv, clips, True, perturb=dict(objs=(2, 3)), K=2, n=64)
    ag, _ = T._agent(Gk, env, be=be, device_rollout=True, device_demo_fetch=True, device_latents=True)
    ag._init_train()
    info = ag.train_epoch()
    torch.cuda.synchronize()
    for k in ('actor_loss', 'critic_loss', 'disc_loss', 'enc_loss'):
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in info[k]), k
    ph = env.physics
    words = [w for _, w in ph.pushed_projectiles if w is not None]
    assert len(words) == 4 and env.launcher.rng_state.tolist()[1] == 4
    proj = ph.state['proj_states']
    assert bool(torch.isfinite(proj).all()) and float(proj[:, 0, 6].min()) == 1.0 and bool((proj[:, 0, 7:10].norm(dim=-1) > 20).all())


def test_player_evaluates_on_the_perturbed_environment(be, fx, boundary, golden_dir):
    """The use the task exists for: an ASEPlayer plays 64 environments under perturbation - episodes that time out after 11 steps,
    projectiles due at counter values 2 and 5 of environment 0's clock - with finite rewards, the launches pushed every step and the resets'
    re-push of all projectiles of the done rows."""
    T = boundary
    Genv, clips, _ = fx
    Gk = T._load(golden_dir, 'ase')
    Gk = dict(Gk, spec=dict(Gk['spec'], num_envs=64))
    env = E.make_env(be, 'cuda', Genv, clips, True, perturb=dict(objs=(2, 3)), K=2, n=64, episode_length=12)
    _, cfg = T._agent(Gk, env, be=be)
    pcfg = dict(cfg)
    pcfg.update(vec_env=env, env_info=None, backend=be, player={'games_num': 128, 'print_stats': False, 'deterministic': False})
    pl = T.PLAYERS['ase'](pcfg)
    pl.run()
    torch.cuda.synchronize()
    ph = env.physics
    assert pl.games_played >= 128 and pl.sum_steps >= 11 * 128 and pl.sum_rewards == pl.sum_rewards and abs(pl.sum_rewards) < float('inf')
    words = [w for _, w in ph.pushed_projectiles if w is not None]
    resets = [ids for ids, w in ph.pushed_projectiles if w is None]
    assert len(words) >= 22 and env.launcher.rng_state.tolist()[1] == len(words) and any(ids.numel() == 64 for ids in resets[1:])
    proj = ph.state['proj_states']
    assert bool(torch.isfinite(proj).all()) and bool((proj[:, :, 6] == 1.0).all()) and bool((proj[:, :, 7:10].norm(dim=-1) > 20).all())
