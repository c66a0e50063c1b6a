"""One environment step as two launches on the GPU: ``ase_hip_env_post_step`` / ``ase_hip_env_pre_step`` through
``HipBackend`` and ``torch.ops.ase_hip.*`` against the separate entries they fold (bit for bit, on contiguous copies of the same
state) and against the recorded reference under its own allowance (tests/golden/env_tensors.pt); ``HumanoidEnv`` with the fused
and the unfused step side by side; the agents on ``HumanoidEnv``.  Outputs are windows of sentinel-filled allocations and every
sentinel is checked after each launch.

Set ASE_ENV_STEP_REPORT to a file name to get the observed maxima, case counts and elements compared as JSON lines."""
import json
import math
import os

import pytest
import torch

import ase_amd.ops  # noqa: F401  (registers torch.ops.ase_hip.*)
from ase_amd import lib as L
from ase_amd.amp_env import action_to_pd_targets
from ase_amd.env_tensors import TASKS as KIND
from tests import env_step_cases as CS
from tests.emu_env_tensors import allowance, golden_obs_max, task_operands
from tests.test_env_step_emu import KEYS, _same

pytestmark = pytest.mark.gpu
SENT = -4321.5
REPORT = {'cases': 0, 'elements': 0, 'max_err': {}}


@pytest.fixture(scope='module')
def fx():
    return CS.load()


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    path = os.environ.get('ASE_ENV_STEP_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(REPORT) + '\n')


def _window(shape, dtype=torch.float32, lead=2):
    """A contiguous window [lead : lead + shape[0]] of a sentinel-filled allocation -> (window, whole allocation)."""
    whole = torch.full((shape[0] + 2 * lead,) + tuple(shape[1:]), SENT if dtype.is_floating_point else -99, dtype=dtype, device='cuda')
    return whole[lead:lead + shape[0]], whole


def _frame_ok(whole, n, lead=2):
    s = SENT if whole.dtype.is_floating_point else -99
    return bool((whole[:lead] == s).all() and (whole[lead + n:] == s).all())


def _state(G, n, B, seed):
    """Contiguous CPU state of n environments: the fixture's at 17 bodies, seeded unit-scale state otherwise."""
    i = {k: v.clone() for k, v in G['inputs'].items()}
    if B != 17:
        g = torch.Generator().manual_seed(seed)
        N = G['num_envs']
        q = torch.randn(N, B, 4, generator=g)
        i.update(body_pos=torch.randn(N, B, 3, generator=g), body_rot=q / q.norm(dim=-1, keepdim=True),
                 body_vel=torch.randn(N, B, 3, generator=g), body_ang_vel=torch.randn(N, B, 3, generator=g),
                 contact_forces=torch.randn(N, B, 3, generator=g) * (torch.rand(N, B, 1, generator=g) < 0.3),
                 termination_heights=torch.rand(B, generator=g) * 0.5)
    return {k: (v[:n].contiguous() if v.shape[:1] == (G['num_envs'],) else v) for k, v in i.items()}


def _post_case(be, G, clips, task, n, B, extra, S, local_root, task_obs, getup, clip=math.inf, check_ref=True):
    i = _state(G, n, B, seed=B)
    D = 31
    dof = CS.dof_state(G['num_envs'], D)[:n].contiguous()
    c = {k: v.cuda() for k, v in i.items()}                  # the contiguous copies the separate entries take
    p = {k: v.cuda() for k, v in CS.packed(i, dof, extra_body=bool(extra)).items()}
    rb, cfp = p['rigid_body_state'], p['contact_forces']
    v = dict(body_pos=rb[:, :B, 0:3], body_rot=rb[:, :B, 3:7], body_vel=rb[:, :B, 7:10], body_ang_vel=rb[:, :B, 10:13],
             contact_forces=cfp[:, :B], root_states=p['root_states'][:, 0], tar_states=p['root_states'][:, 1],
             tar_contact_forces=cfp[:, B] if extra else c['tar_contact_forces'])
    contact = [b for b in G['contact_body_ids'] if b < B] if B >= 17 else [B - 1]
    strike_ids = G['strike_body_ids'] if B >= 17 else [1, 2]
    F = 15 * B - 2
    kind = KIND[task]
    tcols = L.TASK_OBS_COLS[kind] if (task is not None and task_obs) else 0
    off, wide = 3, F + tcols + 8
    obs, obs_all = _window((n, wide))
    rew, rew_all = _window((n,))
    reset, reset_all = _window((n,), torch.int64)
    term, term_all = _window((n,), torch.int64)
    prog, prog_all = _window((n,), torch.int64)
    prog.copy_(c['progress_buf'])
    kw = dict(task_kind=kind, enable_task_obs=task_obs)
    iv = dict(c)
    iv.update(root_states=v['root_states'], tar_states=v['tar_states'], body_pos=v['body_pos'])
    if task is not None:
        ops = dict(task_operands(G, iv, task, 'rew'))
        if task_obs:
            ops.update(task_operands(G, iv, task, 'obs'))
        if 'body_pos' in ops:
            ops.pop('body_pos')
            kw['reach_body_id'] = ops.pop('body_id')
        kw.update(ops)
    if task == 'strike':
        kw.update(tar_contact_forces=v['tar_contact_forces'], strike_body_ids=strike_ids)
    counter = None
    if getup:
        counter = ((torch.arange(n) % 3 == 0).to(torch.int32) * 2).cuda()
        kw['recovery_counter'] = counter
    hist = hist0 = None
    keys, offs = clips['key_body_ids'], clips['dof_offsets']
    if S is not None:
        hist, hist_all = _window((n, S, 140))
        hist0 = torch.randn(n, S, 140, generator=torch.Generator().manual_seed(2)).cuda()
        hist.copy_(hist0)
        kw.update(hist=hist, dof_pos=p['dof_state'][:, :, 0], dof_vel=p['dof_state'][:, :, 1], dof_offsets=offs, key_body_ids=keys)
    be.env_post_step(v['body_pos'], v['body_rot'], v['body_vel'], v['body_ang_vel'], v['contact_forces'], prog, obs, rew, reset, term,
                     c['termination_heights'], contact, G['max_episode_length'], True, local_root, True, col_offset=off, clip_obs=clip,
                     **kw)
    torch.cuda.synchronize()
    # ---- every sentinel
    assert _frame_ok(obs_all, n) and _frame_ok(rew_all, n) and _frame_ok(reset_all, n) and _frame_ok(term_all, n) and _frame_ok(prog_all, n)
    assert (obs[:, :off] == SENT).all() and (obs[:, off + F + tcols:] == SENT).all()
    assert S is None or _frame_ok(hist_all, n)
    # ---- the separate entries on contiguous copies
    assert torch.equal(prog, c['progress_buf'] + 1)
    want = torch.full((n, F + tcols), SENT, device='cuda')
    be.humanoid_obs_max(c['body_pos'], c['body_rot'], c['body_vel'], c['body_ang_vel'], local_root, True, want, 0)
    w_rew = torch.ones(n, device='cuda')
    if task is not None:
        if task_obs:
            be.task_obs(kind, want, F, None, **task_operands(G, c, task, 'obs'))
        be.task_reward(kind, w_rew, **task_operands(G, c, task, 'rew'))
    got = obs[:, off:off + F + tcols]
    w_obs = want.clamp(-clip, clip)
    assert torch.equal(torch.isnan(got), torch.isnan(w_obs)) and torch.equal(got.nan_to_num(nan=SENT), w_obs.nan_to_num(nan=SENT))
    assert torch.equal(rew, w_rew)
    w_reset, w_term = torch.zeros_like(reset), torch.zeros_like(term)
    be.humanoid_reset(prog.clone(), c['contact_forces'], c['body_pos'], c['termination_heights'], contact, G['max_episode_length'], True,
                      w_reset, w_term, c['tar_contact_forces'] if task == 'strike' else None, strike_ids if task == 'strike' else None)
    if getup:
        w_reset.masked_fill_(counter > 0, 0)
        w_term.masked_fill_(counter > 0, 0)
    assert torch.equal(reset, w_reset) and torch.equal(term, w_term)
    elements = got.numel() + 3 * n
    if S is not None:
        w_hist = hist0.clone()
        be.build_amp_obs(c['body_pos'][:, 0].contiguous(), c['body_rot'][:, 0].contiguous(), c['body_vel'][:, 0].contiguous(),
                         c['body_ang_vel'][:, 0].contiguous(), dof[:, :, 0].contiguous().cuda(), dof[:, :, 1].contiguous().cuda(),
                         c['body_pos'][:, keys].contiguous(), offs, local_root, True, w_hist, shift=True)
        assert torch.equal(hist, w_hist)
        elements += hist.numel()
    # ---- the recorded reference, under its own allowance
    if check_ref and B == 17 and clip == math.inf:
        refs = [('obs_max', got[:, :F], golden_obs_max(G, 'f64', local_root, True)[:n])]
        if task is not None:
            refs.append((f'{task}_rew', rew, G['f64'][f'{task}_rew'][:n]))
            if task_obs:
                refs.append((f'{task}_obs', got[:, F:], G['f64'][f'{task}_obs'][:n]))
        for name, x, ref in refs:
            err = float((x.double().cpu() - ref).abs().max())
            print(f'{name} n={n}: max |fused - f64 reference| = {err:.3g}, allowance {allowance(G, name):.3g}')
            REPORT['max_err'][name] = max(REPORT['max_err'].get(name, 0.0), err)
            assert err <= allowance(G, name), (name, err)
    REPORT['cases'] += 1
    REPORT['elements'] += elements
    return dict(obs=obs, kw=kw, v=v, c=c, prog0=c['progress_buf'], contact=contact, off=off)


# (n, bodies, extra body per environment, history steps, local_root_obs, enable_task_obs, getup)
SHAPES = [(96, 17, 1, 10, True, True, False), (70, 17, 0, 2, False, True, True), (1, 17, 1, 1, True, True, False),
          (96, 17, 0, None, True, True, True), (70, 17, 1, 10, False, False, False)]


@pytest.mark.parametrize('task', CS.TASKS)
def test_post_step_is_the_separate_entries(be, fx, task):
    G, clips, _ = fx
    for n, B, extra, S, local_root, task_obs, getup in SHAPES:
        if task == 'strike' and not extra:
            extra = 1
        _post_case(be, G, clips, task, n, B, extra, S, local_root, task_obs and task is not None, getup)


@pytest.mark.parametrize('B,S', [(5, None), (24, 2), (64, 10)])
@pytest.mark.parametrize('task', [None, 'strike'])
def test_post_step_body_counts(be, fx, task, B, S):
    G, clips, _ = fx
    for n, extra in ((70, 1), (96, 0), (1, 1)):
        _post_case(be, G, clips, task, n, B, 1 if task == 'strike' else extra, S, True, task is not None, True)


def test_post_step_clip_keeps_nan(be, fx):
    G, clips, _ = fx
    r = _post_case(be, G, clips, 'heading', 96, 17, 1, 2, True, True, False, clip=5.0)      # clamp == eager torch.clamp, bitwise
    # a NaN body position stays NaN through the clip; +-100 become +-5 bitwise
    G2 = dict(G)
    G2['inputs'] = {k: v.clone() for k, v in G['inputs'].items()}
    G2['inputs']['body_pos'][3, 4, 1] = float('nan')
    G2['inputs']['body_vel'][5, 2] = torch.tensor([100.0, -100.0, 100.0])
    r = _post_case(be, G2, clips, None, 96, 17, 1, None, True, False, False, clip=5.0, check_ref=False)
    row = r['obs'][:, r['off']:r['off'] + 253]
    assert torch.isnan(row[3]).any() and not torch.isnan(row[4]).any()
    vel = row[5, 1 + 48 + 102 + 6: 1 + 48 + 102 + 9]
    assert (vel.abs() <= 5.0).all() and (vel.abs() == 5.0).any() and float(row.nan_to_num().abs().max()) == 5.0


@pytest.mark.parametrize('pd', [True, False])
def test_pre_step(be, pd):
    g = torch.Generator().manual_seed(4)
    n, D = 70, 31
    wide_all = torch.randn(n, D + 5, generator=g) * 1.2
    wide_all[0, 2:8] = torch.tensor([1.0, -1.0, 1.5, -1.5, float('nan'), -0.0])
    wide = wide_all.cuda()
    a_in = wide[:, 2:2 + D]                                               # a view with a pitch wider than its width
    off, sc, eff = (torch.randn(D, generator=g).cuda(), (torch.rand(D, generator=g) + 0.5).cuda(), (torch.rand(D, generator=g) * 50).cuda())
    roots = torch.randn(n, 2, 13, generator=g).cuda()
    rs = roots[:, 0]
    acts, acts_all = _window((n, D))
    tg, tg_all = _window((n, D))
    prev, prev_all = _window((n, 3))
    cnt, cnt_all = _window((n,), torch.int32)
    cnt.copy_(torch.tensor([0, 1, 5], dtype=torch.int32).repeat(n // 3 + 1)[:n])
    cnt0 = cnt.clone()
    kw = dict(pd_offset=off, pd_scale=sc) if pd else dict(motor_efforts=eff)
    be.env_pre_step(a_in, acts, tg, 1.0, power_scale=0.75, root_states=rs, prev_root_pos=prev, recovery_counter=cnt, **kw)
    torch.cuda.synchronize()
    assert all(_frame_ok(w, n) for w in (acts_all, tg_all, prev_all, cnt_all))
    bits = lambda t: t.contiguous().view(torch.int32)
    want = torch.clamp(a_in, -1.0, 1.0)
    assert torch.equal(bits(acts), bits(want)) and torch.isnan(acts[0, 4]) and int(bits(acts)[0, 5]) == -2147483648
    w_t = action_to_pd_targets(want, off, sc) if pd else want * eff.unsqueeze(0) * 0.75
    assert torch.equal(bits(tg), bits(w_t))
    assert torch.equal(bits(prev), bits(rs[:, 0:3])) and torch.equal(cnt, (cnt0 - 1).clamp_min(0))
    assert torch.equal(wide.cpu().view(torch.int32), wide_all.view(torch.int32))         # the input is only read
    # reach: prev_root_pos and the counter are not given and not touched; the torch.ops form gives the same bits
    acts2, tg2 = torch.zeros(n, D).cuda(), torch.zeros(n, D).cuda()
    before = prev_all.clone()
    torch.ops.ase_hip.env_pre_step(a_in, acts2, tg2, 1.0, off if pd else None, sc if pd else None, None if pd else eff, 0.75, None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(bits(acts2), bits(acts)) and torch.equal(bits(tg2), bits(tg)) and torch.equal(prev_all, before)


def test_torch_ops_post_step_gives_the_same_bits(be, fx):
    G, clips, _ = fx
    r = _post_case(be, G, clips, 'strike', 96, 17, 1, 10, True, True, True)
    v, c, kw, n = r['v'], r['c'], r['kw'], 96
    obs = torch.full_like(r['obs'], SENT)
    rew, reset, term = torch.zeros(n).cuda(), torch.zeros(n, dtype=torch.int64).cuda(), torch.zeros(n, dtype=torch.int64).cuda()
    prog = r['prog0'].clone()
    hist = torch.randn(n, 10, 140, generator=torch.Generator().manual_seed(2)).cuda()
    torch.ops.ase_hip.env_post_step(v['body_pos'], v['body_rot'], v['body_vel'], v['body_ang_vel'], v['contact_forces'], prog, obs, rew,
                                    reset, term, c['termination_heights'], r['contact'], G['max_episode_length'], True, True, True,
                                    r['off'], math.inf, 'strike', True, kw['root_states'], kw['prev_root_pos'], None, None, None, 0.0,
                                    kw['tar_states'], 0, kw['dt'], kw['tar_contact_forces'], kw['strike_body_ids'],
                                    kw['recovery_counter'], hist, kw['dof_pos'], kw['dof_vel'], kw['dof_offsets'], kw['key_body_ids'])
    torch.cuda.synchronize()
    assert torch.equal(obs, r['obs']) and torch.equal(hist, kw['hist']) and torch.equal(prog, r['prog0'] + 1)


def test_bad_arguments_name_the_entry(be, fx):
    G, clips, _ = fx
    n = 8
    z = lambda *s: torch.zeros(*s).cuda()
    zi = lambda: torch.zeros(n, dtype=torch.int64).cuda()

    def post(B=17, **kw):
        args = dict(body_pos=z(n, B, 3), body_rot=z(n, B, 4), body_vel=z(n, B, 3), body_ang_vel=z(n, B, 3), contact_forces=z(n, B, 3))
        args.update({k: kw.pop(k) for k in list(kw) if k in args})
        be.env_post_step(args['body_pos'], args['body_rot'], args['body_vel'], args['body_ang_vel'], args['contact_forces'], zi(),
                         z(n, 15 * B + 20), z(n), zi(), zi(), z(B), [], 300.0, True, True, True, **kw)
    with pytest.raises(L.AseHipError, match='env_post_step.*bodies'):
        post(B=65)
    with pytest.raises(L.AseHipError, match='env_post_step.*needs tar_a'):
        post(task_kind=L.TASK_HEADING, root_states=z(n, 13), prev_root_pos=z(n, 3), tar_b=z(n, 2), tar_speed=z(n), dt=0.1)
    offs = list(range(0, 3 * 33, 3))                                                   # 32 joints of 3 dofs: F = 13 + 192 + 96 > 255
    with pytest.raises(L.AseHipError, match='env_post_step.*255'):
        post(hist=z(n, 2, 13 + 6 * 32 + 96), dof_pos=z(n, 96), dof_vel=z(n, 96), dof_offsets=offs, key_body_ids=[])
    with pytest.raises(L.AseHipError, match='env_pre_step'):
        be.env_pre_step(z(n, 4), z(n, 4), z(n, 4), -1.0, motor_efforts=z(4))


def test_post_step_refuses_an_element_stride_below_the_element(be):
    n, B = 8, 17
    z = lambda *s: torch.zeros(*s).cuda()
    zi = lambda: torch.zeros(n, dtype=torch.int64).cuda()
    narrow = torch.as_strided(z(n * B * 4), (n, B, 4), (B * 3, 3, 1))                  # rotations at the pitch of positions
    with pytest.raises(L.AseHipError, match='env_post_step.*element stride'):
        be.env_post_step(z(n, B, 3), narrow, z(n, B, 3), z(n, B, 3), z(n, B, 3), zi(), z(n, 300), z(n), zi(), zi(), z(B), [], 300.0,
                         True, True, True)


@pytest.mark.parametrize('device_resets', [False, True])
@pytest.mark.parametrize('task,getup', [(None, True), ('heading', False), ('strike', True)])
def test_env_fused_and_unfused_steps_agree_on_the_device(be, fx, task, getup, device_resets):
    G, clips, A = fx
    runs = []
    for fused in (True, False):
        env = CS.make_env(be, 'cuda', G, clips, A, task, getup, fused)
        runs.append(CS.run(env, 12, device_resets, device='cuda') + (env,))
    assert torch.equal(runs[0][0], runs[1][0])
    _same(runs[0][1], runs[1][1], KEYS)
    recs = runs[0][1]
    assert sum(int((r['terminate'] != 0).sum()) for r in recs) >= 8
    assert sum(int(((r['dones'] != 0) & (r['terminate'] == 0)).sum()) for r in recs) >= 8


def test_both_entries_replay_from_a_launch_program(be, fx):
    G, clips, A = fx
    env = CS.make_env(be, 'cuda', G, clips, A, 'location', False, True)
    ref = CS.make_env(be, 'cuda', G, clips, A, 'location', False, True)
    n, D = env.num_envs, 31
    for e in (env, ref):
        torch.manual_seed(17)
        e.reset()
    acts = CS.actions_of(0, n, D).cuda()
    prog = be.prog_create()
    be.prog_begin(prog)
    env.pre_physics_step(acts)
    env.post_physics_step()
    be.prog_end(prog)
    assert 3 <= be.prog_size(prog) <= 4                       # env_pre_step, the task's update (one or two entries), env_post_step
    try:
        for k in range(3):                                    # the replay follows progress_buf and the buffers' contents
            acts.copy_(CS.actions_of(k, n, D).cuda())
            env.physics.step()
            be.prog_launch(prog)
            ref.physics.step()
            ref.pre_physics_step(acts)
            ref.post_physics_step()
            torch.cuda.synchronize()
            assert torch.equal(env.progress_buf, ref.progress_buf) and int(env.progress_buf[0]) == k + 1
            assert torch.equal(env.obs_buf, ref.obs_buf) and torch.equal(env.reset_buf, ref.reset_buf)
            assert torch.equal(env.amp.amp_obs_buf, ref.amp.amp_obs_buf) and torch.equal(env.targets, ref.targets)
    finally:
        be.prog_destroy(prog)


# ---- the agents on HumanoidEnv -------------------------------------------------------------------------------------------------
@pytest.fixture
def boundary(monkeypatch):
    import tests.test_boundary_emu as T
    from ase_amd.backend import HipBackend
    monkeypatch.setattr(T, '_DEV', 'cuda:0')
    monkeypatch.setattr(T, '_BE', lambda: HipBackend('cuda:0'))
    return T


@pytest.mark.parametrize('device_mode', [False, True])
@pytest.mark.parametrize('kind', ('amp', 'ase'))
def test_agents_train_on_humanoid_env(be, fx, boundary, golden_dir, kind, device_mode):
    """64 environments, horizon 4, the tiny nets: two train_epochs with finite losses, and the experience buffer holds the bits the
    environment handed out at each step."""
    T = boundary
    Gf, clips, A = fx
    G = T._load(golden_dir, kind)
    G = dict(G, spec=dict(G['spec'], num_envs=64), cfg=dict(G['cfg'], horizon_length=4))
    env = CS.make_env(be, 'cuda', Gf, clips, A, None, False, True, n=64)
    extra = {}
    if device_mode:
        extra = dict(device_rollout=True, device_demo_fetch=True)
        if kind == 'ase':
            extra['device_latents'] = True
    seen, last = [], {}
    step, reset, reset_done = env.step, env.reset, env.reset_done

    def rec_step(actions):
        out = step(actions)
        seen.append(dict(before=last['obs'], obs=out[0].clone(), amp_obs=out[3]['amp_obs'].clone(), dones=out[2].clone()))
        return out

    def rec_reset(env_ids=None):
        last['obs'] = reset(env_ids).clone()
        return last['obs']

    def rec_reset_done(mask=None):
        last['obs'] = reset_done(mask).clone()
        return last['obs']
    env.step, env.reset, env.reset_done = rec_step, rec_reset, rec_reset_done
    ag, _ = T._agent(G, env, be=be, **extra)
    ag._init_train()
    for _ in range(2):
        info = ag.train_epoch()
        torch.cuda.synchronize()
        for k in ('actor_loss', 'critic_loss', 'disc_loss') + (('enc_loss',) if kind == 'ase' else ()):
            assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in info[k]), k
    assert len(seen) == 8 and (1 if device_mode else 0) <= len(env.physics.pushed)
    W = env.observation_space.shape[0]
    for n, s in enumerate(seen[-4:]):
        E = ag.experience
        assert torch.equal(E['obses'][n][:, :W], s['before']), f'obses {n}'
        assert torch.equal(E['next_obses'][n][:, :W], s['obs']), f'next_obses {n}'
        assert torch.equal(E['amp_obs'][n], s['amp_obs']), f'amp_obs {n}'
        assert torch.equal(E['dones'][n].to(torch.int64), s['dones']), f'dones {n}'
    assert sum(int(s['dones'].sum()) for s in seen) > 0
