"""The agents' ``rollout_program`` without a GPU: one environment step recorded once as a launch program and
replayed horizon_length times, against ``device_rollout`` alone on an agent and an environment of the same seeds - every tensor
of the experience, both Philox streams, the latents, the episode accumulators, the id list and the meter words equal after each
of three rollouts, and the losses of the epoch that follows.  The emulator's programs (tests/emu_rollout_step.py) keep every
call made while recording as a closure and run nothing, so code that reads a result during recording fails here."""
import pytest
import torch

import tests.test_boundary_emu as T
from tests.emu_rollout_step import EmuRolloutStep

KINDS = ('ppo', 'amp', 'ase')
SEED = 3


def tiny(golden_dir, kind):
    G = T._load(golden_dir, kind)
    return dict(G, spec=dict(G['spec'], num_envs=64), cfg=dict(G['cfg'], horizon_length=4))


def pair(T, G, make_be, env=None, **extra):
    """(eager agent, program agent) from the same seed on environments of the same seed."""
    env = env or (lambda: T._env(G, seed=SEED))
    kw = dict(device_rollout=True, **(dict(device_latents=True) if G['kind'] == 'ase' else {}), **extra)
    torch.manual_seed(7)                                          # (the network's initial weights come from the global generator)
    a, _ = T._agent(G, env(), be=make_be(), **kw)
    torch.manual_seed(7)
    b, _ = T._agent(G, env(), be=make_be(), rollout_program=True, **kw)
    assert torch.equal(a.model.a2c_network.flat_params, b.model.a2c_network.flat_params)
    return a, b


def state(ag):
    s = {'E.' + k: v for k, v in ag.experience.items()}
    s.update(action_rng=ag.action_rng, current_rewards=ag.current_rewards, current_lengths=ag.current_lengths,
             done_ids=ag._done_ids, meter=ag._meter_words)
    if ag.kind == 'ase':
        s.update(rng_state=ag.engine.rng_state, ase_latents=ag._ase_latents, latent_reset_steps=ag._latent_reset_steps)
    return s


def assert_same_state(a, b, what):
    sa, sb = state(a), state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)


def check_fixture(ag, what):
    """At least one done row and one not-done row in the rollout; ASE: a latent renewed by the due test (a row that was not
    reset and whose latent changed between two steps)."""
    d = ag.experience['dones']
    assert bool((d != 0).any()) and bool((d == 0).any()), what
    if ag.kind == 'ase':
        z = ag.experience['ase_latents']
        changed = (z[1:] != z[:-1]).any(-1)
        assert bool((changed & (d[:-1] == 0)).any()), (what, 'no latent renewed by the due test')


_ADAM = ('adam_m', 'adam_v', 'opt_state')
_RING = ('_head', '_total_count', '_data', '_sample_idx', '_sample_head')


def snapshot(ag):
    """Everything an update reads and writes that a rollout does not: parameters, optimizer, running statistics and the engine's
    streams (the checkpoint), the agent's two generators, the dataset permutation, the demo and replay rings."""
    import copy
    rings = {}
    for name in ('_amp_obs_demo_buffer', '_amp_replay_buffer'):
        if hasattr(ag, name):
            rings[name] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(getattr(ag, name)).items() if k in _RING}
    return dict(ck=copy.deepcopy(ag.get_full_state_weights()), adam=[getattr(ag.engine, k).clone() for k in _ADAM], gen=ag._gen.get_state(), host_gen=ag._host_gen.get_state(),
                perm=ag.dataset_perm.clone(), rings=rings, last_lr=ag.last_lr, demo_ready=getattr(ag, '_demo_ready', None))


def restore(ag, snap):
    ag.set_full_state_weights(snap['ck'])
    for k, v in zip(_ADAM, snap['adam']):            # (a checkpoint taken before the first step carries no moments to load)
        getattr(ag.engine, k).copy_(v)
    ag._gen.set_state(snap['gen'])
    ag._host_gen.set_state(snap['host_gen'])
    ag.dataset_perm.copy_(snap['perm'])
    ag.last_lr = snap['last_lr']
    if snap['demo_ready'] is not None:
        ag._demo_ready = snap['demo_ready']
    for name, fields in snap['rings'].items():
        ring = getattr(ag, name)
        for k, v in fields.items():
            cur = getattr(ring, k)
            if torch.is_tensor(v):
                cur.copy_(v)
            elif not torch.is_tensor(cur):               # (a ring allocated by the first update keeps its storage: its count says empty)
                setattr(ring, k, v)


def epoch_on_one_engine(a, b, sync):
    """The epoch's losses on a's rollout and on b's, BOTH through a's engine from one checkpoint: the update is then the same
    launches on the same buffers twice, and what differs can only be the rollout's.  (Two engines add bias gradients and
    loss sums of several workgroups with atomics, csrc/heads.hip, whose arrival order follows the allocation layout: two
    updates on bitwise-equal inputs need not agree in the last bit.)"""
    snap = snapshot(a)
    for ag in (a, b):
        torch.manual_seed(103)
        batch = ag.play_steps() if ag is a else (ag.play_steps(), batch)[1]
    sync()
    assert_same_state(a, b, 'the fourth rollout')
    env = getattr(a.vec_env, 'env', a.vec_env)
    env_gen = env.gen.get_state()                        # the demo fetch of the update draws from the environment's generator
    streams = [t.clone() for t in (a.action_rng,) + ((a.engine.rng_state,) if a.kind == 'ase' else ())]
    ia = a.update(batch)
    ia = {k: [torch.as_tensor(v).clone() for v in vs] for k, vs in ia.items()}
    restore(a, snap)
    env.gen.set_state(env_gen)
    for t, v in zip((a.action_rng,) + ((a.engine.rng_state,) if a.kind == 'ase' else ()), streams):
        t.copy_(v)
    for k in a.experience:
        a.experience[k].copy_(b.experience[k])
    ib = a.update(a._play_steps_tail())
    sync()
    return ia, ib


def run_equal(T, G, make_be, sync=lambda: None, train=True, one_engine=False, **kw):
    a, b = pair(T, G, make_be, **kw)
    for ag in (a, b):
        if train:
            ag._init_train()
    for r in range(3):
        for ag in (a, b):
            torch.manual_seed(100 + r)                  # (HumanoidEnv's host reset path draws from the global generator)
            ag.play_steps()
        sync()
        check_fixture(a, f'rollout {r}')
        assert_same_state(a, b, f'rollout {r}')
    assert b._rp is not None and a._rp is None
    if not train:
        return a, b
    if one_engine:
        ia, ib = epoch_on_one_engine(a, b, sync)
    else:
        ia, ib = a.train_epoch(), b.train_epoch()
        sync()
        assert_same_state(a, b, 'the epoch')
    for k in ('actor_loss', 'critic_loss') + (('disc_loss',) if G['kind'] != 'ppo' else ()) + (('enc_loss',) if G['kind'] == 'ase' else ()):
        va, vb = [torch.as_tensor(v) for v in ia[k]], [torch.as_tensor(v) for v in ib[k]]
        assert len(va) == len(vb) > 0 and all(torch.equal(x, y) for x, y in zip(va, vb)), k
    return a, b


@pytest.mark.parametrize('kind', KINDS)
def test_program_rollouts_equal_the_device_rollouts(golden_dir, kind):
    run_equal(T, tiny(golden_dir, kind), EmuRolloutStep)


@pytest.mark.parametrize('kind', KINDS)
def test_epoch_on_one_engine_from_one_checkpoint(golden_dir, kind):
    """The form the GPU file compares the epoch in: both rollouts through one engine from one checkpoint.  On the emulator
    both forms hold."""
    run_equal(T, tiny(golden_dir, kind), EmuRolloutStep, one_engine=True)


@pytest.mark.parametrize('kind', KINDS)
def test_recorded_once_and_again_after_drop_graphs(golden_dir, kind):
    G = tiny(golden_dir, kind)
    a, b = pair(T, G, EmuRolloutStep)
    be = b.backend
    b.play_steps()
    assert be.prog_begins == 0 and b._rp is None                  # the first rollout is _play_steps_device, noting what env_step returns
    b.play_steps()
    assert be.prog_begins == 1
    size = be.prog_size(b._rp['prog'])
    b.play_steps()
    assert be.prog_begins == 1 and be.prog_size(b._rp['prog']) == size > 0
    steps = b.vec_env.steps
    assert steps == 3 * b.horizon_length                         # the environment is stepped exactly as often as on the eager path
    b._drop_graphs()
    assert b._rp is None and b._rp_notes is None
    b.play_steps()
    b.play_steps()
    assert be.prog_begins == 2 and be.prog_size(b._rp['prog']) == size
    assert b.vec_env.steps == 5 * b.horizon_length
    for _ in range(5):
        a.play_steps()
    assert_same_state(a, b, 'after a re-recording')


@pytest.mark.parametrize('kind', KINDS)
def test_replay_path_runs_no_nonzero_and_no_item(golden_dir, kind, monkeypatch):
    G = tiny(golden_dir, kind)
    _, b = pair(T, G, EmuRolloutStep)
    b.play_steps()
    b.play_steps()                                               # recorded

    def raising(*a, **kw):
        raise AssertionError('nonzero / item called on the replay path')
    monkeypatch.setattr(torch.Tensor, 'nonzero', raising)
    monkeypatch.setattr(torch.Tensor, 'item', raising)
    begins = b.backend.prog_begins
    b.play_steps()                                               # the whole of it: prologue, replays, meters, the tail
    monkeypatch.undo()
    assert b.backend.prog_begins == begins and int(b._rp['word']) == b.horizon_length


def test_library_calls_per_step(golden_dir):
    """The number of backend calls one step takes on both paths, counted on the emulator (DESIGN §6 quotes them)."""
    G = tiny(golden_dir, 'ase')
    a, b = pair(T, G, EmuRolloutStep)
    for ag in (a, b):
        ag.play_steps()
    n0 = len(a.backend.calls)
    a.play_steps()
    eager = (len(a.backend.calls) - n0) / a.horizon_length
    b.play_steps()
    recorded = b.backend.prog_size(b._rp['prog'])
    print('backend calls per step: eager', eager, 'recorded entries', recorded)
    assert recorded == 30 and eager * a.horizon_length == 139     # the figures DESIGN quotes for this fixture


def test_default_path_touches_no_new_entry(golden_dir):
    class Refusing(EmuRolloutStep):
        def rollout_head(self, *a, **kw):
            raise AssertionError('rollout_head called without rollout_program')

        def word_step(self, *a, **kw):
            raise AssertionError('word_step called without rollout_program')

        def prog_begin(self, *a, **kw):
            raise AssertionError('prog_begin called from play_steps without rollout_program')
    for kind in KINDS:
        G = tiny(golden_dir, kind)
        extra = dict(device_latents=True) if kind == 'ase' else {}
        for kw in ({}, dict(device_rollout=True, **extra)):
            ag, _ = T._agent(G, T._env(G, seed=SEED), be=Refusing(), **kw)
            assert ag._rollout_program is False
            ag.play_steps()
            ag.play_steps()


def test_refusals_at_construction(golden_dir):
    from tests.emu_rollout_store import EmuRolloutStore
    G = tiny(golden_dir, 'amp')
    with pytest.raises(AssertionError, match='rollout_program needs device_rollout'):
        T._agent(G, T._env(G), be=EmuRolloutStep(), rollout_program=True)
    with pytest.raises(AssertionError, match='rollout_program needs a backend with'):
        T._agent(G, T._env(G), be=EmuRolloutStore(), device_rollout=True, rollout_program=True)
    from ase_amd.learning.agents import HRLAgent
    with pytest.raises(AssertionError, match='HRL agent'):
        HRLAgent('t', dict(rollout_program=True, llc_config={}, llc_checkpoint='x'))
    # an environment that declares another device than the agent's
    env = T._env(G)
    env.device = torch.device('meta')
    with pytest.raises(AssertionError, match='the environment is on meta'):
        T._agent(G, env, be=EmuRolloutStep(), device_rollout=True, rollout_program=True)
    Gs = tiny(golden_dir, 'ase')
    env = T._env(Gs)
    env.progress_buf = env.progress_buf.to('meta')
    with pytest.raises(AssertionError, match='progress_buf is on meta'):
        T._agent(Gs, env, be=EmuRolloutStep(), device_rollout=True, device_latents=True, rollout_program=True)


def test_a_moved_progress_buf_raises(golden_dir):
    G = tiny(golden_dir, 'ase')
    _, b = pair(T, G, EmuRolloutStep)
    b.play_steps()
    b.play_steps()
    env = b.vec_env
    env.progress_buf = env.progress_buf.clone()
    steps, before = env.steps, {k: v.clone() for k, v in state(b).items()}
    with pytest.raises(RuntimeError, match='progress_buf moved'):
        b.play_steps()
    # a refused replay neither steps the environment nor stores
    assert env.steps == steps and b._rp['refused'] and int(b._rp['word']) < 0
    after = state(b)
    for k in before:
        if k != 'done_ids':                                      # (cleared by the rollout's prologue, before the first replay)
            assert torch.equal(before[k], after[k]), k


def test_a_refused_replay_on_the_program_emulation_of_the_device(golden_dir):
    """A backend that replays a program keeps a callback's exception and runs the rest of the program (HipBackend.host_call):
    the same refusal under that behaviour still steps nothing and stores nothing in the experience, the accumulators or the meters."""
    class KeepsGoing(EmuRolloutStep):
        def prog_launch(self, prog):
            err = None
            self._depth += 1
            try:
                for fn in self._progs[prog]:
                    try:
                        fn()
                    except BaseException as e:
                        err = err or e
            finally:
                self._depth -= 1
            if err is not None:
                raise err
    G = tiny(golden_dir, 'ase')
    _, b = pair(T, G, KeepsGoing)
    b.play_steps()
    b.play_steps()
    env = b.vec_env
    env.progress_buf = env.progress_buf.clone()
    steps, before = env.steps, {k: v.clone() for k, v in state(b).items()}
    with pytest.raises(RuntimeError, match='progress_buf moved'):
        b.play_steps()
    assert env.steps == steps
    after = state(b)
    # (launches that name no slot - the latent renewals, the policy pass and its draws - still ran once: the streams moved on)
    for k in before:
        if k.startswith('E.') or k in ('current_rewards', 'current_lengths', 'meter'):
            assert torch.equal(before[k], after[k]), k


# ---- HumanoidEnv over PlaybackPhysics: the fused step returns its own buffers (the skipped-copy branch, the address check) -------
def humanoid_env(env_be, dev):
    from tests import env_step_cases as CS
    Gf, clips, A = CS.load()
    return lambda: CS.make_env(env_be(), dev, Gf, clips, A, None, False, True, n=64)


def run_humanoid(T, golden_dir, make_be, env_be, dev, sync=lambda: None, train=True):
    G = tiny(golden_dir, 'amp')
    a, b = run_equal(T, G, make_be, sync=sync, train=train, env=humanoid_env(env_be, dev))
    stable = sorted(k for k, e in b._rp_notes.items() if e['stable'])
    assert 'obs' in stable and 'amp_obs' in stable and 'dones' not in stable, stable
    assert b._rp['step_obs'].data_ptr() == b.vec_env.obs_buf.data_ptr()            # read in place: no copy of the observation
    # an environment whose step hands out a fresh tensor where the recording saw a persistent one: refused, nothing stale stored
    step = b.vec_env.step

    def fresh(actions):
        obs, rewards, dones, infos = step(actions)
        return obs.clone(), rewards, dones, infos
    b.vec_env.step = fresh
    with pytest.raises(RuntimeError, match="env_step's obs was the environment's own storage"):
        b.play_steps()
    sync()


def test_humanoid_env_reads_the_environments_buffers_in_place(golden_dir):
    from tests.emu_env_step import EmuEnvStep
    # (no epoch here: without a GPU the fixture's motion library has no backend to fetch demo observations with)
    run_humanoid(T, golden_dir, EmuRolloutStep, EmuEnvStep, 'cpu', train=False)
