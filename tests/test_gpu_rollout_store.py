"""The one-launch rollout step on the MI355X: ``ase_hip_rollout_store`` through ``HipBackend``,
``torch.ops.ase_hip.rollout_store``, a launch program and the agents' ``device_rollout``.

The bars (tests/ref_rollout_store.py): the copies, the shaped reward, the done flags, the masked next value, both accumulators and
the id list BITWISE the f32 run of the reference's lines, NaN pattern included, inside sentinel-filled allocations whose every
guard word is looked at after each launch; the meters against the f64 restatement of AverageMeter.update at
(k + 8) 2^-53 max(|previous mean|, max |x|) per call and accumulated, their integer words exactly, and against
``agents.AverageMeter`` in f32 at 2 e_ref + 2^-23 max |ref|.  ASE_ROLLOUT_STORE_REPORT=<file> writes the observed maxima and
the counts (for COVERAGE.md N12).

Observed on one MI355X (COVERAGE.md row N12): 38 tests in under 5 s - 153 checked calls, 4 415 133 elements compared, 0 not
bitwise equal, 5 056 128 guard words; meters over 140 calls: max |hip - f64| 0 (sums of at most 130 f32 values are exact in f64),
|hip - f32 meter| 7.5e-06 at e_ref 7.5e-06."""
import json
import os

import pytest
import torch

from tests import ref_rollout_store as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    yield HipBackend('cuda:0')
    out = os.environ.get('ASE_ROLLOUT_STORE_REPORT')
    if out:
        with open(out, 'w') as f:
            json.dump(R.report(), f, indent=1)


def test_widths_pitches_and_paths(be):
    R.check_widths(be, DEV)


@pytest.mark.parametrize('n', R.N_ENVS)
def test_done_patterns_at_every_size(be, n):
    R.check_n_envs(be, DEV, n)


@pytest.mark.parametrize('n_fields', (0, 1, 16))
def test_field_counts(be, n_fields):
    R.check_n_fields(be, DEV, n_fields)


@pytest.mark.parametrize('term_dtype', R.KINDS)
@pytest.mark.parametrize('dones_dtype', R.KINDS)
def test_flag_kinds(be, dones_dtype, term_dtype):
    R.check_kinds(be, DEV, dones_dtype, term_dtype)


def test_non_finite_rewards(be):
    R.check_special(be, DEV)


def test_nullable_groups(be):
    R.check_groups(be, DEV)


def test_device_slot_word(be):
    R.check_slot_word(be, DEV)


@pytest.mark.parametrize('start_size', (0, 60))
@pytest.mark.parametrize('n', (257, 1030))
def test_meter_sequences(be, n, start_size):
    """Six calls that meet the fixture conditions, per call and accumulated; the same sequence twice: bitwise-equal meters."""
    h1 = R.run_meter_sequence(be, DEV, n, start_size)
    h2 = R.run_meter_sequence(be, DEV, n, start_size)
    assert [R.bits(torch.tensor(w, dtype=R.F64)).tolist() for w in h1] == [R.bits(torch.tensor(w, dtype=R.F64)).tolist() for w in h2]


def test_launch_program_follows_the_slot_word(be):
    """Recorded once - recording executes nothing -, replayed twice with the slot word and the inputs rewritten in between:
    each replay is the reference's step at the slot it finds, and bitwise the eager call of a twin."""
    fields = [(3, 0, False), (64, 0, False), (253, 7, False)]
    st, twin = R.Step(DEV, 257, n_slots=3, fields=fields, seed=81), R.Step(DEV, 257, n_slots=3, fields=fields, seed=81)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    prog = be.prog_create()
    be.prog_begin(prog)
    try:
        be.rollout_store(st.d_dones, **st.kwargs(0, -0.5, 0.01, slot_dev=word))
    finally:
        be.prog_end(prog)
    torch.cuda.synchronize()
    assert be.prog_size(prog) == 2                               # the store and the fold
    st.untouched('recording')
    for v in (2, 0):
        word.fill_(v)
        for s in (st, twin):
            s.inputs(R.done_pattern('random', s.n, s.gen))
        ref, w0, w = st.run(be, 0, -0.5, 0.01, slot_dev=word, word=v, what=f'replay at slot {v}',
                            call=lambda dones, **kw: be.prog_launch(prog))
        R.check_meter(w0, w, ref)
        twin.run(be, v, -0.5, 0.01, what=f'eager twin at slot {v}')
        for a, b in zip(st.guarded(), twin.guarded()):
            R.same(a.alloc, b.alloc, f'replay against the eager call, slot {v}')
    be.prog_destroy(prog)


def test_torch_op_equals_the_backend_call(be):
    import ase_amd.ops  # noqa: F401
    fields = [(31, 0, False), (64, 0, False)]
    st, twin = R.Step(DEV, 65, n_slots=2, fields=fields, seed=91), R.Step(DEV, 65, n_slots=2, fields=fields, seed=91)

    def op(dones, slot, n_slots, fields, shift, scale, slot_dev, rewards, rewards_out, dones_out, next_values, terminate,
           next_values_out, cur_rewards, cur_lengths, meter, max_size, done_ids_out):
        torch.ops.ase_hip.rollout_store(dones, slot, n_slots, [f[0] for f in fields], [f[1] for f in fields], rewards, shift, scale,
                                        rewards_out, dones_out, next_values, terminate, next_values_out, cur_rewards, cur_lengths,
                                        meter, max_size, done_ids_out, slot_dev)
    ref, w0, w = st.run(be, 1, -0.5, 0.01, what='torch op', call=op)
    R.check_meter(w0, w, ref)
    twin.run(be, 1, -0.5, 0.01, what='backend call')
    for a, b in zip(st.guarded(), twin.guarded()):
        R.same(a.alloc, b.alloc, 'torch op against the backend call')


# ---- the agents ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def boundary(monkeypatch):
    import tests.test_boundary_emu as T
    from ase_amd.backend import HipBackend
    monkeypatch.setattr(T, '_DEV', 'cuda:0')
    monkeypatch.setattr(T, '_BE', lambda: HipBackend('cuda:0'))
    return T


@pytest.mark.parametrize('kind', ('amp', 'ase'))
def test_agent_trains_an_epoch_without_nonzero(boundary, golden_dir, monkeypatch, kind):
    """64 environments, horizon 4, the tiny nets: device_rollout on SyntheticVecEnv under a nonzero that raises, one train_epoch
    to the end with finite losses; the experience's done flags, the id list and the meter's episode count agree."""
    T = boundary
    G = T._load(golden_dir, kind)
    G = dict(G, spec=dict(G['spec'], num_envs=64), cfg=dict(G['cfg'], horizon_length=4))
    env = T._env(G)
    extra = dict(device_latents=True) if kind == 'ase' else {}
    ag, _ = T._agent(G, env, device_rollout=True, **extra)
    ag._init_train()

    def raising(*a, **kw):
        raise AssertionError('nonzero called with device_rollout')
    monkeypatch.setattr(torch.Tensor, 'nonzero', raising)
    info = ag.train_epoch()
    torch.cuda.synchronize()
    monkeypatch.undo()
    for k in ('actor_loss', 'critic_loss', 'disc_loss') + (('enc_loss',) if kind == 'ase' else ()):
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in info[k]), k
    dones = ag.experience['dones']
    assert dones.shape == (4, 64) and int(ag._meter_words[3]) == int(dones.sum()) > 0
    rows = torch.arange(64, dtype=torch.int32, device=dones.device)
    assert torch.equal(ag._done_ids, torch.where(dones[-1] != 0, rows, torch.full_like(rows, -1)))
    assert ag.game_rewards.current_size == min(int(dones.sum()), ag.games_to_track) and float(ag.game_lengths.get_mean()) > 0
    assert bool((ag.current_lengths[dones[-1] != 0] == 0).all()) and bool((ag.current_lengths[dones[-1] == 0] > 0).all())


def test_agent_with_the_environment_on_the_host(boundary, golden_dir, monkeypatch):
    """A CPU environment under a GPU agent - what the default play_steps accepts: every tensor of infos is moved before its
    address enters the field table, and the stored rows are the environment's."""
    T = boundary
    G = T._load(golden_dir, 'amp')
    monkeypatch.setattr(T, '_DEV', 'cpu')
    env = T._env(G)
    monkeypatch.setattr(T, '_DEV', 'cuda:0')
    ag, _ = T._agent(G, env, device_rollout=True)
    seen = []
    step = env.step

    def recording_step(actions):
        out = step(actions)
        assert not out[3]['amp_obs'].is_cuda
        seen.append((out[0].clone(), out[3]['amp_obs'].clone(), out[2].clone()))
        return out
    env.step = recording_step
    ag.play_steps()
    torch.cuda.synchronize()
    assert len(seen) == ag.horizon_length
    for n, (obs, amp_obs, dones) in enumerate(seen):
        R.same(ag.experience['amp_obs'][n], amp_obs, f'amp_obs {n}')
        R.same(ag.experience['next_obses'][n], obs, f'next_obses {n}')
        R.same(ag.experience['dones'][n], dones, f'dones {n}')
    assert int(ag._meter_words[3]) == sum(int(d.sum()) for _, _, d in seen)
