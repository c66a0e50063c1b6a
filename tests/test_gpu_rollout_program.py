"""The agents' ``rollout_program`` on the MI355X: the cases of tests/test_rollout_program_emu.py with the HIP
backend - one environment step recorded once as a launch program of the library, replayed horizon_length times, against
``device_rollout`` alone, tensor for tensor, and the epoch that follows loss for loss."""
import pytest
import torch

from tests import test_rollout_program_emu as P

pytestmark = pytest.mark.gpu


@pytest.fixture
def boundary(monkeypatch):
    import tests.test_boundary_emu as T
    monkeypatch.setattr(T, '_DEV', 'cuda:0')
    return T


def _be():
    from ase_amd.backend import HipBackend
    return HipBackend('cuda:0')


@pytest.mark.parametrize('kind', P.KINDS)
def test_program_rollouts_equal_the_device_rollouts(boundary, golden_dir, kind):
    """Three rollouts tensor for tensor, a fourth, then the epoch's losses on the eager agent's rollout and on the program
    agent's, both through ONE engine from one checkpoint (P.epoch_on_one_engine): two engines add the encoder head's bias
    gradients and the loss sums of several workgroups with atomics (csrc/heads.hip), whose arrival order follows the
    allocation layout, so two updates on bitwise-equal inputs need not agree in the last bit; one engine runs the same
    launches on the same buffers twice."""
    a, b = P.run_equal(boundary, P.tiny(golden_dir, kind), _be, sync=torch.cuda.synchronize, one_engine=True)
    # recorded once, for the second rollout; the third and fourth replayed it
    assert b.backend.prog_size(b._rp['prog']) > 0 and int(b._rp['word']) == b.horizon_length


def test_recorded_again_after_drop_graphs(boundary, golden_dir):
    G = P.tiny(golden_dir, 'ase')
    a, b = P.pair(boundary, G, _be)
    for _ in range(2):
        b.play_steps()
    size = b.backend.prog_size(b._rp['prog'])
    b._drop_graphs()
    assert b._rp is None
    for _ in range(2):
        b.play_steps()
    for _ in range(4):
        a.play_steps()
    torch.cuda.synchronize()
    assert b.backend.prog_size(b._rp['prog']) == size and b.vec_env.steps == a.vec_env.steps == 4 * b.horizon_length
    P.assert_same_state(a, b, 'after a re-recording')


@pytest.mark.parametrize('kind', ('amp', 'ase'))
def test_replay_path_runs_no_nonzero_and_no_item(boundary, golden_dir, kind, monkeypatch):
    _, b = P.pair(boundary, P.tiny(golden_dir, kind), _be)
    b.play_steps()
    b.play_steps()

    def raising(*a, **kw):
        raise AssertionError('nonzero / item called on the replay path')
    monkeypatch.setattr(torch.Tensor, 'nonzero', raising)
    monkeypatch.setattr(torch.Tensor, 'item', raising)
    b.play_steps()                                               # the whole of it: prologue, replays, meters, the tail
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert int(b._rp['word']) == b.horizon_length


def test_humanoid_env_reads_the_environments_buffers_in_place(boundary, golden_dir):
    # (rollouts only: the epoch comparison above runs on SyntheticVecEnv, whose demo fetch one generator restores)
    P.run_humanoid(boundary, golden_dir, _be, _be, 'cuda', sync=torch.cuda.synchronize, train=False)
