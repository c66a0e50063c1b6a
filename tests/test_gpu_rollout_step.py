"""The head of a rollout step in one launch on the MI355X: ``ase_hip_rollout_head`` / ``ase_hip_word_step``
through ``HipBackend``, ``torch.ops.ase_hip`` and a launch program.

The bars (tests/ref_rollout_step.py): every output BITWISE the composition the entry replaces - the rms_normalize expression in
f32 and torch's cast, the saturating latent conversion, an indexed copy for the slot - NaN patterns and -0.0 included, inside
sentinel-filled allocations whose every guard word is compared after each launch; and bitwise the existing HIP entries
(rms_normalize into two outputs, gather_rows twice, copy_) on the same inputs.  ASE_ROLLOUT_STEP_REPORT=<file> writes the
counts (for COVERAGE.md N18)."""
import json
import os

import pytest
import torch

from tests import ref_rollout_step as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    yield HipBackend('cuda:0')
    out = os.environ.get('ASE_ROLLOUT_STEP_REPORT')
    if out:
        with open(out, 'w') as f:
            json.dump(R.COUNTS, f, indent=1)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('n', R.NS)
def test_every_width_at_every_row_count(be, n, dtype):
    R.check_shapes(be, DEV, n, dtype)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('knob,value,side', R.VIOLATIONS)
def test_each_clause_of_the_path_condition(be, dtype, knob, value, side):
    R.check_violation(be, DEV, dtype, knob, value, side)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('outs', R.OUTPUT_SETS, ids='+'.join)
def test_each_output_alone_and_together(be, dtype, outs):
    R.check_outputs(be, DEV, dtype, outs)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_slots_by_value_and_by_word(be, dtype):
    R.check_slots(be, DEV, dtype)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_one_row_views_with_meaningless_row_strides(be, dtype):
    R.check_one_row(be, DEV, dtype)


def test_word_step(be):
    R.check_word_step(be, DEV)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_program_of_head_store_and_counter(be, dtype):
    R.check_program(be, DEV, dtype)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('D,Z,lay', ((253, 64, {}), (260, 64, {}), (260, 1, {}), (4, 64, dict(obs_off=5)), (1, 1, {}), (3, 0, {})))
def test_head_equals_the_entries_it_replaces(be, dtype, D, Z, lay):
    """The device functions agree, not only the reference: the same inputs through ase_hip_rms_normalize into two outputs,
    ase_hip_gather_rows twice and copy_ leave every allocation bitwise as the one launch leaves it."""
    n, slot = 300, 2
    c, twin = R.Case(DEV, n, D, Z, dtype, seed=7, **lay), R.Case(DEV, n, D, Z, dtype, seed=7, **lay)
    c.run(be, slot=slot, what='one launch')
    b = twin.bufs
    be.rms_normalize(twin.obs.view, D, None, (0, 0), n, twin.mean.view, twin.std.view, [b['xa'].view, b['xc'].view])
    b['obses_out'].view[slot].copy_(twin.obs.view)
    if Z:
        be.gather_rows(twin.z.view, Z, None, (0, 0), n, b['zc'].view)
        be.gather_rows(twin.z.view, Z, None, (0, 0), n, b['zs'].view)
        b['z_out'].view[slot].copy_(twin.z.view)
    torch.cuda.synchronize()
    for k in c.bufs:
        assert torch.equal(R.bits(c.bufs[k].alloc), R.bits(b[k].alloc)), (k, D, Z, str(dtype))


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_torch_ops_equal_the_backend_calls(be, dtype):
    import ase_amd.ops  # noqa: F401

    def op(obs, z=None, mean=None, std=None, xa=None, xc=None, zc=None, zs=None, obses_out=None, z_out=None, slot=0, slot_dev=None):
        torch.ops.ase_hip.rollout_head(obs, z, mean, std, xa, xc, zc, zs, obses_out, z_out, slot, slot_dev)
    word = torch.tensor([1], dtype=torch.int32, device=DEV)
    for outs, kw in ((R.OUTS, dict(slot=1)), (R.CRITIC_ONLY, {}), (R.OUTS, dict(slot=0, slot_dev=word, word=1))):
        c, twin = R.Case(DEV, 65, 253, 64, dtype, outs=outs, seed=9), R.Case(DEV, 65, 253, 64, dtype, outs=outs, seed=9)
        c.run(be, call=op, what='torch op', **kw)
        twin.run(be, what='backend call', **kw)
        for k in c.bufs:
            assert torch.equal(R.bits(c.bufs[k].alloc), R.bits(twin.bufs[k].alloc)), k
    R.check_word_step(be, DEV, call=torch.ops.ase_hip.word_step)
