"""``rollout_head`` / ``word_step`` without a GPU: the emulator (tests/emu_rollout_step.py) against the
composition the entry replaces (tests/ref_rollout_step.py), the same cases tests/test_gpu_rollout_step.py runs on the device,
bitwise and with every guard word; the entry's host refusals through the C ABI, each before any launch; the torch ops'
registration."""
import ctypes

import pytest
import torch

from ase_amd import lib as L
from tests import ref_rollout_step as R
from tests.emu_rollout_step import EmuRolloutStep

DEV = 'cpu'


@pytest.fixture(scope='module')
def be():
    return EmuRolloutStep()


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


def test_reference_values_are_what_the_cases_claim():
    """The steering works: in an exact column the clamp's bounds and the ties come out exactly, the tie cases round to even in
    both 16-bit types, and the latent conversion saturates (NaN -> -65504 in half)."""
    mean, std = torch.tensor([0.5]), torch.tensor([0.25])
    y = torch.tensor(R.Y_SPECIAL, dtype=torch.float64)
    x = (mean.double() + y * std.double()).float().view(-1, 1)
    ref, _ = R.reference(x, None, mean, std, torch.float32)
    want = torch.clamp(y, -5.0, 5.0).float().view(-1, 1)
    want[14] = 0.0                                   # mean + (-0.0) std is mean: the target -0.0 arrives as +0.0
    assert torch.equal(R.bits(ref)[1:], R.bits(want)[1:]) and bool(torch.isnan(ref[0]))
    b16, _ = R.reference(x, None, mean, std, torch.bfloat16)
    assert b16[7].item() == 1.0 and b16[8].item() == 1 + 2.0 ** -6            # 1 + 2^-8 -> 1 (even), 1 + 3 2^-8 -> 1 + 2^-6
    h16, _ = R.reference(x, None, mean, std, torch.float16)
    assert h16[9].item() == 1.0 and h16[10].item() == 1 + 2.0 ** -9
    _, z = R.reference(x, torch.tensor([R.Z_SPECIAL]), mean, std, torch.float16)
    assert z[0].tolist()[:7] == [65504.0, -65504.0, -65504.0, -0.0, 65504.0, 65504.0, -65504.0]
    assert R.bits(z)[0, 3].item() == -0x8000                                 # -0.0 keeps its sign


# ---- the C ABI: refusals on the host, before any launch (no GPU needed) -----------------------------------------------------------
def _head(lib, **kw):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p).value // 16 * 16 + 16
    a = dict(obs=p, ld_obs=8, D=8, z=p, ld_z=4, Z=4, mean=p, std=p, xa=p, ld_xa=8, xc=p, ld_xc=8, zc=p, ld_zc=4, zs=p, ld_zs=4,
             x_dtype=L.F32, obses_out=p, ld_oo=8, ss_oo=32, z_out=p, ld_zo=4, ss_zo=16, n=4, slot=0, slot_dev=None, n_slots=2)
    a.update(kw)
    rc = lib.ase_hip_rollout_head(a['obs'], a['ld_obs'], a['D'], a['z'], a['ld_z'], a['Z'], a['mean'], a['std'], a['xa'], a['ld_xa'],
                                  a['xc'], a['ld_xc'], a['zc'], a['ld_zc'], a['zs'], a['ld_zs'], a['x_dtype'], a['obses_out'],
                                  a['ld_oo'], a['ss_oo'], a['z_out'], a['ld_zo'], a['ss_zo'], a['n'], a['slot'], a['slot_dev'],
                                  a['n_slots'], None)
    return rc, lib.ase_hip_last_error()


REFUSALS = [
    (dict(xa=None, xc=None, zc=None, zs=None, obses_out=None, z_out=None), b'no output'),
    (dict(n=0), b'n 0'), (dict(n=-3), b'n -3'), (dict(D=0), b'D 0'),
    (dict(obs=None), b'null obs'),
    (dict(ld_obs=7), b'pitch below D'), (dict(ld_xa=7), b'pitch below D'), (dict(ld_xc=7), b'pitch below D'),
    (dict(ld_oo=7), b'pitch below D'),
    (dict(ld_z=3), b'pitch below Z'), (dict(ld_zc=3), b'pitch below Z'), (dict(ld_zs=3), b'pitch below Z'),
    (dict(ld_zo=3), b'pitch below Z'),
    (dict(z=None), b'without z'), (dict(Z=-1), b'without z'),
    (dict(Z=0, zc=None, zs=None), b'Z == 0'), (dict(Z=0, z_out=None, zs=None), b'Z == 0'), (dict(Z=0, z_out=None, zc=None), b'Z == 0'),
    (dict(mean=None), b'mean and std'), (dict(std=None, xa=None), b'mean and std'),
    (dict(x_dtype=L.F32X3), b'x_dtype'),
    (dict(ss_oo=31), b'slot stride'), (dict(ss_zo=15), b'slot stride'),
    (dict(n_slots=0), b'slot'), (dict(slot=2), b'slot 2'), (dict(slot=-1), b'slot -1'),
]


@pytest.mark.parametrize('kw,msg', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_head_refusals_on_the_host(kw, msg):
    rc, err = _head(L.load(), **kw)
    assert rc == -1 and b'rollout_head' in err and msg in err, (kw, rc, err)


def test_slot_arguments_are_checked_only_with_a_slot_output_and_word_step_refuses_null():
    lib = L.load()
    word = (ctypes.c_int32 * 1)(5)
    # slot_dev does not lift the host check of slot
    rc, err = _head(lib, slot=2, slot_dev=ctypes.cast(word, ctypes.c_void_p))
    assert rc == -1 and b'slot 2' in err
    assert lib.ase_hip_word_step(None, 1, 0, None) == -1 and b'word_step' in lib.ase_hip_last_error()


def test_ops_are_registered():
    import ase_amd.ops  # noqa: F401
    assert hasattr(torch.ops.ase_hip, 'rollout_head') and hasattr(torch.ops.ase_hip, 'word_step')
    assert 'Tensor(a' in str(torch.ops.ase_hip.word_step.default._schema)          # word is written in place
    with pytest.raises(NotImplementedError):
        torch.ops.ase_hip.word_step(torch.zeros(1, dtype=torch.int32), 1, 0)
