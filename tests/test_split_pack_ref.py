"""The reference packer of the half-split shadows (tests/ref_split_pack.py) on the CPU: its words unpack to (hi + lo) * 2^-e exactly,
everything it does not cover keeps the sentinel, its cases contain what they claim, and it is half_split wherever nothing saturates.
The GPU tests compare ase_hip_refresh_shadow (tests/test_gpu_gemm_tn_exact.py) and the optimizer launch (tests/test_gpu_gp_fuse.py)
against it."""
import pytest
import torch

from tests import ref_split_pack as S
from tests.emu_backend import half_split, unpack_split

SHAPES = [(1, 1, 1, 1), (33, 65, 65, 65), (48, 53, 37, 64)]
EXPS = [0, 11, 24]


def _shapes(n, k, ss, sd):
    kp = k + (sd - ss)
    return (n + 3, (kp + 7) // 8 * 8 + 8), (kp + 2, (n + 7) // 8 * 8 + 16)


@pytest.mark.parametrize('e', EXPS)
@pytest.mark.parametrize('n,k,ss,sd', SHAPES)
def test_packer_round_trips_through_unpack_split(n, k, ss, sd, e):
    W = S.split_case(n, k, e, 100 * n + k + e)
    shape_ws, shape_wts = _shapes(n, k, ss, sd)
    ws, wts = S.expected_pair(W, e, ss, sd, shape_ws, shape_wts)
    hi, lo = S.split_halves(W, e)
    want = (hi.double() + lo.double()) * 2.0 ** -e
    kd = S.shadow_cols(k, ss, sd)
    got_ws = unpack_split(ws.view(torch.float32), n, shape_ws[1], e)[:, kd]
    got_wts = unpack_split(wts.view(torch.float32), shape_wts[0], n, e)[kd]
    assert torch.equal(got_ws, want) and torch.equal(got_wts, want.t())
    # -0.0 keeps its sign in hi (the sum above cannot tell), lo of it is +0.0
    neg0 = W.view(torch.int32) == -2 ** 31
    assert bool((hi.view(torch.int16)[neg0] == -2 ** 15).all()) and bool((lo.view(torch.int16)[neg0] == 0).all())


@pytest.mark.parametrize('n,k,ss,sd', SHAPES)
def test_packer_leaves_the_sentinel_everywhere_else(n, k, ss, sd):
    """Pad rows, pad columns, gap columns and the uncovered positions of a partly covered group of 8: half-words of the sentinel."""
    e = 11
    W = S.split_case(n, k, e, 7)
    shape_ws, shape_wts = _shapes(n, k, ss, sd)
    kd, rn = S.shadow_cols(k, ss, sd), torch.arange(n)
    sent = torch.full((1,), S.SENTINEL).view(torch.int16)
    for words, rows, cols in ((S.pack_split(W, rn, kd, e, shape_ws), rn, kd), (S.pack_split(W.t(), kd, rn, e, shape_wts), kd, rn)):
        h = words.view(torch.int16).clone()
        covered = torch.zeros_like(h, dtype=torch.bool)
        pos = (cols >> 3) * 16 + (cols & 7)
        covered[rows[:, None], pos[None, :]] = True
        covered[rows[:, None], pos[None, :] + 8] = True
        assert int(covered.sum()) == 2 * n * k
        want = sent.repeat(h.shape[0], h.shape[1] // 2)
        assert torch.equal(h[~covered], want[~covered])
    if sd > ss:     # the gap and the partly covered group of this shape are really there
        assert int(kd[ss]) - int(kd[ss - 1]) > 1 and ss % 8 != 0


@pytest.mark.parametrize('e', EXPS)
def test_packer_is_half_split_where_nothing_saturates(e):
    """... and differs from it exactly at the saturated elements, where the kernels' order (saturate, then split) gives lo = 0."""
    W = S.split_case(33, 65, e, 3)
    hi, lo = S.split_halves(W, e)
    h0, l0 = half_split(W, e)
    sat = (W * 2.0 ** e).abs() > 65504
    assert int(sat.sum()) == 2
    assert torch.equal(hi.double(), h0) and torch.equal(lo.double()[~sat], l0[~sat])
    assert bool((lo[sat] == 0).all()) and bool((l0[sat] != 0).all())


def test_case_generator_refuses_a_case_without_its_coverage(monkeypatch):
    monkeypatch.setattr(S, 'planted', lambda e: torch.ones(12) * 2.0 ** -e)
    with pytest.raises(AssertionError, match='no saturated element'):
        S.split_case(33, 65, 11, 1)
