"""tests/ref_rollout.py pinned without a GPU: the published Philox4x32-10 known answers, the keep-uniform's 24-bit
definition, the size of the f32 Box-Muller error, and the emulator's deterministic rollout operations (tests/emu_backend.py)
against the f64 reference on the inputs of tests/test_gpu_rollout.py - emulator, reference and kernel stay in one chain."""
import numpy as np
import pytest
import torch

from tests import ref_rollout as RR
from tests.emu_backend import EmuBackend

KAT = [   # Random123 kat_vectors, philox4x32 10 rounds: counter; key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers(ctr, key, want):
    elem, offset, seed = ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32, key[0] | key[1] << 32
    got = RR.philox4x32_10(elem, offset, seed)
    assert tuple(int(w[0]) for w in got) == want
    # vectorised: the same element among others gives the same words
    if elem < (1 << 63):
        many = RR.philox4x32_10(np.array([5, elem, 1 << 40], dtype=np.uint64), offset, seed)
        assert tuple(int(w[1]) for w in many) == want


def test_negative_seed_is_twos_complement():
    a = RR.philox4x32_10(np.arange(4, dtype=np.uint64), 3, -5)
    b = RR.philox4x32_10(np.arange(4, dtype=np.uint64), 3, (1 << 64) - 5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('offset', [20477295, 31492960, 36996719])
def test_keep_uniform_is_below_one(offset):
    """seed 7, n = 8, A = 2, row 3 -> element 19: the 32-bit conversion rounds the word to exactly 1.0 (Bernoulli(1.0) draws 0),
    the 24-bit one stays below 1."""
    c2 = RR.philox4x32_10(19, offset, 7)[2]
    if offset == 20477295:
        assert int(c2[0]) == 0xffffff8c
    assert int(c2[0]) >= 0xffffff80
    assert float(RR.keep_uniform_32bit(c2)[0]) == 1.0
    u = RR.keep_uniform(c2)
    assert u.dtype == np.float32 and float(u[0]) < 1.0
    top = RR.keep_uniform(np.array([0xffffffff, 0], dtype=np.uint32))
    assert float(top[0]) == 1.0 - 2.0 ** -24 and float(top[1]) == 0.0


def test_box_muller_f32_error():
    """max |f32 - f64| of the normal over 2M random word pairs (numpy here: 1.17e-6).  Bound: the f32 product 2 pi * u2 is off
    by at most half an ulp of a number below 8, 2.4e-7, times the largest radius sqrt(-2 ln 2^-32) = 6.66 -> 1.6e-6; the
    remaining roundings (log, sqrt, cos, product: a few ulp of a result below 6.66, ulp 4.8e-7) stay below 1.4e-6."""
    rng = np.random.default_rng(0)
    c0 = rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64).astype(np.uint32)
    c1 = rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64).astype(np.uint32)
    c0[:3] = (0, 0xffffffff, 1)                            # u1 = 2^-32 (largest radius), 1 (radius 0)
    z64, z32 = RR._box_muller(c0, c1), RR._box_muller(c0, c1, np.float32)
    assert z32.dtype == np.float32 and z64.dtype == np.float64
    assert np.isfinite(z64).all() and np.isfinite(z32).all()
    err = float(np.abs(z32.astype(np.float64) - z64).max())
    print(f'box-muller: max |f32 - f64| over 2M draws = {err:.3g}; mean {z64.mean():.3g}, var {z64.var():.4g}')
    assert err <= 3e-6
    assert abs(z64.mean()) < 5e-3 and abs(z64.var() - 1) < 5e-3


def test_normal_and_keep_elements_are_disjoint():
    """sample_actions: normals use elements [0, n*A), the keep draws [n*A, n*A + n) - and they read different words."""
    n, A = 7, 3
    r = np.arange(n, dtype=np.uint64)
    normal = (r[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)).ravel()
    keep = np.uint64(n * A) + r
    assert not set(normal.tolist()) & set(keep.tolist())
    ref = RR.sample_actions(torch.zeros(n, A), torch.zeros(A), torch.full((n,), 0.5), 7, 0, n, A)
    assert torch.equal(ref['sampled'], RR.normals(normal.reshape(n, A), 0, 7))
    assert torch.equal(ref['actions'][ref['keep'] == 0], ref['mu'][ref['keep'] == 0])


def test_sample_latents_reference_rows_are_stream_rows():
    full = RR.sample_latents(40, 65, -3, 1 << 33)
    assert torch.equal(RR.sample_latents(7, 65, -3, 1 << 33, row_offset=20), full[20:27])
    big = RR.latent_elems(2, 64, 70_000_000)
    assert int(big[0, 0]) == 70_000_000 * 64 > (1 << 32)


# ------------------------------------------------------------------------------------------------ emulator vs reference
@pytest.mark.parametrize('c', RR.disc_cases(), ids=lambda c: c['name'])
def test_emu_disc_reward(c):
    RR.check_disc_reward(EmuBackend(), 'cpu', c, 'emu')


@pytest.mark.parametrize('c', RR.row_cases(), ids=lambda c: c['name'])
def test_emu_enc_reward_and_normalize_rows(c):
    RR.check_enc_reward(EmuBackend(), 'cpu', c, 'emu')
    RR.check_normalize_rows(EmuBackend(), 'cpu', c, 'emu')


@pytest.mark.parametrize('H,N', RR.GAE_SHAPES)
def test_emu_gae(H, N):
    for c in RR.gae_cases(H, N):
        RR.check_gae(EmuBackend(), 'cpu', c, 'emu')


@pytest.mark.parametrize('c', RR.adv_cases(), ids=lambda c: c['name'])
def test_emu_adv_norm(c):
    RR.check_adv_norm(EmuBackend(), 'cpu', c, 'emu')


@pytest.mark.parametrize('D', RR.RING_DIMS)
def test_emu_ring_store(D):
    for c in RR.ring_cases(D):
        RR.check_ring_store(EmuBackend(), 'cpu', c, 'emu')


def test_row_map():
    idx = torch.tensor([0, 1, 5, 44, 7], dtype=torch.int32)
    assert RR.row_map(idx, (5, 9), 5).tolist() == [0, 9, 1, 4 * 9 + 8, 2 * 9 + 1]        # p = env*H + t -> t*N + env
    assert RR.row_map(None, (0, 0), 3).tolist() == [0, 1, 2]
    assert RR.row_map(idx, (0, 0), 2).tolist() == [0, 1]
