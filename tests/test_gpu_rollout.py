"""The rollout kernels (csrc/rollout.hip) against tests/ref_rollout.py: the Philox stream word for word, and every
operation against an f64 evaluation of the reference's own formula.

Float outputs: max |hip - f64| <= 2 e_ref + 1e-7, with e_ref = max |f32 run - f64 run| of the reference on the same inputs
(never of the kernel); both numbers are printed.  Integer, mask and copy outputs are exactly equal, and
what a call does not own keeps the sentinel it was filled with.  The deterministic operations run the same bodies
(ref_rollout.check_*) as the emulator does in tests/test_rollout_ref.py."""
import pytest
import torch

from tests import ref_rollout as RR

pytestmark = pytest.mark.gpu

SEEDS = [(1234, 5), ((1 << 40) + 17, (1 << 35) + 3), (-987654321012, 1 << 32)]     # (seed, offset): small, >= 2^32, negative seed


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend()


def _state(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64).cuda()


def _filled(shape, dtype=torch.float32):
    return torch.full(shape, RR.SENTINEL, dtype=dtype).cuda()


def _kept(t):
    return bool((t == torch.tensor(RR.SENTINEL, dtype=t.dtype)).all())       # the sentinel as the storage type rounds it


# ------------------------------------------------------------------------------------------------ sample_latents
@pytest.mark.parametrize('rows', [1, 5, 1027])
@pytest.mark.parametrize('dim', [1, 63, 64, 65, 128])
def test_sample_latents(be, dim, rows):
    for seed, offset in SEEDS:
        st = _state(seed, offset)
        z = _filled((rows + 2, dim))
        be.sample_latents(z, rows, dim, st)
        assert st.tolist() == [seed, offset + 1]
        RR.within(z[:rows], RR.sample_latents(rows, dim, seed, offset), RR.sample_latents(rows, dim, seed, offset, dtype=torch.float32),
                  f'sample_latents {rows}x{dim} seed {seed} offset {offset}')
        assert _kept(z[rows:])


def test_sample_latents_element_index_past_2_32(be):
    """row_offset = 70 000 000 with dim 64: the first element is 4.48e9 - the high counter word is in use."""
    rows, dim, ro = 5, 64, 70_000_000
    assert ro * dim > 1 << 32
    seed, offset = SEEDS[1]
    st = _state(seed, offset)
    z = _filled((rows + 1, dim))
    be.sample_latents(z, rows, dim, st, row_offset=ro, advance=False)
    assert st.tolist() == [seed, offset]
    RR.within(z[:rows], RR.sample_latents(rows, dim, seed, offset, ro), RR.sample_latents(rows, dim, seed, offset, ro, torch.float32),
              'sample_latents row_offset 7e7')
    assert _kept(z[rows:])
    low = _filled((rows, dim))
    be.sample_latents(low, rows, dim, st, row_offset=ro - (1 << 32) // dim, advance=False)      # the index modulo 2^32
    assert not torch.equal(low, z[:rows])


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('dim', [63, 65])
def test_sample_latents_second_output(be, dim, dt):
    rows, ld = 9, dim + 7
    st = _state(*SEEDS[0])
    z = _filled((rows, dim))
    wide = _filled((rows + 1, ld), dt)
    be.sample_latents(z, rows, dim, st, row_offset=3, z2=wide[:rows, :dim])
    assert torch.equal(wide[:rows, :dim], z.to(dt))                    # the exact conversion (round to nearest even) of z
    assert _kept(wide[:, dim:]) and _kept(wide[rows:])
    RR.within(z, RR.sample_latents(rows, dim, *SEEDS[0], 3), RR.sample_latents(rows, dim, *SEEDS[0], 3, torch.float32),
              f'sample_latents with z2 {dt}')


# ------------------------------------------------------------------------------------------------ sample_actions
def _actions_case(be, n, A, mu_tanh, rows_logstd, seed, offset, probs='mixed', want_mask=True, name=''):
    g = torch.Generator().manual_seed(n * 131 + A)
    mu = torch.full((n, A + 3), RR.NAN)                                # NaN padding: a read past A shows in neglogp
    mu[:, :A] = torch.randn(n, A, generator=g) * 0.5
    if rows_logstd:
        logstd = torch.full((n, A + 5), RR.NAN)
        logstd[:, :A] = -2.9 + 0.3 * torch.randn(n, A, generator=g)
    else:
        logstd = -1.0 + 0.5 * torch.randn(A, generator=g)
    p = None
    if probs == 'mixed':
        p = torch.rand(n, generator=g)
        p[0::5] = 1.0
        p[1::5] = 0.0
    elif probs == 'ones':
        p = torch.ones(n)
    st = _state(seed, offset)
    out = {k: _filled((n + 1, A)) for k in ('mu', 'sigma', 'act')}
    nlp, mask = _filled((n + 1,)), _filled((n + 1,))
    be.sample_actions(mu.cuda(), logstd.cuda(), None if p is None else p.cuda(), st, out['mu'], out['sigma'], out['act'], nlp,
                      mask if want_mask else None, n, A, mu_tanh=mu_tanh, logstd_rows=rows_logstd)
    assert st.tolist() == [seed, offset + 1]                           # the offset advances by exactly one
    r64 = RR.sample_actions(mu, logstd, p, seed, offset, n, A, mu_tanh)
    r32 = RR.sample_actions(mu, logstd, p, seed, offset, n, A, mu_tanh, torch.float32)
    assert torch.equal(r64['keep'], r32['keep'])
    if want_mask:
        assert torch.equal(mask[:n].cpu(), r64['keep']), name          # every row, bit for bit
    else:
        assert _kept(mask)
    if p is not None:
        assert bool((r64['keep'][p == 1.0] == 1).all()) and bool((r64['keep'][p == 0.0] == 0).all())
    det = (r64['keep'] == 0).cuda()
    assert torch.equal(out['act'][:n][det], out['mu'][:n][det])        # deterministic rows return mu bitwise
    if not mu_tanh:
        assert torch.equal(out['mu'][:n].cpu(), mu[:, :A])
    RR.within(out['mu'][:n], r64['mu'], r32['mu'], f'sample_actions mu {name}')
    RR.within(out['sigma'][:n], r64['sigma'], r32['sigma'], f'sample_actions sigma {name}')
    RR.within(out['act'][:n], r64['actions'], r32['actions'], f'sample_actions actions {name}')
    RR.within(nlp[:n], r64['neglogp'], r32['neglogp'], f'sample_actions neglogp {name}')
    for t in (out['mu'], out['sigma'], out['act'], nlp):
        assert _kept(t[n:])
    return r64


@pytest.mark.parametrize('rows_logstd', [False, True])
@pytest.mark.parametrize('mu_tanh', [False, True])
@pytest.mark.parametrize('A', [1, 31, 64])
def test_sample_actions(be, A, mu_tanh, rows_logstd):
    seed, offset = SEEDS[(A + mu_tanh + rows_logstd) % 3]
    r = _actions_case(be, 1027, A, mu_tanh, rows_logstd, seed, offset, name=f'A{A} tanh={int(mu_tanh)} rows={int(rows_logstd)}')
    assert 0 < int(r['keep'].sum()) < 1027


def test_sample_actions_optional_operands(be):
    r = _actions_case(be, 13, 31, False, False, *SEEDS[0], probs=None, name='rand_probs None')
    assert bool((r['keep'] == 1).all())                                # no eps-greedy: every row keeps its sample
    _actions_case(be, 13, 31, True, True, *SEEDS[1], want_mask=False, name='rand_mask None')


@pytest.mark.parametrize('offset', [20477295, 31492960, 36996719])
def test_sample_actions_bernoulli_one_draws_one(be, offset):
    """seed 7, n = 8, A = 2: row 3's keep word (element n*A + 3 = 19) is >= 0xFFFFFF80, which a 32-bit conversion rounds to a
    uniform of exactly 1.0 - and 1.0 < 1.0 made Bernoulli(1.0) draw 0."""
    assert int(RR.philox4x32_10(19, offset, 7)[2][0]) >= 0xffffff80
    r = _actions_case(be, 8, 2, False, False, 7, offset, probs='ones', name=f'Bernoulli(1) offset {offset}')
    assert bool((r['keep'] == 1).all())


# ------------------------------------------------------------------------------------------------ deterministic operations
@pytest.mark.parametrize('c', RR.disc_cases(), ids=lambda c: c['name'])
def test_disc_reward(be, c):
    RR.check_disc_reward(be, 'cuda', c, 'hip')


@pytest.mark.parametrize('c', RR.row_cases(), ids=lambda c: c['name'])
def test_enc_reward(be, c):
    RR.check_enc_reward(be, 'cuda', c, 'hip')


@pytest.mark.parametrize('c', RR.row_cases(), ids=lambda c: c['name'])
def test_normalize_rows(be, c):
    RR.check_normalize_rows(be, 'cuda', c, 'hip')


@pytest.mark.parametrize('H,N', RR.GAE_SHAPES)
def test_gae(be, H, N):
    for c in RR.gae_cases(H, N):
        RR.check_gae(be, 'cuda', c, 'hip')


@pytest.mark.parametrize('c', RR.adv_cases(), ids=lambda c: c['name'])
def test_adv_norm(be, c):
    RR.check_adv_norm(be, 'cuda', c, 'hip')


@pytest.mark.parametrize('D', RR.RING_DIMS)
def test_ring_store(be, D):
    for c in RR.ring_cases(D):
        RR.check_ring_store(be, 'cuda', c, 'hip')
