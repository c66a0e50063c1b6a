"""Renewals of the ASE latents on the MI355X: ``ase_hip_latent_renew`` through ``HipBackend``,
``torch.ops.ase_hip.latent_renew``, a launch program and ``ASEAgent`` / ``ASEPlayer`` with ``device_latents``.

The bars: passed-in draws against the f64 restatement of the recording of the reference's own methods
(tests/golden/latent_renew.pt) at max |hip - f64| <= 2 e_ref + 1e-7 (e_ref is stored in the fixture); device draws
against the stream's specification tests/ref_rollout.py at the same rule and bitwise against ``sample_latents`` of the same
library; integers (step counts, stream positions) exactly; everything a call does not own bitwise unchanged."""
import pytest
import torch

from tests import emu_latent_renew as E
from tests import ref_rollout as RR

pytestmark = pytest.mark.gpu

SEED = (1 << 33) + 12345
OFFSETS = (0, (1 << 32) + 7)
NAN = float('nan')


@pytest.fixture(scope='module')
def be():
    from ase_amd.backend import HipBackend
    return HipBackend('cuda:0')


@pytest.fixture(scope='module')
def G():
    return E.load_fixture()


def _state(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64).cuda()


def _i32(ids):
    return torch.tensor(list(ids), dtype=torch.int32).cuda()


# ---- 1. passed-in draws against the recording --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.SCENARIOS)
def test_recorded_draws_reproduce_the_reference(be, G, name):
    """Renewed rows within 2 e_ref + 1e-7 of the f64 restatement, step counts exact, every other row bitwise the prefill.
    Observed on one MI355X: max |hip - f64| 3.1e-08 in each of the three scenarios, 1.69e-07 allowed (COVERAGE.md N9)."""
    sc = G['scenarios'][name]
    ids = sc['env_ids']
    others = [e for e in range(G['num_envs']) if e not in ids]
    latents, reset_steps, progress = E.prefill(G, name, device='cuda')
    be.latent_renew(latents, reset_steps=reset_steps, **E.call_of(G, name, 'cuda'))
    l64, s64 = E.expected(G, name, torch.float64)
    err = float((latents.cpu()[ids].double() - l64[ids]).abs().max())
    print(f'latent_renew {name}: max |hip - f64| = {err:.3g}, e_ref = {sc["e_ref"]:.3g}, allowance {E.allowance(G, name):.3g}')
    assert err <= E.allowance(G, name), (name, err)
    assert torch.equal(reset_steps.cpu(), sc['reset_steps']) and torch.equal(reset_steps.cpu(), s64)
    lat0, steps0, progress0 = E.prefill(G, name)
    assert torch.equal(latents.cpu()[others], lat0[others]) and torch.equal(reset_steps.cpu()[others], steps0[others])
    assert progress is None or torch.equal(progress.cpu(), progress0)


# ---- 2. device draws ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('advance', (True, False))
@pytest.mark.parametrize('offset', OFFSETS)
def test_device_draws_are_the_stream(be, offset, advance):
    n, dim, lo, hi = 37, 65, 1, 150
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:21].tolist()
    others = [e for e in range(n) if e not in ids]
    lat0 = E.pattern(n, dim)
    steps0 = torch.arange(n, dtype=torch.int32) * 13 + 5
    latents, reset_steps, st = lat0.cuda(), steps0.cuda(), _state(SEED, offset)
    be.latent_renew(latents, env_ids=_i32(ids), rng_state=st, advance=advance, reset_steps=reset_steps, steps_low=lo, steps_high=hi)
    assert st.tolist() == [SEED, offset + int(advance)]                    # the stream position moves by exactly `advance`
    RR.within(latents[ids], RR.sample_latents(n, dim, SEED, offset)[ids], RR.sample_latents(n, dim, SEED, offset, dtype=torch.float32)[ids],
              f'latent_renew device draws offset {offset}')
    z = torch.zeros(n, dim).cuda()
    be.sample_latents(z, n, dim, _state(SEED, offset))
    bitwise = torch.equal(latents[ids], z[ids])
    print(f'latent_renew rows bitwise equal to sample_latents rows at offset {offset}: {bitwise}')
    assert bitwise
    assert torch.equal(reset_steps.cpu()[ids], E.device_draws(ids, dim, SEED, offset, lo, hi)[1])
    assert torch.equal(latents.cpu()[others], lat0[others]) and torch.equal(reset_steps.cpu()[others], steps0[others])


# ---- 3. due mode equals ids mode on the due list -----------------------------------------------------------------------------
@pytest.mark.parametrize('pdt', (torch.int32, torch.int64))
def test_due_mode_equals_ids_mode_on_the_due_list(be, G, pdt):
    sc = G['scenarios']['update']
    lat_a, steps_a, progress = E.prefill(G, 'update', device='cuda')
    lat_b, steps_b, _ = E.prefill(G, 'update', device='cuda')
    progress = progress.to(pdt)
    due = (steps_b <= progress).nonzero().flatten()
    assert G['edge_row'] in due.tolist() and G['below_row'] not in due.tolist() and due.tolist() == sc['env_ids']
    sa, sb = _state(SEED, 5), _state(SEED, 5)
    kw = dict(steps_add=True, steps_low=G['steps_low'], steps_high=G['steps_high'])
    be.latent_renew(lat_a, rng_state=sa, progress_buf=progress, reset_steps=steps_a, **kw)
    be.latent_renew(lat_b, env_ids=due.to(torch.int32), rng_state=sb, reset_steps=steps_b, **kw)
    assert torch.equal(lat_a, lat_b) and torch.equal(steps_a, steps_b) and sa.tolist() == sb.tolist() == [SEED, 6]
    lat0, steps0, progress0 = E.prefill(G, 'update')
    keep = [e for e in range(G['num_envs']) if e not in sc['env_ids']]
    assert torch.equal(lat_a.cpu()[keep], lat0[keep]) and torch.equal(steps_a.cpu()[keep], steps0[keep])
    assert bool((steps_a.cpu()[sc['env_ids']] > steps0[sc['env_ids']]).all()) and torch.equal(progress.cpu(), progress0.to(pdt))


# ---- 4. shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_envs', (1, 4, 5, 257))
@pytest.mark.parametrize('dim', (1, 63, 64, 65, 128))
def test_shapes_in_both_modes(be, n_envs, dim):
    g = torch.Generator().manual_seed(1000 * n_envs + dim)
    emu = E.EmuLatentRenew()
    # ids mode, passed-in draws: ld_z > dim and ld_eps > dim with NaN in the gaps, ids -1 and n_envs are skipped, the first
    # valid row's eps is all zero (-> zeros), the second one's last column is NaN (-> a NaN row)
    valid = torch.randperm(n_envs, generator=g)[:max(1, (n_envs + 1) // 2)].tolist()
    ids = [-1] + valid + [n_envs]
    eps = torch.full((len(ids), dim + 2), NAN)
    eps[:, :dim] = torch.randn(len(ids), dim, generator=g)
    eps[1, :dim] = 0.0
    if len(valid) > 1:
        eps[2, dim - 1] = NAN
    steps = torch.randint(1, 150, (len(ids),), generator=g, dtype=torch.int32)
    lat0, steps0 = E.pattern(n_envs, dim), torch.arange(n_envs, dtype=torch.int32) * 3 + 1
    wide = torch.full((n_envs, dim + 3), NAN)
    wide[:, :dim] = lat0
    wide, reset_steps = wide.cuda(), steps0.cuda()
    be.latent_renew(wide[:, :dim], env_ids=_i32(ids), eps=eps.cuda()[:, :dim], steps=steps.cuda(), reset_steps=reset_steps)
    ref = {}
    for dt in (torch.float32, torch.float64):
        ref[dt], s_ref = lat0.clone().to(dt), steps0.clone()
        emu.latent_renew(ref[dt], env_ids=torch.tensor(ids, dtype=torch.int32), eps=eps[:, :dim], steps=steps, reset_steps=s_ref)
    RR.within(wide[:, :dim], ref[torch.float64], ref[torch.float32], f'latent_renew ids {n_envs}x{dim}')
    assert bool(torch.isnan(wide[:, dim:]).all()) and torch.equal(reset_steps.cpu(), s_ref)
    assert not wide[valid[0], :dim].any() and (len(valid) < 2 or bool(torch.isnan(wide[valid[1], :dim]).all()))
    # due mode, device draws: whichever rows are due
    progress = torch.randint(0, 100, (n_envs,), generator=g, dtype=torch.int32)
    rs0 = (progress + torch.randint(-3, 4, (n_envs,), generator=g, dtype=torch.int32))
    latents, reset_steps, st = lat0.cuda(), rs0.cuda(), _state(SEED, OFFSETS[1])
    be.latent_renew(latents, rng_state=st, progress_buf=progress.cuda(), reset_steps=reset_steps, steps_add=True, steps_low=1, steps_high=150)
    for dt in (torch.float32, torch.float64):
        ref[dt], s_ref = lat0.clone().to(dt), rs0.clone()
        emu.latent_renew(ref[dt], rng_state=torch.tensor([SEED, OFFSETS[1]]), progress_buf=progress, reset_steps=s_ref, steps_add=True,
                         steps_low=1, steps_high=150)
    RR.within(latents, ref[torch.float64], ref[torch.float32], f'latent_renew due {n_envs}x{dim}')
    assert torch.equal(reset_steps.cpu(), s_ref) and st.tolist() == [SEED, OFFSETS[1] + 1]
    not_due = (rs0 > progress)
    assert torch.equal(latents.cpu()[not_due], lat0[not_due])


def test_one_id_and_the_empty_list(be):
    n, dim = 6, 64
    lat0 = E.pattern(n, dim)
    latents, st = lat0.cuda(), _state(SEED, 0)
    be.latent_renew(latents, env_ids=_i32([4]), rng_state=st)                                 # n_ids = 1, no steps bookkeeping
    want = RR.sample_latents(n, dim, SEED, 0)
    RR.within(latents[4:5], want[4:5], RR.sample_latents(n, dim, SEED, 0, dtype=torch.float32)[4:5], 'latent_renew one id')
    keep = [0, 1, 2, 3, 5]
    assert torch.equal(latents.cpu()[keep], lat0[keep]) and st.tolist() == [SEED, 1]
    after = latents.clone()
    steps = torch.full((n,), 9, dtype=torch.int32).cuda()
    be.latent_renew(latents, env_ids=_i32([]), rng_state=st, reset_steps=steps, steps_low=1, steps_high=150)     # a call is one position
    assert st.tolist() == [SEED, 2] and torch.equal(latents, after) and bool((steps == 9).all())
    be.latent_renew(latents, env_ids=_i32([]), rng_state=st, advance=False)
    be.latent_renew(latents, env_ids=_i32([]), eps=torch.zeros(0, dim).cuda())
    assert st.tolist() == [SEED, 2] and torch.equal(latents, after)


# ---- 5. the second output ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', (torch.float32, torch.float16, torch.bfloat16))
def test_second_output_holds_every_row(be, dt):
    n, dim, ld = 9, 65, 72
    g = torch.Generator().manual_seed(17)
    lat0 = torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1)
    progress = torch.full((n,), 50, dtype=torch.int64)
    rs0 = torch.tensor([40, 60, 50, 51, 49, 70, 10, 90, 55], dtype=torch.int32)
    due = (rs0 <= progress)
    assert 0 < int(due.sum()) < n
    wide = torch.full((n + 1, ld), RR.SENTINEL, dtype=dt).cuda()
    latents, reset_steps = lat0.cuda(), rs0.cuda()
    be.latent_renew(latents, rng_state=_state(SEED, 9), progress_buf=progress.cuda(), reset_steps=reset_steps, steps_add=True,
                    steps_low=1, steps_high=150, z2=wide[:n, :dim])
    assert torch.equal(wide[:n, :dim], latents.to(dt))                       # renewed and kept rows alike, exact conversion
    sentinel = torch.tensor(RR.SENTINEL, dtype=dt)
    assert bool((wide[:, dim:] == sentinel).all()) and bool((wide[n:] == sentinel).all())
    assert torch.equal(latents.cpu()[~due], lat0[~due]) and bool((latents.cpu()[due] != lat0[due]).any(dim=-1).all())


# ---- 6. a launch program -----------------------------------------------------------------------------------------------------
def test_due_mode_replays_in_a_launch_program(be, G):
    """Recorded once, replayed twice with progress_buf advanced in between: each replay renews what is due by the progress_buf
    it finds, on the stream position it finds; recording executes nothing."""
    N, dim = G['num_envs'], G['dim']
    kw = dict(steps_add=True, steps_low=G['steps_low'], steps_high=G['steps_high'])
    lat, steps, progress = E.prefill(G, 'update', device='cuda')
    lat2, steps2, _ = E.prefill(G, 'update', device='cuda')
    lat0, steps0 = lat.clone(), steps.clone()
    slot, slot2 = torch.zeros(N, dim).cuda(), torch.zeros(N, dim).cuda()
    st, st2 = _state(SEED, 1), _state(SEED, 1)
    prog = be.prog_create()
    be.prog_begin(prog)
    be.latent_renew(lat, rng_state=st, progress_buf=progress, reset_steps=steps, z2=slot, **kw)
    be.prog_end(prog)
    torch.cuda.synchronize()
    assert be.prog_size(prog) >= 1
    assert torch.equal(lat, lat0) and torch.equal(steps, steps0) and st.tolist() == [SEED, 1] and not slot.any()
    sizes = []
    for replay in range(2):
        due = (steps2 <= progress).nonzero().flatten()
        sizes.append(due.numel())
        be.latent_renew(lat2, env_ids=due.to(torch.int32), rng_state=st2, reset_steps=steps2, **kw)      # the eager ids-mode twin
        be.prog_launch(prog)
        torch.cuda.synchronize()
        assert torch.equal(lat, lat2) and torch.equal(steps, steps2) and torch.equal(slot, lat), replay
        assert st.tolist() == st2.tolist() == [SEED, replay + 2]
        progress += 40                                                     # the simulator's steps between two updates
    assert 0 < sizes[0] < N and sizes[1] > 0
    be.prog_destroy(prog)


# ---- 7. the torch op ---------------------------------------------------------------------------------------------------------
def test_torch_op_equals_the_backend_call(be, G):
    import ase_amd.ops  # noqa: F401
    op = torch.ops.ase_hip.latent_renew
    N, dim, lo, hi = G['num_envs'], G['dim'], G['steps_low'], G['steps_high']
    ids = _i32(G['scenarios']['reset_ids']['env_ids'])
    lat_a, steps_a, progress = E.prefill(G, 'update', device='cuda')
    lat_b, steps_b, _ = E.prefill(G, 'update', device='cuda')
    sa, sb = _state(SEED, 4), _state(SEED, 4)
    op(lat_a, ids, None, None, sa, True, None, steps_a, False, lo, hi, None)
    be.latent_renew(lat_b, env_ids=ids, rng_state=sb, reset_steps=steps_b, steps_low=lo, steps_high=hi)
    assert torch.equal(lat_a, lat_b) and torch.equal(steps_a, steps_b) and sa.tolist() == sb.tolist() == [SEED, 5]
    za, zb = torch.zeros(N, dim, dtype=torch.bfloat16).cuda(), torch.zeros(N, dim, dtype=torch.bfloat16).cuda()
    op(lat_a, None, None, None, sa, True, progress, steps_a, True, lo, hi, za)
    be.latent_renew(lat_b, rng_state=sb, progress_buf=progress, reset_steps=steps_b, steps_add=True, steps_low=lo, steps_high=hi, z2=zb)
    assert torch.equal(lat_a, lat_b) and torch.equal(steps_a, steps_b) and torch.equal(za, zb) and torch.equal(za, lat_a.to(torch.bfloat16))
    sc = G['scenarios']['reset_ids']
    lat_c, steps_c, _ = E.prefill(G, 'reset_ids', device='cuda')
    op(lat_c, ids, sc['eps'].cuda(), sc['steps'].cuda(), None, True, None, steps_c, False, lo, hi, None)
    lat_d, steps_d, _ = E.prefill(G, 'reset_ids', device='cuda')
    be.latent_renew(lat_d, reset_steps=steps_d, **E.call_of(G, 'reset_ids', 'cuda'))
    assert torch.equal(lat_c, lat_d) and torch.equal(steps_c, steps_d)
    with pytest.raises(RuntimeError):
        op(lat_c, ids.long(), None, None, sa, True, None, None, False, lo, hi, None)                      # env_ids must be int32


# ---- 8. the agent and the player -----------------------------------------------------------------------------------------------
@pytest.fixture
def boundary(monkeypatch):
    import tests.test_boundary_emu as T
    from ase_amd.backend import HipBackend
    monkeypatch.setattr(T, '_DEV', 'cuda:0')
    monkeypatch.setattr(T, '_BE', lambda: HipBackend('cuda:0'))
    return T


def test_agent_with_device_latents(boundary, golden_dir):
    T = boundary
    GA = T._load(golden_dir, 'ase')
    env, env_h = T._env(GA), T._env(GA)
    dev, cfg = T._agent(GA, env, device_latents=True)
    host, _ = T._agent(GA, env_h)
    N = env.num_envs
    # a full reset: bitwise the host path's latents, from the same stream position
    dev.obs, host.obs = dev.env_reset(), host.env_reset()
    assert torch.equal(dev._ase_latents, host._ase_latents) and bool(dev._ase_latents.any())
    assert dev.engine.rng_state.tolist() == host.engine.rng_state.tolist()
    lo, hi = int(dev._latent_steps_min), int(dev._latent_steps_max)
    assert bool(((dev._latent_reset_steps >= lo) & (dev._latent_reset_steps < hi)).all())
    # one horizon: record what each step's launch finds (copies, before it runs)
    seen = []
    update = dev._update_latents

    def recording_update():
        seen.append((env.progress_buf.clone(), dev._latent_reset_steps.clone(), dev._ase_latents.clone()))
        update()
    dev._update_latents = recording_update
    dev.play_steps()
    torch.cuda.synchronize()
    z = dev.experience['ase_latents']
    assert len(seen) == dev.horizon_length == z.shape[0]
    assert torch.allclose(z.norm(dim=-1), torch.ones(z.shape[:2], device=z.device), atol=1e-5)
    partial = 0
    for n, (progress, steps, before) in enumerate(seen):
        due = (steps.cpu() <= progress.cpu())                              # the host recomputation of the step's due set
        changed = (z[n] != before).any(dim=-1).cpu()
        assert torch.equal(changed, due), n
        partial += int(0 < int(due.sum()) < N)
        if n > 0:                                                          # between two slots: the due rows and the rows env_reset renewed
            reset_rows = (before != z[n - 1]).any(dim=-1).cpu()
            assert torch.equal((z[n] != z[n - 1]).any(dim=-1).cpu(), due | reset_rows), n
    assert partial > 0 and torch.equal(z[-1], dev._ase_latents)
    # the player
    pcfg = dict(cfg)
    pcfg.update(vec_env=T._env(GA, seed=4), env_info=None, backend=T._BE(), device_latents=True, player={'games_num': 1, 'print_stats': False})
    pl = T.PLAYERS['ase'](pcfg)
    pl._reset_latents()
    z0, count0 = pl._ase_latents.clone(), pl._latent_step_count
    pl._reset_latents([2, 5])
    changed = (pl._ase_latents != z0).any(dim=-1).nonzero().flatten().tolist()
    assert changed == [2, 5] and pl._latent_step_count == count0
    assert torch.allclose(pl._ase_latents.norm(dim=-1), torch.ones(N, device=z.device), atol=1e-5)
