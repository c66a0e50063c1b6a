"""Plain-torch restatement of ``HipBackend.latent_renew`` with the same signature, the host statement of its
device draws, and the helpers of the fixture tests/golden/latent_renew.pt (scripts/make_golden_latent_renew.py).
TEST INFRASTRUCTURE ONLY: the CPU stand-in for the backend in the host tests and the f64 leg of the fixture.

Written from the contract in include/ase_hip.h, following learning/ase_agent.py:310-379 and
learning/ase_network_builder.py:221-225 of the reference.  The arithmetic runs in the dtype of ``latents``: f32 repeats the
reference's operations, f64 is the yardstick on the same f32 normals cast up (device draws: the stream's normals evaluated in
f64, tests/ref_rollout.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import ref_rollout as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SCENARIOS = ('reset_ids', 'reset_all', 'update')


# ---- the device draws, stated on the host ------------------------------------------------------------------------------------
def reduce_steps(word, low, high):
    """The step count of a 32-bit word: low + floor(word * (high - low) / 2^32), exact integers, in [low, high)."""
    return int(low) + ((int(word) * (int(high) - int(low))) >> 32)


def device_draws(ids, dim, seed, offset, low=0, high=1, dtype=torch.float32):
    """(normals [n, dim] in dtype, steps int32 [n]) as ase_hip_latent_renew draws them for the environments ids: normal j of
    environment e is the normal of element e * dim + j of the stream at (seed, offset) - row e of latent_elems(n_envs, dim) -,
    the step count comes from word 3 of element e * dim."""
    ids = [int(e) for e in ids]
    if not ids:
        return torch.zeros(0, dim, dtype=dtype), torch.zeros(0, dtype=torch.int32)
    elems = np.concatenate([RR.latent_elems(1, dim, e) for e in ids], axis=0)
    eps = RR.normals(elems, offset, seed, dtype).to(dtype)
    w3 = RR.philox4x32_10(elems[:, 0].copy(), offset, seed)[3]
    return eps, torch.tensor([reduce_steps(w, low, high) for w in w3.tolist()], dtype=torch.int32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
class EmuLatentRenew:
    name = "emu-latent-renew"
    device = torch.device('cpu')

    def latent_renew(self, latents, env_ids=None, eps=None, steps=None, rng_state=None, advance=True, progress_buf=None,
                     reset_steps=None, steps_add=False, steps_low=0, steps_high=1, z2=None):
        n, dim = latents.shape
        dt = latents.dtype
        assert 1 <= dim <= 128 and n > 0
        assert (eps is None) != (rng_state is None), 'exactly one draw source'
        assert (steps is not None) == (eps is not None and reset_steps is not None), 'steps comes with eps and reset_steps'
        if env_ids is None:
            assert eps is None and progress_buf is not None and reset_steps is not None and steps_add, 'due mode'
            ids = torch.arange(n)[reset_steps <= progress_buf]                   # learning/ase_agent.py:367, rows in order
        else:
            assert progress_buf is None and z2 is None, 'ids mode'
            ids = env_ids.long()
            keep = (ids >= 0) & (ids < n)                                        # ids outside the buffers are skipped
            ids = ids[keep]
            if eps is not None:
                eps, steps = eps[keep], None if steps is None else steps[keep]
        if eps is None:
            assert reset_steps is None or 0 < int(steps_high) - int(steps_low) <= 0xFFFFFFFF
            eps, steps = device_draws(ids.tolist(), dim, int(rng_state[0]), int(rng_state[1]), steps_low, steps_high, dt)
            if advance:
                rng_state[1] += 1
        if ids.numel() > 0:
            latents[ids] = F.normalize(eps[:, :dim].to(dt), dim=-1)              # the normals are f32 values in both runs
            if reset_steps is not None:
                reset_steps[ids] = (reset_steps[ids] + steps.to(reset_steps.dtype)) if steps_add else steps.to(reset_steps.dtype)
        if z2 is not None:
            z2[:, :dim] = latents.to(z2.dtype)


# ---- the fixture tests/golden/latent_renew.pt (scripts/make_golden_latent_renew.py) -------------------------------------------
def load_fixture():
    return torch.load(os.path.join(GOLDEN, 'latent_renew.pt'), weights_only=False)


def pattern(*shape):
    """The latents before a scenario: an arithmetic pattern, so that untouched rows are detectable."""
    n = int(np.prod(shape))
    return ((torch.arange(n) * 7919) % 2003).to(torch.float32).view(*shape) / 100.0 - 10.0


def prefill(G, name, dtype=torch.float32, device='cpu'):
    """The state before a scenario -> (latents [N, dim] in dtype, reset_steps int32 [N], progress_buf int64 [N] or None)."""
    N, dim = G['num_envs'], G['dim']
    sc = G['scenarios'][name]
    latents = pattern(N, dim).to(dtype).to(device)
    if name == 'update':
        return latents, sc['reset_steps0'].clone().to(device), sc['progress_buf'].clone().to(device)
    return latents, (torch.arange(N, dtype=torch.int32) * 13 + 5).to(device), None


def call_of(G, name, device='cpu'):
    """A scenario as the keyword arguments of an ids-mode latent_renew on the recorded draws ('update': its due list, steps
    added)."""
    sc = G['scenarios'][name]
    return dict(env_ids=torch.tensor(sc['env_ids'], dtype=torch.int32, device=device), eps=sc['eps'].to(device),
                steps=sc['steps'].to(device), steps_add=name == 'update', steps_low=G['steps_low'], steps_high=G['steps_high'])


def expected(G, name, dtype=torch.float64):
    """A scenario's result by the restatement on the recorded f32 draws -> (latents in dtype, reset_steps)."""
    latents, reset_steps, _ = prefill(G, name, dtype)
    EmuLatentRenew().latent_renew(latents, reset_steps=reset_steps, **call_of(G, name))
    return latents, reset_steps


def allowance(G, name):
    """The bar of the device tests: max |x - f64| <= 2 e_ref + 1e-7, e_ref = what the reference's own f32
    normalisation loses against f64 on the recorded normals."""
    return 2.0 * G['scenarios'][name]['e_ref'] + 1e-7
