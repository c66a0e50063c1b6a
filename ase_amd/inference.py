"""Forward-only use of the HIP engine behind the network-level API (eval_actor / eval_critic /
eval_disc / eval_enc / sample_latents; learning/ase_network_builder.py:115-144,214-225 and
learning/amp_network_builder.py:51-84 under /root/reference/ase).  Inputs are already-normalised
observations, as in the reference."""
import torch

from .forward import ForwardEngine


class InferenceEngine:
    def __init__(self, net, engine=None, dtype=torch.bfloat16):
        if engine is None:
            from .backend import HipBackend
            cfg = {'normalize_input': True, 'normalize_value': True, 'normalize_amp_input': True}
            engine = ForwardEngine(net.kind, net, cfg, HipBackend(net.flat_params.device), dtype=dtype)
        self.eng = engine

    def refresh(self):
        self.eng.refresh_shadows()

    def actor(self, obs, z=None):
        return self.eng.policy_forward(obs, z, normalize=False, want=('mu',))['mu']

    def actor_logstd(self, obs, z=None):
        """(mu, per-row log-std) of a policy with a sigma head: one actor forward."""
        out = self.eng.policy_forward(obs, z, normalize=False, want=('mu', 'logstd'))
        return out['mu'], out['logstd']

    def critic(self, obs, z=None):
        return self.eng.policy_forward(obs, z, normalize=False, unnorm_value=False, want=('value',))['value']

    def disc(self, amp_obs):
        HD, _ = self.eng.amp_heads(amp_obs, normalize=False)
        return HD[:, 0:1].clone()

    def enc(self, amp_obs):
        _, e = self.eng.amp_heads(amp_obs, normalize=False)
        e = e[:, :self.eng.z]
        return e / e.norm(dim=-1, keepdim=True).clamp_min(1e-12)

    def sample_latents(self, n):
        z = torch.empty(n, self.eng.z, dtype=torch.float32, device=self.eng.dev)
        self.eng.be.sample_latents(z, n, self.eng.z, self.eng.rng_state)
        return z
