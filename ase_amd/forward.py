"""MI355X forward engine: the layer table of an ASE / AMP / PPO network, its compute-dtype shadow weights, the running
statistics and the eval-mode forward passes of the rollout and of inference (policy_forward / policy_act / amp_heads) as
explicit sequences of HIP kernel launches.  Everything that only needs a forward pass - players, the network-level API of
``inference.InferenceEngine`` - builds a ``ForwardEngine``; the trainer is ``engine.UpdateEngine``, which derives from it and
adds the optimisation step.

Data layout in HBM
  * master parameters: one flat f32 buffer in checkpoint layout (the network's ``flat_params``);
  * per layer "shadow" copies in the compute dtype (bf16, f16 or f32): W_s [P(N), Kpad] and its
    transpose Wt_s [Kpad, P(N)], zero padded (P(x) = x rounded up to 64), rewritten by refresh_shadows; the concat inputs
    [obs | z] of the first actor/critic layer are laid out as [obs, pad to P(obs) | z], so the latent block starts on a
    128-byte boundary;
  * activations [rows, P(features)] in the compute dtype in persistent scratch that grows with the largest row count seen;
    head outputs in f32.
"""
import torch

from . import lib as L


def P(x, m=64):
    return (int(x) + m - 1) // m * m


# rl_games activations_factory names (learning/ase_network_builder.py:162) -> epilogue codes; 'swish' is SiLU
_ACT = {'relu': L.ACT_RELU, 'tanh': L.ACT_TANH, 'None': L.ACT_NONE, 'none': L.ACT_NONE, None: L.ACT_NONE,
        'swish': L.ACT_SILU, 'silu': L.ACT_SILU, 'elu': L.ACT_ELU, 'gelu': L.ACT_GELU, 'sigmoid': L.ACT_SIGMOID,
        'selu': L.ACT_SELU, 'softplus': L.ACT_SOFTPLUS}
# what the data-gradient epilogue multiplies by: ReLU - the activation's sign (bit-mask twin), tanh - 1 - y^2 of the output
# itself, the smooth activations - act'(z) of the pre-activation the forward launch kept in the layer's twin buffer
_AUX = {L.ACT_RELU: L.AUX_RELU_MASK, L.ACT_TANH: L.AUX_TANH_GRAD, L.ACT_NONE: L.AUX_NONE}
_AUX.update({a: L.AUX_PREACT | (a << 8) for a in range(L.ACT_SILU, L.ACT_SOFTPLUS + 1)})


class Dense:
    """One linear layer (or a group of heads sharing an input, stacked along N at 64-aligned offsets)."""

    def __init__(self, parts, k_in, act, split=None):
        # parts: list of (param prefix, n_real, row offset in the padded N dimension)
        self.parts = parts
        self.K = k_in
        self.act = _ACT[act] if not isinstance(act, int) else act
        if split is None:
            self.split_src = self.split_dst = k_in
            self.k_pad = P(k_in)
        else:
            self.split_src, self.split_dst, self.k_pad = split
        self.n_pad = max(off + P(n) for _, n, off in parts)
        self.N = parts[0][1]

    @property
    def name(self):
        return self.parts[0][0]


class ForwardEngine:
    """kind: 'ase' | 'amp' | 'ppo'.  cfg: read for normalize_input / normalize_value / normalize_amp_input / seed only."""

    def __init__(self, kind, net, cfg, backend, *, dtype=torch.bfloat16):
        self.kind, self.net, self.cfg, self.be = kind, net, cfg, backend
        self.dtype = dtype
        self.dev = net.flat_params.device
        # (rl_games default: normalize_value False)
        self.norm_value = bool(cfg.get('normalize_value', False))
        self.obs, self.act = net.obs_size, net.actions_num
        self.z = net.latent_dim if kind == 'ase' else 0
        self.amp = net.amp_obs_size if kind in ('amp', 'ase') else 0
        self.has_disc = kind in ('amp', 'ase')
        self.has_enc = kind == 'ase'
        self.enc_sep = bool(getattr(net, 'enc_separate', False))
        self.mu_tanh = kind == 'ppo' and getattr(net, 'mu_tanh', False)
        # the policy's log-std (network space.continuous): 'frozen' (learn_sigma False: the reference's configurations),
        # 'vector' (a learned state-independent vector, one bias-only row of the Adam table) or 'head' (the sigma head, stacked
        # beside mu in one head group: mu columns [0, act), log-std columns [64, 64 + act))
        self.sigma_mode = getattr(net, 'sigma_mode', 'frozen')
        self._scratch = {}
        self._frozen = {}            # eval statistics kept while the engine is frozen: frozen_stats / drop_frozen_stats
        self._refresh_desc = None
        self._build_layers()
        self._bind_params()
        self._alloc()
        self.refresh_shadows()

    # ------------------------------------------------------------------ structure
    def _build_layers(self):
        net, z = self.net, self.z
        act = net.activation
        split = (self.obs, P(self.obs), P(self.obs) + P(z)) if z else None
        self.style = []
        if self.kind == 'ase':
            k = z
            for i, u in enumerate(net.style_units):
                self.style.append(Dense([(f'actor_mlp._style_mlp.{2 * i}', u, 0)], k, act))
                k = u
            self.style.append(Dense([('actor_mlp._style_dense', z, 0)], k, 'tanh'))
            names_a = [f'actor_mlp._dense_layers.{i}' for i in range(len(net.units))]
            names_c = [f'critic_mlp._mlp.{2 * i}' for i in range(len(net.units))]
        else:
            names_a = [f'actor_mlp.{2 * i}' for i in range(len(net.units))]
            names_c = [f'critic_mlp.{2 * i}' for i in range(len(net.units))]
        self.actor, self.critic = [], []
        k = self.obs + z
        for i, u in enumerate(net.units):
            sp = split if (i == 0 and z) else None
            self.actor.append(Dense([(names_a[i], u, 0)], k, act, sp))
            self.critic.append(Dense([(names_c[i], u, 0)], k, act, sp))
            k = u
        if self.sigma_mode == 'head':
            self.mu_head = Dense([('mu', self.act, 0), ('sigma', self.act, P(self.act))], k, 'None')
        else:
            self.mu_head = Dense([('mu', self.act, 0)], k, 'None')
        self.value_head = Dense([('value', 1, 0)], k, 'None')
        self.disc, self.enc_chain = [], []
        self.disc_head = self.enc_head = None
        if self.has_disc:
            k = self.amp
            for i, u in enumerate(net.disc_units):
                self.disc.append(Dense([(f'_disc_mlp.{2 * i}', u, 0)], k, net.disc_activation))
                k = u
            parts = [('_disc_logits', 1, 0)]
            if self.has_enc and not self.enc_sep:
                parts.append(('_enc', z, P(1)))
            self.disc_head = Dense(parts, k, 'None')
            if self.has_enc and self.enc_sep:
                k = self.amp
                for i, u in enumerate(net.enc_units):
                    self.enc_chain.append(Dense([(f'_enc_mlp.{2 * i}', u, 0)], k, net.enc_activation))
                    k = u
                self.enc_head = Dense([('_enc', z, 0)], k, 'None')
        self.layers = (self.style + self.actor + [self.mu_head] + self.critic + [self.value_head] + self.disc +
                       ([self.disc_head] if self.disc_head else []) + self.enc_chain +
                       ([self.enc_head] if self.enc_head else []))

    def _bind_params(self):
        net, dev, T = self.net, self.dev, self.dtype
        self.params = net.flat_params
        net._engine_bound = True          # A2CNetwork._apply refuses to re-allocate the flat buffer from now on
        for d in self.layers:
            d.Ws = torch.zeros(d.n_pad, d.k_pad, dtype=T, device=dev)
            d.Wts = torch.zeros(d.k_pad, d.n_pad, dtype=T, device=dev)
            d.bs = torch.zeros(d.n_pad, dtype=torch.float32, device=dev)
            d.W, d.b = [], []
            for name, nr, off in d.parts:
                o, shp = net.param_slices[name + '.weight']
                assert tuple(shp) == (nr, d.K), (name, shp, nr, d.K)
                d.W.append(self.params[o:o + nr * d.K].view(nr, d.K))
                ob, _ = net.param_slices[name + '.bias']
                d.b.append(self.params[ob:ob + nr])
        self.logstd = None           # 'head': the log-std is the sigma columns of the head output
        if self.sigma_mode != 'head':
            o, shp = net.param_slices['sigma']
            self.logstd = self.params[o:o + shp[0]]

    def _latent_seed(self):
        """Seed of the engine's Philox latent streams."""
        return int(self.cfg.get('seed', 0))

    def _alloc(self):
        dev = self.dev
        self._bits = {}      # activation buffer (storage pointer) -> (buffer, twin); persistent scratch has no twins
        if self.style:
            # Philox stream of the ROLLOUT's latent draws {seed, offset} (sample_latents(n) of the network, read-then-advance):
            # seeded by the run, advanced on device, part of the checkpoint (CommonAgent.get_full_state_weights)
            self.rng_state = torch.tensor([self._latent_seed() ^ 0x5EED, 0], dtype=torch.int64, device=dev)
        if self.has_disc:
            self.amp_state = torch.zeros(2 * self.amp + 1, dtype=torch.float64, device=dev)
            self.amp_state[self.amp:] = 1.0
        self.obs_state = torch.zeros(2 * self.obs + 1, dtype=torch.float64, device=dev)
        self.obs_state[self.obs:] = 1.0
        self.val_state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ shadows
    def _shadow_rows(self):
        """Per layer part (d, j): the twelve fields [W, n_real, k_real, Ws, ldws, Wts, ldwts, split_src, gap, bias, bias_shadow,
        tiles_k] that open a row of the refresh table and of the optimizer's, and the tensors they point into."""
        for d in self.layers:
            for j, ((name, nr, off), W, b) in enumerate(zip(d.parts, d.W, d.b)):
                ws, wts, bs = d.Ws[off:], d.Wts[:, off:], d.bs[off:off + nr]
                yield d, j, [W.data_ptr(), nr, d.K, ws.data_ptr(), ws.stride(0), wts.data_ptr(), wts.stride(0), d.split_src,
                             d.split_dst - d.split_src, b.data_ptr(), bs.data_ptr(), (d.K + 31) // 32], \
                    (W, ws, wts, d.split_src, d.split_dst, b, bs)

    def refresh_shadows(self):
        """Master f32 weights -> compute-dtype shadows (W, W^T, padded bias) for every layer: one launch."""
        if self._refresh_desc is None:
            parts = list(self._shadow_rows())
            self._refresh_desc = torch.tensor([row for _, _, row, _ in parts], dtype=torch.int64, device=self.dev)
            self._refresh_items = [item for _, _, _, item in parts]
        self.be.refresh_shadow_multi(self._refresh_desc, self._refresh_items, self.dtype)

    # ------------------------------------------------------------------ primitive layer ops
    def _nt(self, *a, **kw):
        self.be.gemm_nt(*a, **kw)

    def _fwd(self, d, X, Y, rows, act=None):
        act = d.act if act is None else act
        self._nt(X, d.Ws, Y, rows, d.n_pad, d.k_pad, bias=d.bs, act=act,
                        mask_out=self._mask_of(Y) if (act == L.ACT_RELU or act >= L.ACT_SILU) else None)

    def _mask_of(self, h):
        """Bit-mask twin of (a row range of) an activation buffer, or None."""
        e = self._bits.get(h.untyped_storage().data_ptr()) if h is not None else None
        if e is None:
            return None
        base, bits = e
        off = (h.data_ptr() - base.data_ptr()) // base.element_size()
        r0, c0 = divmod(off, base.stride(0))
        if c0 != 0 or h.shape[1] != base.shape[1]:
            return None
        return bits[r0:r0 + h.shape[0]]

    def _fwd_chain(self, chain, X, H, rows):
        for d, h in zip(chain, H):
            self._fwd(d, X, h, rows)
            X = h
        return X

    # ------------------------------------------------------------------ inference (rollout side, epoch tail)
    def _scr(self, key, rows, cols, dt=None):
        dt = self.dtype if dt is None else dt
        k = (key, cols, dt)
        t = self._scratch.get(k)
        if t is None or t.shape[0] < rows:
            t = torch.zeros(rows, cols, dtype=dt, device=self.dev)
            self._scratch[k] = t
        return t[:rows]

    def _fwd_scr(self, key, chain, head, X, n, out):
        """A chain on n rows into per-layer scratch (f'{key}{i}'), then its head into `out`: the key of an f32 scratch
        buffer [n, head.n_pad], or a buffer of the caller's.  Returns the head's output."""
        for i, d in enumerate(chain):
            y = self._scr(f'{key}{i}', n, d.n_pad)
            self._fwd(d, X, y, n)
            X = y
        Y = self._scr(out, n, head.n_pad, torch.float32) if isinstance(out, str) else out
        self._fwd(head, X, Y, n)
        return Y

    def _eval_stats(self, state, D, key):
        mean, std = self._scr(key + '_m', 1, D, torch.float32), self._scr(key + '_s', 1, D, torch.float32)
        self.be.rms_finalize(state, D, None, 0, 0, mean, std)
        return mean[0], std[0]

    def frozen_stats(self, which):
        """Eval mean / std of the 'obs' or 'amp' normaliser, computed ONCE and kept while the engine is frozen (a low-level
        controller's statistics never change): the per-call rms_finalize of _eval_stats, hoisted.  Whoever writes the running
        statistics - set_stats_weights, restore, set_train - calls drop_frozen_stats.  Without input normalisation: 0 / 1."""
        hit = self._frozen.get(which)
        if hit is None:
            state, D, key = ((self.obs_state, self.obs, 'normalize_input') if which == 'obs' else
                             (self.amp_state, self.amp, 'normalize_amp_input'))
            mean = torch.zeros(1, D, dtype=torch.float32, device=self.dev)
            std = torch.ones(1, D, dtype=torch.float32, device=self.dev)
            if self.cfg.get(key, True):
                self.be.rms_finalize(state, D, None, 0, 0, mean, std)
            hit = self._frozen[which] = (mean[0], std[0])
        return hit

    def drop_frozen_stats(self):
        self._frozen.clear()

    def style_input(self, n):
        """The style chain's input buffer [n, P(z)] in the compute dtype: what hrl_latent's z2 writes for policy_mu_frozen."""
        return self._scr('Zs', n, P(self.z))

    def policy_mu_frozen(self, obs):
        """The mu-only pass of a frozen ASE controller (learning/hrl_agent.py:231-237): obs is a [n, >= obs] VIEW read at its own
        pitch (no copy), normalised with frozen_stats into the actor input only; the style input is taken as already written
        (style_input); then the style chain, the actor chain and the mu head, one launch per dense layer.  Returns the padded
        head output f32 [n, P(act)], persistent scratch.  No critic input, no gather, no rms_finalize."""
        assert self.kind == 'ase' and self.style, "policy_mu_frozen: an ASE controller"
        n, a0 = obs.shape[0], self.actor[0]
        Xa = self._scr('Xa', n, a0.k_pad)
        mean, std = self.frozen_stats('obs')
        self.be.rms_normalize(obs, self.obs, None, (0, 0), n, mean, std, [Xa])
        self._fwd_scr('Hs', self.style[:-1], self.style[-1], self.style_input(n), n, Xa[:, a0.split_dst:])
        return self._fwd_scr('Ha', self.actor, self.mu_head, Xa, n, 'MU')

    def rollout_stats(self):
        """Eval mean / std of the observation normaliser for the steps of ONE rollout, in persistent buffers of their own
        (their addresses are baked into a recorded rollout step): the statistics do not change inside a rollout - play_steps
        begins with set_eval, and rms_finalize without sums is a pure function of the state - so a caller computes them once,
        before the first step, and nothing inside the recording re-finalises them.  Without input normalisation: 0 / 1."""
        hit = self._scratch.get('rollout_stats')
        if hit is None:
            hit = self._scratch['rollout_stats'] = (torch.zeros(1, self.obs, dtype=torch.float32, device=self.dev),
                                                    torch.ones(1, self.obs, dtype=torch.float32, device=self.dev))
        if self.cfg.get('normalize_input', True):
            self.be.rms_finalize(self.obs_state, self.obs, None, 0, 0, hit[0], hit[1])
        return hit[0][0], hit[1][0]

    def rollout_head(self, obs, z, mean, std, obses_out=None, latents_out=None, slot=0, slot_dev=None, critic_only=False):
        """The persistent Xa / Xc / Zs scratch of _policy_nets filled by ONE rollout_head launch from raw observations
        [n, obs] and the latents z [n, z] (None without a latent): the normalisation with mean / std (rollout_stats) into the
        actor's and the critic's input, the latents into the critic's concat block and the style input, and - obses_out
        [H, n, obs], latents_out [H, n, z] - the raw rows into experience slot `slot` / the device word slot_dev.
        critic_only: Xc and its concat block alone (the _next_values pass).  policy_act / policy_forward(inputs_ready=True)
        run the chains on what this call wrote."""
        n, a0 = obs.shape[0], self.actor[0]
        Xc = self._scr('Xc', n, a0.k_pad)
        zc = Xc[:, a0.split_dst:] if self.z else None
        if critic_only:
            self.be.rollout_head(obs, z if self.z else None, mean, std, xc=Xc, zc=zc)
            return
        Xa = self._scr('Xa', n, a0.k_pad)
        zs = self._scr('Zs', n, P(self.z)) if self.style else None
        self.be.rollout_head(obs, z if self.z else None, mean, std, xa=Xa, xc=Xc, zc=zc, zs=zs, obses_out=obses_out,
                             z_out=latents_out if self.z else None, slot=slot, slot_dev=slot_dev)

    def _policy_nets(self, obs, z, normalize, want_mu, want_value, inputs_ready=False):
        """Eval-mode observation normalisation + actor / critic forward on raw observations [n, obs].  Returns the padded
        head outputs (MU f32 [n, P(act)] before any tanh, V f32 [n, 64]); every buffer is persistent scratch.
        inputs_ready: Xa / Xc / Zs already hold this step's inputs (rollout_head wrote them): no _eval_stats, no
        rms_normalize, no gather_rows - the chains alone; obs gives the row count only."""
        be, n = self.be, obs.shape[0]
        f32 = torch.float32
        a0 = self.actor[0]
        Xa, Xc = self._scr('Xa', n, a0.k_pad), self._scr('Xc', n, a0.k_pad)
        if not inputs_ready:
            if normalize and self.cfg.get('normalize_input', True):
                mean, std = self._eval_stats(self.obs_state, self.obs, 'obs')
            else:
                mean, std = self._scr('one_m', 1, self.obs, f32)[0].zero_(), self._scr('one_s', 1, self.obs, f32)[0].fill_(1.0)
            be.rms_normalize(obs, self.obs, None, (0, 0), n, mean, std, [Xa, Xc])
        MU = V = None
        if self.z and not inputs_ready:
            sd = a0.split_dst
            be.gather_rows(z, self.z, None, (0, 0), n, Xc[:, sd:])
        if want_mu:
            if self.style:
                Zs = self._scr('Zs', n, P(self.z))
                if not inputs_ready:
                    be.gather_rows(z, self.z, None, (0, 0), n, Zs)
                self._fwd_scr('Hs', self.style[:-1], self.style[-1], Zs, n, Xa[:, a0.split_dst:])
            MU = self._fwd_scr('Ha', self.actor, self.mu_head, Xa, n, 'MU')
        if want_value:
            V = self._fwd_scr('Hc', self.critic, self.value_head, Xc, n, 'V')
        return MU, V

    def _value_out(self, V, n, unnorm_value, key='value_out'):
        """Column 0 of the padded value head -> dense [n, 1] (un-normalised like RunningMeanStd(unnorm=True))."""
        v = self._scr(key, n, 1, torch.float32)
        self.be.gather_rows(V, 1, None, (0, 0), n, v)
        if unnorm_value and self.norm_value:
            self.be.rms_unnormalize(self.val_state, v, v)
        return v

    def _logstd_of(self, MU):
        """The log-std operand of the loss / sampling heads: the vector, or (sigma head) the log-std columns of the head output."""
        if self.sigma_mode == 'head':
            off = self.mu_head.parts[1][2]
            return MU[:, off:off + self.act]
        return self.logstd

    def policy_forward(self, obs, z=None, normalize=True, unnorm_value=True, want=('mu', 'value'), inputs_ready=False):
        """Eval-mode actor / critic on raw observations [n, obs] (learning/ase_agent.py:117-148,385-393):
        eval-mode obs normalisation -> nets -> (mu [n, act], value [n, 1] un-normalised).  The returned tensors are
        persistent scratch, overwritten by the next call with the same n.  inputs_ready: the input buffers were filled by
        rollout_head, the call runs the chains alone (_policy_nets); unset, the call sequence is exactly what it was before
        the argument existed."""
        n = obs.shape[0]
        MU, V = self._policy_nets(obs, z, normalize, 'mu' in want or 'logstd' in want, 'value' in want, inputs_ready)
        out = {}
        if 'mu' in want:
            mu = self._scr('mu_out', n, self.act, torch.float32)
            self.be.gather_rows(MU, self.act, None, (0, 0), n, mu)
            out['mu'] = torch.tanh_(mu) if self.mu_tanh else mu
        if 'logstd' in want:          # per row [n, act] (the sigma head's output, no activation), or the vector [act]
            if self.sigma_mode == 'head':
                ls = self._scr('logstd_out', n, self.act, torch.float32)
                self.be.gather_rows(self._logstd_of(MU), self.act, None, (0, 0), n, ls)
                out['logstd'] = ls
            else:
                out['logstd'] = self.logstd
        if 'value' in want:
            out['value'] = self._value_out(V, n, unnorm_value)
        return out

    def policy_act(self, obs, z, rand_probs, rng_state, inputs_ready=False):
        """One rollout step of get_action_values (learning/amp_agent.py:139-169, learning/ase_agent.py:117-148) as an
        explicit launch sequence: normalise -> actor + critic -> ase_hip_sample_actions (tanh / Normal sample / neglogp /
        eps-greedy on device) -> value un-normalisation.  rand_probs None: every row stochastic (plain PPO).
        inputs_ready: the input buffers were filled by rollout_head, the normalise step is skipped (_policy_nets); unset, the
        call sequence is exactly what it was before the argument existed."""
        n, f32 = obs.shape[0], torch.float32
        MU, V = self._policy_nets(obs, z, True, True, True, inputs_ready)
        o = {k: self._scr('act_' + k, n, c, f32) for k, c in (('mus', self.act), ('sigmas', self.act), ('actions', self.act),
                                                             ('neglogpacs', 1), ('rand_action_mask', 1))}
        kw = dict(logstd_rows=True) if self.sigma_mode == 'head' else {}
        self.be.sample_actions(MU, self._logstd_of(MU), rand_probs, rng_state, o['mus'], o['sigmas'], o['actions'],
                               o['neglogpacs'], o['rand_action_mask'] if rand_probs is not None else None, n, self.act,
                               self.mu_tanh, **kw)
        res = {'neglogpacs': o['neglogpacs'].view(-1), 'values': self._value_out(V, n, True, 'act_values'),
               'actions': o['actions'], 'mus': o['mus'], 'sigmas': o['sigmas'], 'rnn_states': None}
        if rand_probs is not None:
            res['rand_action_mask'] = o['rand_action_mask'].view(-1)
        return res

    def amp_heads(self, amp_obs, normalize=True, frozen=False, want_enc=True):
        """Eval-mode discriminator logits [n,1] (+ un-normalised encoder output [n,z]) on raw amp obs
        (learning/amp_agent.py:547-549, learning/ase_agent.py:480-482).  frozen: the statistics of frozen_stats, no rms_finalize.
        want_enc False: a separate encoder chain is not run (the HRL inner loop reads the logit alone)."""
        be, n = self.be, amp_obs.shape[0]
        f32 = torch.float32
        X = self._scr('Xd', n, self.disc[0].k_pad)
        if frozen:
            assert normalize, "amp_heads: frozen statistics are the normalised pass"
            mean, std = self.frozen_stats('amp')
        elif normalize and self.cfg.get('normalize_amp_input', True):
            mean, std = self._eval_stats(self.amp_state, self.amp, 'amp')
        else:
            mean, std = self._scr('one_am', 1, self.amp, f32)[0].zero_(), self._scr('one_as', 1, self.amp, f32)[0].fill_(1.0)
        be.rms_normalize(amp_obs, self.amp, None, (0, 0), n, mean, std, [X])
        HD = self._fwd_scr('Hd', self.disc, self.disc_head, X, n, 'HD')
        enc = None
        if self.has_enc and want_enc:
            if self.enc_sep:
                enc = self._fwd_scr('He', self.enc_chain, self.enc_head, X, n, 'E')
            else:
                enc = HD[:, self.disc_head.parts[1][2]:]
        return HD, enc
