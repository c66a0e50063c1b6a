"""Golden vectors of the learned action log-std (network ``space.continuous.learn_sigma: True``), recorded from the
reference's own code through oracle/make_golden.py.  TEST INFRASTRUCTURE ONLY (needs the reference tree).

    python scripts/make_golden_sigma.py        # writes tests/golden/{ase_lsig,ase_sighead,amp_sighead,ppo_sighead}_tiny.pt

Nothing under oracle/ changes: this process swaps a wrapped ``_case`` into oracle.make_golden that turns on the two
learned forms of rl_games' A2CBuilder and a non-zero entropy coefficient (the only loss term besides neglogp whose
gradient reaches the log-std), then calls the unmodified ``make_case`` with the existing kinds 'ase', 'amp', 'ppo'.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg  # noqa: E402

VECTOR = {'name': 'const_initializer', 'val': -2.9}
# a Linear weight must not be constant: const -2.9 would make the log-std -2.9 * sum(actor_out)
HEAD = {'name': 'random_uniform_initializer', 'a': -0.02, 'b': 0.02}

_orig_case = mg._case


def _wrap(fixed, sigma_init):
    def _case(kind):
        net, cfg = _orig_case(kind)
        sp = net['space']['continuous']
        sp.update(learn_sigma=True, fixed_sigma=fixed, sigma_init=dict(sigma_init))
        cfg['entropy_coef'] = 0.01
        return net, cfg
    return _case


CASES = [  # (file, kind, fixed_sigma, sigma_init, seed)
    ('ase_lsig_tiny', 'ase', True, VECTOR, 70),
    ('ase_sighead_tiny', 'ase', False, HEAD, 71),
    ('amp_sighead_tiny', 'amp', False, HEAD, 72),
    ('ppo_sighead_tiny', 'ppo', False, HEAD, 73),
]

if __name__ == '__main__':
    torch.set_num_threads(4)
    only = set(sys.argv[1:])
    for name, kind, fixed, init, seed in CASES:
        if only and name not in only:
            continue
        mg._case = _wrap(fixed, init)
        mg.make_case(name, kind, seed=seed, epochs=1, regen=True, seeded=True, slim=True, sample=4096)
    mg._case = _orig_case
