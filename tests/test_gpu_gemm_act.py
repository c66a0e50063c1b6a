"""The activation family of ase_hip_gemm_nt, its data-gradient epilogue and its non-finite contract on the GPU, against the f64
reference of tests/ref_gemm_act.py (torch.nn.functional and autograd on a KNOWN pre-activation - not the emulator).

test_activation: tanh and the six smooth activations, forward (the z twin bitwise, tanh's bit twin, column sums, out_f32, a scale
  record) and backward (ASE_AUX_PREACT / ASE_AUX_TANH_GRAD, a stacked block) in every storage mode on the smallest slab shapes of the
  cheap leaves; SiLU and tanh once more per remaining slab instantiation.  Bound: 2 e_ref + 2^-23 max |ref| + half a storage ulp per
  band of z, planted tail values one by one (the module states the rule and its two derived floors).
test_non_finite: NaN of both signs in A and the bias, +-inf in the bias (h3: an operand beyond half's range) through the
  row-per-lane and the slab epilogue: what torch.relu / tanh / sigmoid store, the overflow record, mask_out, colsum, and every
  element the plants do not reach bitwise what the same launch gives without them.

Every launch goes into views of larger sentinel-filled buffers (ldc > N and ldmask > N with column offsets, lda / ldb / ldaux
padded, rows after M), every sentinel checked after each launch; the kernel id of each shape is asserted first.
ASE_GEMM_ACT_REPORT=<file> writes the observed maxima beside their e_ref (for COVERAGE.md); nothing observed is asserted."""
import json
import os

import pytest

from tests import ref_gemm as R
from tests import ref_gemm_act as G

pytestmark = pytest.mark.gpu

CASES = G.cases()
NF_CASES = G.nf_cases()
REPORT, SEEN, COUNTS = {}, {}, {'cases': 0, 'elements': 0, 'nf_cases': 0, 'nf_elements': 0}


@pytest.fixture(scope='module')
def backends():
    from ase_amd.backend import HipBackend
    plain = HipBackend()
    yield {'bf16': plain, 'f16': plain, 'f32': plain, 'x3': HipBackend(x3=True), 'h3': HipBackend(x3='f16')}
    out = os.environ.get('ASE_GEMM_ACT_REPORT')
    if out:
        with open(out, 'w') as f:
            json.dump({'max |hip - f64|, e_ref, allowance': {' | '.join(k): v for k, v in sorted(REPORT.items())},
                       'non-finite': SEEN, 'counts': COUNTS}, f, indent=1)


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_activation(backends, c):
    be = backends[c.store]
    assert be.lib.ase_hip_gemm_nt_kernel_id(c.M, c.N, c.K, R.STORE_CODE[c.store]) == c.kid
    COUNTS['elements'] += G.launch_and_check(be, G.build(c), dev=be.device, report=REPORT)
    COUNTS['cases'] += 1


@pytest.mark.parametrize('c', NF_CASES, ids=[c.id for c in NF_CASES])
def test_non_finite(backends, c):
    be = backends[c.store]
    assert be.lib.ase_hip_gemm_nt_kernel_id(c.M, c.N, c.K, R.STORE_CODE[c.store]) == c.kid
    COUNTS['nf_elements'] += G.nf_run(be, c, dev=be.device, record_seen=SEEN, colsum_report=REPORT)
    COUNTS['nf_cases'] += 1


def test_relu_of_negative_zero_is_positive_zero(backends):
    """z = -0 (alpha = -1 on an all-zero product, bias -0): ReLU stores +0 on the row-per-lane and on the slab epilogue (a column
    sum sends the launch there) alike, as max(z, 0) did before it kept NaN."""
    import torch
    from ase_amd.lib import ACT_RELU
    be = backends['bf16']
    for dt in (torch.bfloat16, torch.float16):
        A = torch.zeros(64, 64, dtype=dt, device=be.device)
        B = torch.ones(64, 64, dtype=dt, device=be.device)
        bias = torch.full((64,), -0.0, device=be.device)
        for cs in (None, torch.zeros(64, device=be.device)):
            C = torch.full((64, 64), -7.0, dtype=dt, device=be.device)
            be.gemm_nt(A, B, C, 64, 64, 64, bias=bias, act=ACT_RELU, alpha=-1.0, colsum=cs, colsum_n=0 if cs is None else 64)
            assert bool((C.cpu().view(torch.int16) == 0).all()), (dt, 'slab' if cs is not None else 'rows')
