"""Every leaf of ase_hip_gemm_nt, bitwise: the HIP kernels against the exact f64 reference of tests/ref_gemm.py.

The operands are integers (tests/ref_gemm.py states and asserts the conditions), so every f32 partial sum is exact in any order
and what a launch stores is one correctly rounded conversion of a known number: C, the mask_out words and the column sums are
compared with torch.equal, there is no tolerance in this file.  One case = one launch on a leaf shape (the kernel id is asserted
first) in one storage mode with one epilogue variant, into views of larger sentinel-filled buffers that must come back intact
outside the call's rectangle.  The reference is tests/ref_gemm.py, NOT the emulator; tests/test_gemm_ref.py runs the same list
through the emulator on the CPU.

`maskout_none` (mask_out without ReLU on the shapes whose other launches take the row-per-lane epilogue) pins the defect recorded
in ADVICE.md: rows_frag formed the bit from min(pattern, 1), which is 0 or 1 only behind ReLU."""
import pytest

from tests import ref_gemm as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


@pytest.fixture(scope='module')
def backends():
    from ase_amd.backend import HipBackend
    plain = HipBackend()
    return {'bf16': plain, 'f16': plain, 'f32': plain, 'x3': HipBackend(x3=True), 'h3': HipBackend(x3='f16')}


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_kernel_equals_exact_reference(backends, c):
    be = backends[c.store]
    assert be.lib.ase_hip_gemm_nt_kernel_id(c.M, c.N, c.K, R.STORE_CODE[c.store]) == c.kid
    R.launch_and_check(be, R.build(c), dev=be.device)
