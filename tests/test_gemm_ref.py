"""The exact NT cases (tests/ref_gemm.py) on the CPU: every builder condition holds, the emulator's gemm_nt equals the f64
reference bit for bit - C, the mask_out words, the column sums - and every leaf shape reports the kernel id written next to it
(ase_hip_gemm_nt_kernel_id is a host-only call).  The GPU twin of this file is tests/test_gpu_gemm_exact.py."""
import pytest

from ase_amd import lib as L
from tests import ref_gemm as R
from tests.emu_backend import EmuBackend

CASES = R.cases()


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_emulator_equals_exact_reference(c):
    b = R.build(c)                      # asserts the conditions
    emu = EmuBackend()
    if c.store == 'h3':
        emu.x3 = 'f16'
    R.launch_and_check(emu, b)


def test_leaf_shapes_report_their_kernel_id():
    lib = L.load()
    for M, N, K, code, kid in R.leaf_shapes():
        assert lib.ase_hip_gemm_nt_kernel_id(M, N, K, code) == kid, (M, N, K, code, kid)


def test_case_list_covers_every_leaf_mode_and_variant():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for store in ('bf16', 'f16'):
        for _, leaf, shapes in R.LEAVES_16:
            if leaf == 'wave4-ragged':                # an extra on top of 'wave4': two variants by design (R.WAVE4_RAGGED)
                continue
            names = {c.variant for c in CASES if c.leaf == leaf and c.store == store}
            want = {n for n in R.VARIANTS if not n.startswith('saturate') or store == 'f16'}
            if all(N % 32 for _, N, _ in shapes):
                want = {n for n in want if not n.startswith('maskout')}
            if all(M < 8 for M, _, _ in shapes):
                want.discard('aux_bits_stacked')
            assert want <= names, (leaf, store, want - names)
    # the defect this list was written for: mask_out without ReLU, on every 16-bit shape the row-per-lane epilogue can take
    assert sum(c.variant == 'maskout_none' for c in CASES) >= 20
