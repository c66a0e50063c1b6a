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


# ---------------------------------------------------------------------------------------------------------------- TN (weight gradients)
# The exact TN cases (tests/ref_gemm_tn.py) on the CPU; the GPU twin is tests/test_gpu_gemm_tn_exact.py.
import torch  # noqa: E402

from tests import ref_gemm_tn as T  # noqa: E402

TN_CASES = T.cases()
TN_GROUPS = [(name, store, kw) for store in ('bf16', 'f16') for name, kw in
             [('tiles', {}), ('splits', {}), ('shared', {}), ('all', {}), ('shared', dict(alpha=4.0, factor=0.5)), ('tiles', dict(poison=True))]]


@pytest.mark.parametrize('c', TN_CASES, ids=[c.id for c in TN_CASES])
def test_tn_emulator_equals_exact_reference(c):
    b = T.build(c)                      # asserts the conditions
    n, bad, sent = T.launch_and_check(EmuBackend(), b)
    assert n > 0 and bad == 0 and sent > 0


@pytest.mark.parametrize('name,store,kw', TN_GROUPS, ids=[f'{n}-{s}-' + '_'.join(k) for n, s, k in TN_GROUPS])
def test_tn_grouped_emulator_equals_exact_reference(name, store, kw):
    g = T.build_group(name, store, **kw)
    _, n, bad, sent = T.launch_group_and_check(EmuBackend(), g)
    assert n > 0 and bad == 0 and sent > 0


def test_tn_cases_report_their_kernel_id():
    lib = L.load()
    for c in TN_CASES:
        assert T.kernel_id(lib, c) == c.kid, c.id
    M, N, K, nr, kr, ss, sd, br = T.PHASED[0]
    # what moves a phased shape off its kernel: ragged rows, a ragged bias limit, 4-byte storage, operands past 2 GiB
    assert lib.ase_hip_gemm_tn_kernel_id(M, N, K, nr, br, N, K, L.BF16) == 1
    assert lib.ase_hip_gemm_tn_kernel_id(M, N, K, nr, 0, N, K, L.F16) == 1
    assert lib.ase_hip_gemm_tn_kernel_id(M, N, K, nr, br + 8, N, K, L.BF16) == 0
    assert lib.ase_hip_gemm_tn_kernel_id(M - 64, N, K, nr, br, N, K, L.BF16) == 0
    assert lib.ase_hip_gemm_tn_kernel_id(M, N, K, nr, br, N, K, L.F32) == 0
    assert lib.ase_hip_gemm_tn_kernel_id(M, N, K, nr, br, 8192, K, L.BF16) == 0


def test_tn_case_list_covers_every_path_mode_and_variant():
    ids = [c.id for c in TN_CASES]
    assert len(set(ids)) == len(ids)
    for s16, s32 in T.T128:
        for store, shape in (('bf16', s16), ('f16', s16), ('f32', s32), ('x3', s32)):
            if shape is None:
                continue
            names = {c.variant for c in TN_CASES if c.shape == shape and c.store == store}
            want = {n for n, f in T.VARIANTS if not f.get('poison') or T.has_padding(shape)}
            assert names == want, (shape, store)
            if store == 'x3':
                assert {c.style for c in TN_CASES if c.shape == shape and c.store == store} == {'wideA', 'wideB'}
    for s in T.PHASED:
        for store in ('bf16', 'f16'):
            names = {c.variant for c in TN_CASES if c.shape == s and c.store == store}
            assert names == {n for n in T.PHASED_VARIANTS if n != 'poison' or T.has_padding(s)}
    assert any(c.poison for c in TN_CASES if c.path == 'phased')


def test_tn_group_sets_reach_their_planner_paths():
    """The host-only planner on the grouped sets: 'tiles' gives work items of 1, 2, 3 and 4 K-tiles, 'splits' more than one split
    per tile with the bias limit inside a split, 'shared' sets bit 30 on exactly the two problems that share their gradient."""
    lib = L.load()
    sets = T.group_sets()
    red, f15 = T.host_plan(lib, *sets['splits'])
    assert all(splits > 1 for *_, splits in red) and len(red) == 4
    M, br = sets['splits'][0][0][0][0], sets['splits'][0][0][0][7]
    chunk = -(-(M // 64) // red[0][3]) * 64
    assert br % chunk != 0 and 0 < br < M
    red, f15 = T.host_plan(lib, *sets['tiles'])
    assert all(splits == 1 for *_, splits in red) and not any(f >> 30 & 1 for f in f15)
    assert sorted({s[0] // 64 for s, _ in sets['tiles'][0]}) == [1, 2, 3, 4]
    red, f15 = T.host_plan(lib, *sets['shared'])
    assert [f >> 30 & 1 for f in f15] == [1, 1, 0]
    red, f15 = T.host_plan(lib, *sets['all'])
    assert sum(f >> 30 & 1 for f in f15) == 2


# Five wrong restatements of the emulator's gemm_tn: the case list must catch each of them (on the CPU - no kernel is ever broken
# for this).  Each takes the emulator's arguments.
def _tn_wrong(kind):
    def gemm_tn(self, A, B, G, M, N, K, n_real, k_real, split_src, split_dst, alpha=1.0, gbias=None, bias_rows=0, alpha_dev=None):
        from tests.emu_backend import _dyn
        alpha = alpha * _dyn(alpha_dev)
        gap = split_dst - split_src
        rows_g = n_real
        if kind == 'n_real_ignored':            # pad rows are stored: they land behind the window, in the guard
            room = G.untyped_storage().nbytes() // 4 - G.storage_offset()
            rows_g = min(N, room // k_real)
            G = G.as_strided((rows_g, k_real), (k_real, 1))
        if gbias is not None:
            br = bias_rows if bias_rows > 0 and kind != 'bias_rows_ignored' else M
            rows_b = n_real
            if kind == 'n_real_ignored':
                rows_b = min(N, gbias.untyped_storage().nbytes() // 4 - gbias.storage_offset())
                gbias = gbias.as_strided((rows_b,), (1,))
            gbias[:rows_b] += alpha * (alpha if kind == 'bias_alpha_twice' else 1.0) * A[:br, :rows_b].float().sum(0)
        a, b = A[:M, :N].float(), B[:M, :K].float()
        if kind == 'x3_ahbl_dropped':
            ah, bh = a.bfloat16().float(), b.bfloat16().float()
            full = alpha * ((a - ah).t() @ bh + ah.t() @ bh)
        else:
            full = alpha * (a.t() @ b)
        if kind == 'gap_shifted' and gap > 0:
            split_src, split_dst = split_src + 1, split_dst + 1
        cols = list(range(split_src)) + [k for k in range(split_dst, K) if k - gap < k_real]
        G[:rows_g, :] += full[:rows_g][:, cols]
    return gemm_tn


@pytest.mark.parametrize('kind', ['bias_rows_ignored', 'gap_shifted', 'n_real_ignored', 'bias_alpha_twice', 'x3_ahbl_dropped'])
def test_tn_case_list_catches_wrong_restatement(kind, monkeypatch):
    small = [c for c in TN_CASES if c.shape[0] <= 1000]
    assert len(small) > 100

    def failures():
        out = []
        for c in small:
            try:
                T.launch_and_check(EmuBackend(), T.build(c))
            except AssertionError:
                out.append(c.id)
        return out
    monkeypatch.setattr(EmuBackend, 'gemm_tn', _tn_wrong('correct'))
    assert failures() == [], 'the restatement itself is wrong'
    monkeypatch.setattr(EmuBackend, 'gemm_tn', _tn_wrong(kind))
    caught = failures()
    assert caught, f'no case notices {kind}'
    if kind == 'x3_ahbl_dropped':
        assert all('-x3-wideB-' in i for i in caught)
