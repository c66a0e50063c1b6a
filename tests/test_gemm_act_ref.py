"""The activation and non-finite cases of tests/ref_gemm_act.py on the CPU: every fixture condition holds, the emulator's gemm_nt
meets the same cases and bounds as the kernels (tests/test_gpu_gemm_act.py), and ten single-term wrong restatements each fail a
bound - so a kernel with the same defect would.  The restatement below is plain f32 torch written from the header; with no defect
switched on it passes every case it is used on, which is what makes the failures below the defects' own."""

import pytest
import torch

from ase_amd import lib as L
from tests import ref_gemm as R
from tests import ref_gemm_act as G
from tests.emu_backend import EmuBackend

CASES = G.cases()
SMALL = [c for c in CASES if c.M <= 130]
LARGE = [c for c in CASES if c.M > 130]
NF_SMALL = [c for c in G.nf_cases() if c.M <= 130]


def _emu(store):
    emu = EmuBackend()
    if store == 'h3':
        emu.x3 = 'f16'
    return emu


@pytest.mark.parametrize('c', SMALL + LARGE, ids=[c.id for c in SMALL + LARGE])
def test_emulator_meets_the_reference(c):
    b = G.build(c)                      # asserts the fixture conditions
    assert G.launch_and_check(_emu(c.store), b) >= c.M * c.N


@pytest.mark.parametrize('c', NF_SMALL, ids=[c.id for c in NF_SMALL])
def test_emulator_non_finite(c):
    assert G.nf_run(_emu(c.store), c) > 0


def test_shapes_report_their_kernel_id():
    lib = L.load()
    for M, N, K, code, kid in G.shapes() + G.nf_shapes():
        assert lib.ase_hip_gemm_nt_kernel_id(M, N, K, code) == kid, (M, N, K, code, kid)


def test_case_list():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for store in ('bf16', 'f16', 'f32', 'x3', 'h3'):
        for act in G.ACTS:
            names = {c.variant for c in SMALL if c.store == store and c.act == act}
            assert {'fwd', 'fwd_twin', 'fwd_colsum_n', 'fwd_colsum_n5', 'fwd_a05_rec', 'bwd', 'bwd_a05_rec', 'bwd_stacked'} - names \
                <= ({'fwd_twin'} if act == L.ACT_TANH else set()), (store, act, names)
            assert ('fwd_out_f32' in names) == (store in ('bf16', 'f16'))
        assert {c.act for c in LARGE if c.store == store} == {L.ACT_SILU, L.ACT_TANH}
    # tanh's bit twin needs N % 32 == 0: the large shapes carry it
    assert sum(c.twin and c.act == L.ACT_TANH for c in LARGE) >= 8
    nf = G.nf_cases()
    assert {c.act for c in nf} == set(G.NF_ACTS + G.NF_OTHER) and {c.epilogue for c in nf} == {'rows', 'slab'}


@pytest.mark.parametrize('c', [c for c in SMALL if c.variant in ('fwd_twin', 'fwd', 'bwd') and c.M == 70],
                         ids=lambda c: c.id)
def test_fixture_conditions(c):
    """What build() asserts, once more in the open: every inner band >= 64 elements, >= 10 % negative z, 16-bit outputs that the
    conversion changes, and the planted values where the module says they are."""
    b = G.build(c)
    assert all(int(b.band_counts[i]) >= 64 for i in range(1, 6)), b.band_counts.tolist()
    assert int((b.band == -1).sum()) >= len(G.PLANTED)
    if not c.back:
        z = b.arg
        assert float((z < 0).float().mean()) >= 0.10
        planted = set(z[b.planted].tolist())
        assert planted == {float(torch.tensor(v, dtype=torch.float32)) for v in G.PLANTED}
        cols = set(b.planted.any(0).nonzero().flatten().tolist())
        assert {0, 31, 32, c.N - 1} <= cols
    if c.out_dtype != torch.float32:
        assert b.rounded >= 0.05


def test_f16_plant_fixture():
    c = [c for c in SMALL if c.f16_plant][0]
    b = G.build(c)
    assert float(b.arg.max()) >= G.F16_PLANT and float(b.ref64.max()) == 1.0
    assert float(b.twin.float().max()) == R.F16_MAX and bool(torch.isfinite(b.twin.float()).all())


# ------------------------------------------------------------------------------------------------------- wrong restatements
_LAM, _AL = 1.0507009873554805, 1.6732632423543772


def _sig(z):
    return 1.0 / (1.0 + torch.exp(-z))


def _fwd(act, z, wrong):
    if act == L.ACT_RELU:
        return torch.fmax(z, torch.zeros(())) if wrong == 'relu_drops_nan' else torch.where(z < 0, torch.zeros(()), z)
    if act == L.ACT_TANH:
        return torch.tanh(z)
    if act == L.ACT_SILU:
        return z * _sig(z)
    if act == L.ACT_ELU:
        return torch.where(z > 0, z, (torch.exp(z) - 1.0) if wrong == 'elu_exp' else torch.expm1(z))
    if act == L.ACT_GELU:
        if wrong == 'gelu_tanh':
            return 0.5 * z * (1.0 + torch.tanh(0.7978845608028654 * (z + 0.044715 * z * z * z)))
        return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    if act == L.ACT_SIGMOID:
        return _sig(z)
    if act == L.ACT_SELU:
        lam, al = (_AL, _LAM) if wrong == 'selu_swapped' else (_LAM, _AL)
        return lam * torch.where(z > 0, z, al * torch.expm1(z))
    if act == L.ACT_SOFTPLUS:
        return torch.log1p(torch.exp(z)) if wrong == 'softplus_no_threshold' else torch.where(z > 20, z, torch.log1p(torch.exp(z)))
    return z


def _grad(act, z, wrong):
    s = _sig(z)
    if act == L.ACT_SILU:
        return s if wrong == 'silu_grad_short' else s * (1.0 + z * (1.0 - s))
    if act == L.ACT_ELU:
        return torch.where(z > 0, torch.ones(()), torch.exp(z))
    if act == L.ACT_GELU:
        return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z)
    if act == L.ACT_SIGMOID:
        return s * (1.0 + s) if wrong == 'sigmoid_grad_sign' else s * (1.0 - s)
    if act == L.ACT_SELU:
        return _LAM * torch.where(z > 0, torch.ones(()), _AL * torch.exp(z))
    if act == L.ACT_SOFTPLUS:
        return torch.where(z > 20, torch.ones(()), s)
    raise AssertionError(act)


class Restated:
    """gemm_nt in plain f32 torch from the header, with at most one term wrong."""
    def __init__(self, wrong=None):
        self.wrong = wrong

    def gemm_nt(self, A, B, Cm, M, N, K, bias=None, aux=None, aux_mode=L.AUX_NONE, colsum=None, colsum_n=0, act=L.ACT_NONE,
                alpha=1.0, aux_split=0, aux_delta=0, mask_out=None, alpha_dev=None):
        w = self.wrong
        a = alpha * (1.0 if alpha_dev is None else float(alpha_dev[0]))
        p = a * (A[:M, :K].float() @ B[:N, :K].float().t())
        z = p if bias is None else p + bias[:N]
        v = _fwd(act, z, w)
        if aux is not None:
            rows = torch.arange(M)
            if aux_split > 0:
                rows = torch.where(rows >= aux_split, rows - aux_delta, rows)
            x = aux[rows][:, :N].float()
            if aux_mode == L.AUX_TANH_GRAD:
                v = v * (1.0 - x * x)
            else:
                assert (aux_mode & 0xFF) == L.AUX_PREACT
                v = v * _grad(aux_mode >> 8, _fwd(aux_mode >> 8, x, None) if w == 'preact_at_output' else x, w)

        def store(t, dt):
            return t.clamp(-R.F16_MAX, R.F16_MAX).to(dt) if dt == torch.float16 else t.to(dt)
        out = store(v, Cm.dtype)
        Cm[:M, :N] = out
        stored = [out]
        if mask_out is not None and act >= L.ACT_SILU:
            t = store(v if w == 'twin_holds_output' else (p if w == 'twin_before_bias' else z), mask_out.dtype)
            mask_out[:M, :N] = t
            stored.append(t)
        elif mask_out is not None:
            mask_out[:M, :N // 32] = R.pack_bits(out.float() > 0)
        if colsum is not None and colsum_n > 0:
            colsum[:colsum_n] += out.float().sum(0)[:colsum_n]
        if alpha_dev is not None:
            for t in stored:
                f = t.float()
                if bool((~torch.isfinite(f)).any()) or (t.dtype == torch.float16 and bool((f.abs() >= R.F16_MAX).any())):
                    alpha_dev[1] += 1.0


def _case(store, act, variant, M=70):
    return [c for c in SMALL if c.store == store and c.act == act and c.variant == variant and c.M == M][0]


# (defect, the case that must catch it)
WRONG = [
    ('gelu_tanh', ('f32', L.ACT_GELU, 'fwd')),
    ('selu_swapped', ('bf16', L.ACT_SELU, 'fwd')),
    ('elu_exp', ('f32', L.ACT_ELU, 'fwd')),
    ('softplus_no_threshold', ('bf16', L.ACT_SOFTPLUS, 'fwd')),
    ('silu_grad_short', ('bf16', L.ACT_SILU, 'bwd')),
    ('sigmoid_grad_sign', ('bf16', L.ACT_SIGMOID, 'bwd')),
    ('preact_at_output', ('bf16', L.ACT_SILU, 'bwd')),
    ('twin_holds_output', ('bf16', L.ACT_SILU, 'fwd_twin')),
    ('twin_before_bias', ('f16', L.ACT_ELU, 'fwd_twin')),
]


@pytest.mark.parametrize('wrong,key', WRONG, ids=[w for w, _ in WRONG])
def test_wrong_restatement_fails_a_bound(wrong, key):
    b = G.build(_case(*key))
    G.launch_and_check(Restated(), b)                  # the restatement itself is inside every bound ...
    with pytest.raises(AssertionError):                # ... and one wrong term is not
        G.launch_and_check(Restated(wrong), b)


def test_restatement_meets_the_reference():
    """The plain restatement on every small f32 / bf16 / f16 case of the first shape: the defects above fail because of their term."""
    n = 0
    for c in SMALL:
        if c.M == 70 and c.store in ('f32', 'bf16', 'f16'):
            n += G.launch_and_check(Restated(), G.build(c))
    assert n > 0


@pytest.mark.parametrize('store', ['bf16', 'f16', 'f32'])
def test_relu_that_drops_nan_fails(store):
    c = [c for c in NF_SMALL if c.act == L.ACT_RELU and c.store == store and not c.out_f32][0]
    assert G.nf_run(Restated(), c) > 0
    with pytest.raises(AssertionError):
        G.nf_run(Restated('relu_drops_nan'), c)
