"""Every path of the weight-gradient kernels (csrc/gemm_tn.hip), bitwise: ase_hip_gemm_tn on the 128 x 128 kernel in its four
storage modes and on the phased 256 x 256 kernel, ase_hip_gemm_tn_grouped with the workspace (gemm_tn8g + tn_reduce) and without
it (f32 atomics), and the shadow refresh kernels that produce these kernels' B operands - against the exact f64 reference of
tests/ref_gemm_tn.py, NOT the emulator (tests/test_gemm_ref.py runs the same lists through the emulator on the CPU).

The operands are integers (tests/ref_gemm_tn.py states and asserts the conditions), so the split-M partial sums are exact in any
order and G / gbias are compared bit for bit - there is no tolerance in this file, the atomic paths included.  (The refresh kernels
live beside the optimizer in csrc/optim.hip, on the tile routine of csrc/shadow.h; their half-split form is held to the packer of
tests/ref_split_pack.py.)  Every
single-problem case asserts ase_hip_gemm_tn_kernel_id first; G and gbias are windows of longer sentinel buffers that must come
back intact around them; the operands' pitch columns and the rows after M hold NaN, and in the `poison` variants so do the pad
columns the header names (no NaN may reach G or gbias)."""
import pytest
import torch

from ase_amd import lib as L
from tests import ref_gemm_tn as T
from tests import ref_split_pack as S

pytestmark = pytest.mark.gpu

CASES = T.cases()
GROUPS = [('tiles', {}), ('splits', {}), ('shared', {}), ('all', {}), ('shared', dict(alpha=4.0, factor=0.5)), ('tiles', dict(poison=True))]
TOTALS = {'cases': 0, 'elements': 0, 'bad': 0, 'sentinels': 0}


@pytest.fixture(scope='module')
def backends():
    from ase_amd.backend import HipBackend
    plain, atomic = HipBackend(), HipBackend()
    atomic.tn_workspace = False
    yield {'bf16': plain, 'f16': plain, 'f32': plain, 'x3': HipBackend(x3=True), 'atomic': atomic}
    print('\ntn exact totals:', TOTALS)


def _count(n, bad, sent):
    TOTALS['cases'] += 1
    TOTALS['elements'] += n
    TOTALS['bad'] += bad
    TOTALS['sentinels'] += sent


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_kernel_equals_exact_reference(backends, c):
    be = backends[c.store]
    assert T.kernel_id(be.lib, c) == c.kid
    _count(*T.launch_and_check(be, T.build(c), dev=be.device))


@pytest.mark.parametrize('ws', [True, False], ids=['workspace', 'atomics'])
@pytest.mark.parametrize('store', ['bf16', 'f16'])
@pytest.mark.parametrize('name,kw', GROUPS, ids=[n + ''.join('-' + k for k in kw) for n, kw in GROUPS])
def test_grouped_launch_equals_exact_reference(backends, name, kw, store, ws):
    be = backends[store] if ws else backends['atomic']
    assert be.tn_workspace == ws
    g = T.build_group(name, store, **kw)
    plan, n, bad, sent = T.launch_group_and_check(be, g, dev=be.device)
    assert (plan['ws'] is not None) == ws
    _count(n, bad, sent)
    red = plan['red'].view(-1, 4).cpu()
    shared = (plan['problems'].view(-1, 16)[:, 15].cpu() >> 30) & 1
    if name == 'splits':
        assert int(red[:, 3].min()) > 1, 'the plan cuts no tile of the set into splits'
    if name == 'tiles':
        nk = sorted({int(w) & 0xFFFF for w in plan['work'].view(-1, 4)[:, 3].cpu()} - {0})
        assert nk == [1, 2, 3, 4], nk
    if name == 'shared':
        assert shared.tolist() == [1, 1, 0]
    if name == 'all':
        assert int(shared.sum()) == 2 and int(red[:, 3].max()) > 1


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_workspace_path_is_deterministic(backends, dt):
    """The header's "deterministic, no atomics": with non-integer operands, whose partial sums DO depend on the order, two runs of
    the workspace path from the same G0 are bitwise equal (a problem that owns its gradient buffer, several splits per tile)."""
    be = backends['bf16']
    (shape, _), = T.group_sets()['splits'][0]
    M, N, K, nr, kr, ss, sd, br = shape
    g = torch.Generator().manual_seed(77)
    A = (torch.randn(M, N, generator=g) * 0.2).to(dt).to(be.device)
    B = (torch.randn(M, K, generator=g) * 0.2).to(dt).to(be.device)
    G0, b0 = torch.randn(nr, kr, generator=g), torch.randn(nr, generator=g)
    outs = []
    for _ in range(2):
        G, gb = G0.to(be.device), b0.to(be.device)
        plan = be.make_tn_plan([(A, B, G, gb, br, M, N, K, nr, kr, ss, sd, 0.7)], T.group_sets()['splits'][1])
        assert plan['ws'] is not None and int(plan['red'].view(-1, 4)[:, 3].min()) > 1
        be.gemm_tn_grouped(plan)
        outs.append((G.cpu(), gb.cpu()))
    assert not torch.equal(outs[0][0], G0)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------------------- shadow refresh
SHADOW_SENTINEL = 7.0


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _planted(dt):
    """Values the conversion can get wrong: exact round-to-nearest-even ties of both 16-bit types (down to even and up to even),
    +-70000 (half saturates at +-65504), a value that becomes a SUBNORMAL half between two of its neighbours, -0.0."""
    return torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11),
                         70000.0, -70000.0, 2.0 ** -20 * (1 + 2.0 ** -6), -(2.0 ** -20) * (1 + 3 * 2.0 ** -6), 2.0 ** -24 * 1.5, -0.0])


def _convert(W, dt):
    """The torch conversion (round to nearest even; half clamped to +-65504 first, as from_f32<f16_t> does)."""
    return (W.clamp(-65504.0, 65504.0) if dt == torch.float16 else W).to(dt)


def _shadow_case(n, k, dt, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(n, k, generator=g)
    v = _planted(dt)
    flat = W.view(-1)
    m = min(flat.numel(), v.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:m]] = v[:m] if flat.numel() >= v.numel() else v[:1]
    return W


def _expected(W, dt, ss, sd, rows_ws, ldws, rows_wts, ldwts):
    n, k = W.shape
    kd = torch.tensor([j if j < ss else j + (sd - ss) for j in range(k)])
    Ws = torch.full((rows_ws, ldws), SHADOW_SENTINEL, dtype=dt)
    Wts = torch.full((rows_wts, ldwts), SHADOW_SENTINEL, dtype=dt)
    C = _convert(W, dt)
    Ws[:n, kd] = C
    Wts[kd, :n] = C.t()
    return Ws, Wts


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16, torch.float32], ids=['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('n,k,ss,sd', [(1, 1, 1, 1), (33, 65, 65, 65), (48, 53, 37, 64)])
def test_refresh_shadow_equals_torch_conversion(backends, dt, n, k, ss, sd):
    """W_s / W_s^T against the torch conversion, bit for bit (-0.0 included), into sentinel-filled buffers with larger pitches:
    pad columns, gap columns and pad rows come back untouched.  W_s only, W_s^T only, both; refresh_shadow_multi writes the same
    bytes plus the bias copy."""
    be = backends['bf16']
    dev = be.device
    W = _shadow_case(n, k, dt, 100 * n + k)
    kp = k + (sd - ss)
    shape_ws, shape_wts = (n + 3, kp + 11), (kp + 2, n + 13)
    want_ws, want_wts = _expected(W, dt, ss, sd, *shape_ws, *shape_wts)
    if n * k >= 12:
        conv = _bits(_convert(W, dt))
        assert bool((conv == _bits(torch.tensor([-0.0]).to(dt))[0]).any()), 'no -0.0 among the expected values'
        if dt == torch.float16:
            assert bool((_convert(W, dt).abs() == 65504).any()) and bool(((_convert(W, dt).abs() < 6e-5) & (W != 0)).any())
    Wd = W.to(dev)
    for do_ws, do_wts in [(True, False), (False, True), (True, True)]:
        Ws = torch.full(shape_ws, SHADOW_SENTINEL, dtype=dt, device=dev)
        Wts = torch.full(shape_wts, SHADOW_SENTINEL, dtype=dt, device=dev)
        be.refresh_shadow(Wd, Ws if do_ws else None, Wts if do_wts else None, ss, sd)
        sent = torch.full((1,), SHADOW_SENTINEL, dtype=dt)
        for name, got, want, done in (('Ws', Ws.cpu(), want_ws, do_ws), ('Wts', Wts.cpu(), want_wts, do_wts)):
            want = want if done else sent.expand_as(want)
            bad = int((_bits(got) != _bits(want)).sum())
            assert bad == 0, (name, do_ws, do_wts, 'words not bitwise equal', bad, 'of', got.numel())
    # the multi form: the same bytes, and the bias copied into its shadow (the words after n_real untouched)
    b = torch.randn(n).to(dev)
    bs = torch.full((n + 5,), SHADOW_SENTINEL, device=dev)
    Ws = torch.full(shape_ws, SHADOW_SENTINEL, dtype=dt, device=dev)
    Wts = torch.full(shape_wts, SHADOW_SENTINEL, dtype=dt, device=dev)
    desc = torch.tensor([[Wd.data_ptr(), n, k, Ws.data_ptr(), Ws.stride(0), Wts.data_ptr(), Wts.stride(0), ss, sd - ss, b.data_ptr(),
                          bs.data_ptr(), (k + 31) // 32]], dtype=torch.int64, device=dev)
    be.refresh_shadow_multi(desc, [(Wd, Ws, Wts, ss, sd, b, bs)], dt)
    assert torch.equal(_bits(Ws.cpu()), _bits(want_ws)) and torch.equal(_bits(Wts.cpu()), _bits(want_wts))
    want_bs = torch.full((n + 5,), SHADOW_SENTINEL)
    want_bs[:n] = b.cpu()
    assert torch.equal(_bits(bs.cpu()), _bits(want_bs))
    TOTALS['elements'] += 4 * (want_ws.numel() + want_wts.numel())
    TOTALS['cases'] += 1


@pytest.mark.parametrize('e', [0, 11, 24])
@pytest.mark.parametrize('n,k,ss,sd', [(1, 1, 1, 1), (33, 65, 65, 65), (48, 53, 37, 64)])
def test_refresh_shadow_half_split_equals_reference_packer(backends, n, k, ss, sd, e):
    """The packed half-split pair (ASE_F32H3, W * 2^e) against the torch packer of tests/ref_split_pack.py as int32 words: saturated
    elements, -0.0, zero and subnormal lo parts among them (the case asserts it), into sentinel-filled buffers whose leading
    dimensions are larger than needed (whole groups of 8, 32-byte aligned base) - pad rows, pad columns, gap columns and the
    uncovered positions of a partly covered group come back untouched.  W_s only, W_s^T only, both."""
    be = backends['bf16']
    dev = be.device
    W = S.split_case(n, k, e, 100 * n + k + e)
    kp = k + (sd - ss)
    shape_ws, shape_wts = (n + 3, (kp + 7) // 8 * 8 + 8), (kp + 2, (n + 7) // 8 * 8 + 16)
    want_ws, want_wts = S.expected_pair(W, e, ss, sd, shape_ws, shape_wts, SHADOW_SENTINEL)
    Wd = W.to(dev)
    for do_ws, do_wts in [(True, False), (False, True), (True, True)]:
        Ws = torch.full(shape_ws, SHADOW_SENTINEL, device=dev)
        Wts = torch.full(shape_wts, SHADOW_SENTINEL, device=dev)
        assert Ws.data_ptr() % 32 == 0 and Wts.data_ptr() % 32 == 0
        be.refresh_shadow(Wd, Ws if do_ws else None, Wts if do_wts else None, ss, sd, x3_exp=e)
        for name, got, want, done in (('Ws', Ws.cpu(), want_ws, do_ws), ('Wts', Wts.cpu(), want_wts, do_wts)):
            want = want if done else _bits(torch.full_like(got, SHADOW_SENTINEL))
            bad = int((_bits(got) != want).sum())
            assert bad == 0, (name, do_ws, do_wts, 'words not bitwise equal', bad, 'of', got.numel())
    TOTALS['elements'] += 3 * (want_ws.numel() + want_wts.numel())
    TOTALS['cases'] += 1
