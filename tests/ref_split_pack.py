"""Reference packer of the half-split shadows (ASE_F32H3: W * 2^e as half hi / lo parts, [8 hi | 8 lo] per group of 8 elements of
the contiguous dimension), in torch on tests/emu_backend.half_split - the words ase_hip_refresh_shadow and the optimizer launch
must write, pad / gap / uncovered positions included.  Independent of csrc/shadow.h, which both of those launches share.

Order of the split, as csrc/shadow.h split_half documents it: s = clamp(W * 2^e, +-65504), hi = half(s), lo = half(s - hi) - the
saturation comes BEFORE the split, so a saturated element has lo = 0.  half_split(W, e) itself forms lo from the unclamped product
(a saturated element's lo is then the clamped excess, which no product ever met: the weights sit far below 32 at 2^11); the packer
therefore saturates first and splits the result at exponent 0.  Everywhere else the two agree (tests/test_split_pack_ref.py)."""
import torch

from tests.emu_backend import half_split

SENTINEL = 7.0


def split_halves(V, e):
    """V (f32) -> (hi, lo) half tensors of the shadows' split at exponent e (the product with 2^e is exact in f32)."""
    s = (V.float() * 2.0 ** e).clamp(-65504.0, 65504.0)
    hi, lo = half_split(s, 0)
    return hi.half(), lo.half()


def pack_split(V, rows, cols, e, shape, sentinel=SENTINEL):
    """Expected int32 words of a packed buffer [shape[0], shape[1]] (4-byte units, shape[1] in whole groups of 8) that starts full of
    `sentinel`: V[i, j] is element cols[j] of packed row rows[i] - its hi half at half-word (c >> 3) * 16 + (c & 7), lo 8 further on."""
    assert shape[1] % 8 == 0
    buf = torch.full(shape, sentinel, dtype=torch.float32)
    h = buf.view(torch.int16)                                   # [rows, 2 * shape[1]] half-words, little endian
    hi, lo = split_halves(V, e)
    pos = (cols >> 3) * 16 + (cols & 7)
    h[rows[:, None], pos[None, :]] = hi.view(torch.int16)
    h[rows[:, None], pos[None, :] + 8] = lo.view(torch.int16)
    return buf.view(torch.int32)


def shadow_cols(k, split_src, split_dst):
    return torch.tensor([j if j < split_src else j + (split_dst - split_src) for j in range(k)])


def expected_pair(W, e, split_src, split_dst, shape_ws, shape_wts, sentinel=SENTINEL):
    """(W_s, W_s^T) words of W [n, k] with the concat gap split_src -> split_dst."""
    n, k = W.shape
    kd, rn = shadow_cols(k, split_src, split_dst), torch.arange(n)
    return pack_split(W, rn, kd, e, shape_ws, sentinel), pack_split(W.t(), kd, rn, e, shape_wts, sentinel)


def planted(e):
    """Twelve weights the split can get wrong at exponent e, as scaled values s = w * 2^e: beyond +-65504 (saturated, lo = 0), -0.0
    and 0.0, lo a SUBNORMAL half (exact, and a round-to-even tie between two subnormals), the largest half itself, a value that
    rounds up onto it (lo < 0), ties of hi to even in both directions (lo = +-2^-11), hi itself subnormal, and a plain value."""
    s = torch.tensor([70000.0, -70000.0, -0.0, 0.0, 1 + 2.0 ** -20, -(2.0 ** -4 + 1.5 * 2.0 ** -24), 65504.0, 65504.0 - 2.0 ** -6,
                      1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -20, 3.0])
    return s * 2.0 ** -e


def split_case(n, k, e, seed):
    """Finite weights [n, k] whose scaled values sit in half's range (|s| ~ 32), the planted ones at random places.  A case with room
    for them asserts its own coverage."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(n, k, generator=g) * 2.0 ** (5 - e)
    v = planted(e)
    flat = W.view(-1)
    m = min(flat.numel(), v.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:m]] = v[:m]
    assert bool(torch.isfinite(W).all())
    if W.numel() >= 12:
        s = W * 2.0 ** e
        hi, lo = split_halves(W, e)
        bits = W.view(torch.int32)
        assert bool(((s.abs() > 65504) & (hi.abs() == 65504) & (lo == 0)).any()), 'no saturated element'
        assert bool((bits == -2 ** 31).any()), 'no -0.0'
        assert bool((bits == 0).any()), 'no zero'
        assert bool(((lo != 0) & (lo.abs().float() < 2.0 ** -14)).any()), 'no element whose lo part is a subnormal half'
    return W
