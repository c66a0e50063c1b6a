"""Edge-case golden vectors of the environment-side tensor functions, a sibling of make_golden_env.py:
the same unmodified jit functions of the reference, run on the CPU in f32 and - on the same inputs cast up - in f64, on rows
BUILT FROM THE DECISION VARIABLE: ties at the f32 thresholds and their two neighbours, the whole truth table of the reset,
the deciding body at every place of the body masks, body counts 1 / 2 / 5 / 24 / 64, environment counts round the 64-lane and
16-environment block edges, exactly representable reward rows, and NaN / infinity in one operand at a time.
TEST INFRASTRUCTURE ONLY (needs the reference tree).

    python scripts/make_golden_env_edges.py      # writes tests/golden/env_edges.pt (tensors and plain lists only)

The file is a dict of named GROUPS.  Every group carries its own n, B, body id lists and max_episode_length, the inputs the
reference consumed, both runs' outputs, the f32 run's masks (make_golden_env.masks), the planted rows with what each plants,
the tie rows (expectation: the f32 run, f64 may take the other branch) and e_ref per float output = max |f32 - f64| of the
reference over the group's finite, non-tie elements and over a seeded 4096-row draw of the group's distribution.

Asserted here and again by tests/test_env_edges_emu.py:
  * every mask of a group with >= 15 rows is taken and not taken by >= 4 rows (a one-row group cannot be asked that)
  * every non-planted row keeps the 1e-3 margin of make_golden_env.py
  * the f32 and the f64 run agree on every mask outside the listed tie rows
  * a group whose allowance 2 e_ref + 2^-23 max |ref| + 1e-7 exceeds 1e-4 is flagged ``wide`` (the ill-conditioned tilts and
    the rows of magnitude 1e3, whose 2^-23 max |ref| alone is 1.2e-4); the wide groups hold <= 5 % of the float elements
"""
import math
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_env as E                                                   # noqa: E402
from make_golden_env import cast, decisions, masks, root_states, run         # noqa: E402,F401

ROOT = E.ROOT
H, HS = E.H, E.HS
MARGIN = E.MARGIN
NAN, INF = float('nan'), float('inf')
DT_EXACT = 1.0 / 32.0
WIDE_BAR, WIDE_SHARE = 1e-4, 0.05
HEADING_MARGIN = 0.05
RESET_MASKS = ['fall_contact', 'fall_height', 'has_fallen', 'tar_has_contact', 'nonstrike_contact', 'tar_fail', 'progress>1',
               'progress>=max-1', 'terminated_plain', 'reset_plain', 'terminated_strike', 'reset_strike']
TASK_MASKS = ['heading_speed<=0', 'location_speed<=0', 'location_pos_err<0.5', 'strike_speed<=0', 'strike_rot_err<0.2']
TASK_FUNCS = E.FLOAT_FUNCS[1:]
FLAGS = [(True, True), (True, False), (False, True), (False, False)]
f32 = np.float32


class patched:
    """make_golden_env's functions read its module constants when they run: set them for one group."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: getattr(E, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(E, k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            setattr(E, k, v)


def nxt(x, up=True):
    return float(np.nextafter(f32(x), f32(INF if up else -INF)))


def three(x):
    """The f32 value of x and its two neighbours."""
    return [nxt(x, False), float(f32(x)), nxt(x, True)]


def max_err(a32, a64, skip=None):
    d = (a32.double() - a64).abs()
    d[~torch.isfinite(d)] = 0
    if skip:
        d[skip] = 0
    return float(d.max()) if d.numel() else 0.0


def max_ref(a64, skip=None):
    a = a64.abs().clone()
    a[~torch.isfinite(a)] = 0
    if skip:
        a[skip] = 0
    return float(a.max()) if a.numel() else 0.0


# =================================================================================================== reset groups
def heights_of(B):
    return torch.tensor([0.3 if b % 4 == 3 else 0.15 for b in range(B)])


def quiet(n, B, g):
    """Nothing fires: forces within 0.05, every body at least 0.6 high, a silent target, progress 10."""
    u = lambda *s: torch.rand(*s, generator=g)
    pos = torch.randn(n, B, 3, generator=g)
    pos[..., 2] = 0.6 + 0.8 * u(n, B)
    return {'contact_forces': (u(n, B, 3) - 0.5) * 0.1, 'body_pos': pos, 'tar_contact_forces': u(n, 3) - 0.5,
            'termination_heights': heights_of(B), 'progress_buf': torch.full((n,), 10, dtype=torch.long)}


def body_sets(B, C):
    keep = [b for b in range(B) if b not in C['contact']]
    return keep, [b for b in keep if b not in C['strike']]


def progress_of(state, M):
    """(progress > 1, progress >= max - 1) -> a progress value."""
    last = int(math.ceil(M - 1))
    return {(False, False): 1 if M > 2.5 else 0, (True, False): 10, (True, True): last if last > 1 else 5, (False, True): 1}[state]


def plant_combo(I, r, C, fc, nsc, fh, thc, pstate, rng, split=False, body=None):
    """One row of the truth table over a quiet state: one deciding body per condition."""
    B = I['body_pos'].shape[1]
    keep, nonstrike = body_sets(B, C)
    what = []
    bc = bh = None
    if fc:
        bc = body if body is not None else rng.choice(nonstrike if nsc else keep)
        val = 3.0 if nsc else (0.5 if bc in nonstrike else rng.choice([0.5, 3.0]))
        comp = rng.randrange(3)
        I['contact_forces'][r, bc, comp] = val * rng.choice([-1.0, 1.0])
        what.append(f'contact {val} on body {bc} component {comp}')
    if fh:
        others = [b for b in keep if b != bc]
        bh = body if body is not None and not split else rng.choice(others if (split and others) else keep)
        I['body_pos'][r, bh, 2] = float(I['termination_heights'][bh]) - 0.05
        what.append(f'body {bh} below its height')
    if thc:
        k = rng.randrange(2)
        I['tar_contact_forces'][r, k] = 2.0 * rng.choice([-1.0, 1.0])
        what.append(f'target contact component {k}')
    I['progress_buf'][r] = progress_of(pstate, C['max_len'])
    return '; '.join(what) + f'; progress {int(I["progress_buf"][r])}', bc, bh


def combos(pstates):
    return [(fc, nsc, fh, thc, p) for fc, nsc in ((False, False), (True, False), (True, True)) for fh in (False, True)
            for thc in (False, True) for p in pstates]


def run_reset(I, C, dtype):
    J = cast(I, dtype)
    n = J['body_pos'].shape[0]
    reset_buf = torch.ones(n, dtype=torch.long)
    cb, sb = torch.tensor(C['contact'], dtype=torch.long), torch.tensor(C['strike'], dtype=torch.long)
    O = {}
    for early in (True, False):
        O[('reset', 'plain', early)] = H.compute_humanoid_reset(reset_buf, J['progress_buf'], J['contact_forces'], cb, J['body_pos'],
                                                                C['max_len'], early, J['termination_heights'])
        O[('reset', 'strike', early)] = HS.compute_humanoid_reset(reset_buf, J['progress_buf'], J['contact_forces'], cb, J['body_pos'],
                                                                  J['tar_contact_forces'], sb, C['max_len'], early,
                                                                  J['termination_heights'])
    return O


def reset_masks(I, C, O, dtype):
    """make_golden_env.masks on a reset group: the task operands it also reads are zeros."""
    n, B = I['body_pos'].shape[:2]
    J = dict(I)
    z = lambda *s: torch.zeros(*s)
    J.update(prev_root_pos=z(n, 3), tar_dir=z(n, 2), tar_pos_loc=z(n, 2), tar_states=z(n, 13))
    with patched(B=B, CONTACT_BODY_IDS=C['contact'], STRIKE_BODY_IDS=C['strike'], MAX_EPISODE_LENGTH=C['max_len']):
        M = masks(J, O, dtype)
    return {k: M[k] for k in RESET_MASKS}


def reset_margin_ok(I, rows):
    """The 1e-3 margin of the float decision quantities on the given rows."""
    c = I['contact_forces'][rows].abs().double()
    ok = ((c - 0.1).abs() >= MARGIN).all() and ((c - 1.0).abs() >= MARGIN).all()
    ok = ok and ((I['body_pos'][rows][..., 2].double() - I['termination_heights'].double()).abs() >= MARGIN).all()
    return bool(ok and ((I['tar_contact_forces'][rows][:, :2].abs().double() - 1.0).abs() >= MARGIN).all())


RESET_KEYS = [('reset', form, early) for form in ('plain', 'strike') for early in (True, False)]


def pack_reset(O):
    """{('reset', form, early): (reset, terminated)} as one int8 tensor [4, 2, n] in the order of RESET_KEYS."""
    return torch.stack([torch.stack(list(O[k])) for k in RESET_KEYS]).to(torch.int8)


def pack_masks(M, names):
    return torch.stack([M[k] for k in names])


def counts_ok(M):
    return all(min(int(v.sum()), int((~v).sum())) >= 4 for v in M.values())


def reset_group(n, B, C, planter=None, seed=0, truth=None, note=''):
    """`planter(I, rng)` -> [(row, what)] plants the first rows; the rest is a seeded mix of the truth table, re-drawn until every
    mask is taken and not taken by >= 4 rows.  `truth`: the listed combinations in order instead of the mix."""
    pstates = [(False, False), (True, False), (True, False), (True, True)]
    for attempt in range(400):
        g = torch.Generator().manual_seed(7000 + 31 * seed + attempt)
        rng = random.Random(9000 + 31 * seed + attempt)
        I = quiet(n, B, g)
        planted = planter(I, rng) if planter else []
        split_rows = 0
        taken = {r for r, _ in planted}
        free = [r for r in range(n) if r not in taken]
        if truth is not None:
            assert len(truth) == len(free)
            for k, (r, cmb) in enumerate(zip(free, truth)):
                what, bc, bh = plant_combo(I, r, C, *cmb, rng, split=(k % 2 == 0))
                planted.append((r, 'truth table: ' + what))
                split_rows += int(bc is not None and bh is not None and bc != bh)
            free = []
        else:
            _, nonstrike = body_sets(B, C)
            for r in free:
                fc, nsc = rng.choice([(False, False), (True, False), (True, True), (True, True)])
                plant_combo(I, r, C, fc, nsc and bool(nonstrike), rng.random() < 0.55, rng.random() < 0.5, rng.choice(pstates), rng,
                            split=rng.random() < 0.5)
        O32, O64 = run_reset(I, C, torch.float32), run_reset(I, C, torch.float64)
        M32, M64 = reset_masks(I, C, O32, torch.float32), reset_masks(I, C, O64, torch.float64)
        if n < 15 or counts_ok(M32):
            break
    else:
        raise AssertionError('no seed gives every mask both ways 4 times')
    ties = sorted({r for r, w in planted if w.startswith('tie')})
    rest = [r for r in range(n) if r not in ties]
    for k in M32:
        assert torch.equal(M32[k][rest], M64[k][rest]), f'the f32 and the f64 run disagree on {k} outside the tie rows'
    assert reset_margin_ok(I, free), 'a non-planted row is within the margin'
    return {'kind': 'reset', 'n': n, 'B': B, 'contact_body_ids': list(C['contact']), 'strike_body_ids': list(C['strike']),
            'max_episode_length': float(C['max_len']), 'inputs': I, 'f32': pack_reset(O32), 'f64': pack_reset(O64),
            'masks': pack_masks(M32, RESET_MASKS), 'planted': planted,
            'tie_rows': ties, 'free_rows': free, 'e_ref': {}, 'max_ref': {}, 'wide': False, 'note': note,
            'split_rows': split_rows, 'branch_counts': {k: [int(v.sum()), int((~v).sum())] for k, v in M32.items()}}


STD = {'contact': [11, 14], 'strike': [4, 5, 6, 8, 9, 10], 'max_len': 300.0}


def plant_ties(I, rng):
    """B = 17, the standard id lists.  Body 2 is neither a contact nor a strike body (height 0.15), body 3 has height 0.3."""
    P = []
    r = 0

    def row(what):
        nonlocal r
        P.append((r, what))
        r += 1
        return r - 1
    low = lambda k, b: I['body_pos'].__setitem__((k, b, 2), float(I['termination_heights'][b]) - 0.05)
    for thr in (0.1, 1.0):
        for comp in range(3):
            for sign in (-1.0, 1.0):
                for j, v in enumerate(three(thr)):
                    k = row(f'tie: contact component {comp} of body 2 = {sign:+.0f} * ({thr} {("- ulp", "", "+ ulp")[j]})')
                    I['contact_forces'][k, 2, comp] = sign * v
                    if thr == 0.1:
                        low(k, 7)                                        # the height half is pending
                    else:
                        I['tar_contact_forces'][k, 0] = 2.0              # the target half is pending
    for comp in range(2):
        for sign in (-1.0, 1.0):
            for j, v in enumerate(three(1.0)):
                k = row(f'tie: target contact component {comp} = {sign:+.0f} * (1 {("- ulp", "", "+ ulp")[j]})')
                I['tar_contact_forces'][k, comp] = sign * v
                I['contact_forces'][k, 2, 1] = 3.0
    for sign in (-1.0, 1.0):
        k = row('target contact z alone is loud: it must not count')
        I['tar_contact_forces'][k, 2] = sign * 50.0
        I['contact_forces'][k, 2, 1] = 3.0
    for b in (2, 3):
        for j, v in enumerate(three(float(I['termination_heights'][b]))):
            k = row(f'tie: height of body {b} = its termination height {("- ulp", "", "+ ulp")[j]}')
            I['body_pos'][k, b, 2] = v
            I['contact_forces'][k, 12, 0] = 0.5
    for p in (0, 1, 2, 298, 299, 300):
        k = row(f'progress {p} with a fall pending')
        I['contact_forces'][k, 2, 2] = -0.5
        low(k, 3)
        I['progress_buf'][k] = p
    for b in (0, 16, 10, 12, 13, 15):
        k = row(f'the deciding body is {b}: force and height')
        I['contact_forces'][k, b, rng.randrange(3)] = 3.0
        low(k, b)
        I['tar_contact_forces'][k, 1] = -2.0
    for b in (11, 14):
        k = row(f'contact body {b} alone: its force and its height are ignored')
        I['contact_forces'][k, b] = torch.tensor([50.0, -50.0, 50.0])
        low(k, b)
        I['tar_contact_forces'][k, 0] = 2.0
    for b in (11, 14):
        k = row(f'contact body {b} below its height with the contact half pending from body 2: its height is ignored')
        low(k, b)
        I['contact_forces'][k, 2, 0] = 0.5
        k = row(f'contact body {b} loud with the height half pending from body 3: its force is ignored')
        I['contact_forces'][k, b] = torch.tensor([-50.0, 50.0, -50.0])
        low(k, 3)
    k = row('strike body 4 alone, loud, target contact pending: fall_contact but not nonstrike_contact')
    I['contact_forces'][k, 4, 0] = 3.0
    I['tar_contact_forces'][k, 0] = 2.0
    k = row('strike body 10 alone, loud, its own height pending: it counts for fall_contact')
    I['contact_forces'][k, 10, 2] = -3.0
    low(k, 10)
    for bad in (NAN, INF, -INF):
        for loud in (True, False):
            k = row(f'contact triple of body 2 with {bad} in x and {"a loud" if loud else "a quiet"} y, height pending')
            I['contact_forces'][k, 2, 0] = bad
            I['contact_forces'][k, 2, 1] = 0.5 if loud else 0.01
            low(k, 7)
    k = row('NaN height of body 2 with a contact pending: NaN < h is false')
    I['body_pos'][k, 2, 2] = NAN
    I['contact_forces'][k, 12, 0] = 0.5
    k = row('NaN in the force of contact body 11: masked')
    I['contact_forces'][k, 11, 1] = NAN
    return P


def plant_progress_ties(I, rng):
    P = []
    for k, p in enumerate((297, 298, 299, 300, 298, 299, 300, 301)):
        P.append((k, f'progress {p} against max_episode_length 300.5' + (' with a fall pending' if k < 4 else '')))
        I['progress_buf'][k] = p
        if k < 4:
            I['contact_forces'][k, 2, 2] = -0.5
            I['body_pos'][k, 3, 2] = 0.2
    return P


def plant_body(body, rows=4):
    def f(I, rng):
        P = []
        for k in range(rows):
            P.append((k, f'the deciding body is {body}: loud force, below its height' + ('' if k % 2 else ', target contact')))
            I['contact_forces'][k, body, k % 3] = 3.0 * (-1.0) ** k
            I['body_pos'][k, body, 2] = float(I['termination_heights'][body]) - 0.05
            if k % 2 == 0:
                I['tar_contact_forces'][k, k // 2 % 2] = 2.0
        return P
    return f


def plant_edges(body):
    """The last row of every 64-lane and 16-environment block, and the first of the next, terminate through `body`."""
    def f(I, rng):
        n = I['body_pos'].shape[0]
        P = []
        for r in sorted({0, 15, 16, 63, 64, 127, 128, n - 1}):
            if r < n:
                P.append((r, f'row {r} at a block edge terminates through body {body}'))
                I['contact_forces'][r, body, r % 3] = 3.0
                I['body_pos'][r, body, 2] = float(I['termination_heights'][body]) - 0.05
        return P
    return f


def reset_groups():
    G = {}
    short = dict(STD, max_len=2.0)
    G['reset_truth'] = reset_group(36, 17, STD, truth=combos([(False, False), (True, False), (True, True)]), seed=1,
                                   note='36 of the 48 feasible combinations: progress > 1 false / true, >= max - 1 with > 1')
    G['reset_truth_short'] = reset_group(36, 17, short, truth=combos([(False, True), (False, False), (True, True)]), seed=2,
                                         note='max_episode_length 2: the 12 combinations with progress >= max - 1 but not > 1')
    G['reset_ties'] = reset_group(136, 17, STD, plant_ties, seed=3)
    G['reset_ties_300_5'] = reset_group(32, 17, dict(STD, max_len=300.5), plant_progress_ties, seed=4)
    G['reset_b1'] = reset_group(1, 1, {'contact': [], 'strike': [], 'max_len': 300.0}, plant_body(0, 1), seed=5, note='no id lists')
    G['reset_b1_n17'] = reset_group(17, 1, {'contact': [], 'strike': [], 'max_len': 300.0}, plant_body(0, 2), seed=6, note='no id lists')
    G['reset_b2_n130'] = reset_group(130, 2, {'contact': [], 'strike': [1], 'max_len': 300.0}, plant_edges(1), seed=7)
    c24 = {'contact': [11, 14], 'strike': [4, 5, 6, 8, 9, 10, 23], 'max_len': 300.0}
    G['reset_b24_n64'] = reset_group(64, 24, c24, plant_edges(22), seed=8)
    G['reset_b24_n15'] = reset_group(15, 24, c24, plant_body(23, 2), seed=9)
    G['reset_b2_n33'] = reset_group(33, 2, {'contact': [1], 'strike': [], 'max_len': 300.0}, plant_edges(0), seed=10)
    G['reset_b17_n63'] = reset_group(63, 17, STD, plant_edges(16), seed=11)
    G['reset_b17_n16'] = reset_group(16, 17, STD, plant_body(15, 2), seed=12)
    c64 = {'contact': [62, 63], 'strike': [4, 5, 6, 8, 9, 10], 'max_len': 300.0}
    G['reset_b64_n65'] = reset_group(65, 64, c64, plant_edges(61), seed=13, note='contact ids {62, 63}, the deciding body 61')
    s63 = [4, 5, 32, 63]
    G['reset_b64_63_contact'] = reset_group(16, 64, {'contact': [63], 'strike': [4, 5, 32], 'max_len': 300.0}, plant_body(63), seed=15)
    G['reset_b64_63_strike'] = reset_group(16, 64, {'contact': [11], 'strike': s63, 'max_len': 300.0}, plant_body(63), seed=16)
    G['reset_b64_63_neither'] = reset_group(16, 64, {'contact': [11], 'strike': [4, 5, 32], 'max_len': 300.0}, plant_body(63), seed=17)
    # what the planted rows must show, in the reference's own outputs
    keys = ('fall_contact', 'nonstrike_contact', 'fall_height', 'tar_has_contact', 'progress>1', 'progress>=max-1')
    seen = {tuple(bool(G[name]['masks'][RESET_MASKS.index(k)][r]) for k in keys) for name in ('reset_truth', 'reset_truth_short') for r in range(36)}
    assert len(seen) == 48, len(seen)
    assert G['reset_truth']['split_rows'] >= 8, G['reset_truth']['split_rows']
    mk = lambda name, k: G[name]['masks'][RESET_MASKS.index(k)]
    for name, want in (('reset_b64_63_contact', (0, 0)), ('reset_b64_63_strike', (1, 1)), ('reset_b64_63_neither', (1, 1))):
        for form, w in zip(('plain', 'strike'), want):
            assert int(G[name]['f32'][RESET_KEYS.index(('reset', form, True)), 1, 0]) == w, (name, form)
    assert int(mk('reset_b64_63_strike', 'nonstrike_contact')[0]) == 0 and int(mk('reset_b64_63_neither', 'tar_fail')[0]) == 1
    return G


# =================================================================================================== task group
def exact_rows(I, r0):
    """Rows whose decision variable is exactly representable: identity root rotation, dyadic positions, dt = 1/32."""
    P = []
    ident = torch.tensor([0.0, 0.0, 0.0, 1.0])

    def base(k, what, root=(0.0, 0.0), prev=(0.0, 0.0), tar=(2.0, 0.0), tdir=(1.0, 0.0), face=(1.0, 0.0), speed=1.0):
        I['body_rot'][k, 0] = ident
        I['body_pos'][k, 0, :2] = torch.tensor(root)
        I['prev_root_pos'][k, :2] = torch.tensor(prev)
        I['tar_pos_loc'][k] = torch.tensor(tar)
        I['tar_states'][k, :2] = torch.tensor(tar)
        I['tar_dir'][k] = torch.tensor(tdir)
        I['tar_face_dir'][k] = torch.tensor(face)
        I['tar_speed'][k] = speed
        P.append((k, what))
    s = 2.0 ** -10
    rows = [('the root exactly where it was: speed +0', {}),
            ('the root moved +2^-10 along the target direction', dict(root=(s, 0.0))),
            ('the root moved -2^-10 against the target direction', dict(root=(-s, 0.0))),
            ('the root moved +2^-10 along y, the target direction (0, 1)', dict(root=(0.0, s), tar=(0.0, 2.0), tdir=(0.0, 1.0))),
            ('the root moved -2^-10 along y, the target direction (0, 1)', dict(root=(0.0, -s), tar=(0.0, 2.0), tdir=(0.0, 1.0))),
            ('pos_err exactly 0.5', dict(tar=(0.5, 0.5), prev=(-s, -s))),
            ('pos_err 0.5 - 2^-25', dict(tar=(0.5, 0.5 - 2.0 ** -25), prev=(-s, -s))),
            ('pos_err 0.5 + 2^-24', dict(tar=(0.5, 0.5 + 2.0 ** -24), prev=(-s, -s))),
            ('the target on the root: normalize(0) = 0', dict(root=(0.25, -0.5), prev=(0.25 - s, -0.5), tar=(0.25, -0.5))),
            ('speed 2 above the target speed 1: the clamped error is exactly 0', dict(root=(2.0 ** -4, 0.0), speed=1.0)),
            ('speed exactly the target speed 1', dict(root=(2.0 ** -5, 0.0), speed=1.0)),
            ('facing dot product -1', dict(root=(s, 0.0), tar=(-2.0, 0.0), face=(-1.0, 0.0), prev=(2 * s, 0.0), tdir=(-1.0, 0.0))),
            ('facing dot product exactly 0', dict(root=(0.0, s), tar=(0.0, 2.0), face=(0.0, 1.0), tdir=(0.0, 1.0))),
            ('facing dot product exactly 0, from below', dict(root=(0.0, -s), prev=(0.0, 0.0), tar=(0.0, -2.0), face=(0.0, -1.0), tdir=(0.0, -1.0)))]
    for j, (what, kw) in enumerate(rows):
        base(r0 + j, 'exact: ' + what, **kw)
    return P


def strike_ties(count=4):
    """Target quaternions (0, 0, z, w) whose f32 value of (2 w^2 - 1) + 2 z z is float32(0.2) and its two neighbours (only +, -,
    * reach the quantity).  -> {0: [...], -1: [...], +1: [...]} of (z, w) pairs."""
    g = torch.Generator().manual_seed(515)
    w = (0.3 + 0.45 * torch.rand(200000, generator=g)).float()
    z = torch.sqrt((1.2 - 2.0 * w.double() ** 2) / 2.0).float()
    want = {-1: nxt(0.2, False), 0: float(f32(0.2)), 1: nxt(0.2, True)}
    found = {k: [] for k in want}
    for _ in range(5):
        v = (2.0 * w ** 2 - 1.0) + 2.0 * z * z
        for k, t in want.items():
            for i in torch.nonzero(v == t).view(-1)[:count].tolist():
                if len(found[k]) < count:
                    found[k].append((float(z[i]), float(w[i])))
        z = torch.nextafter(z, torch.full_like(z, 2.0))
    return found


NONFINITE = [('NaN root position x', 'body_pos', (0, 0), NAN), ('NaN root position z', 'body_pos', (0, 2), NAN),
             ('NaN previous root position x', 'prev_root_pos', (0,), NAN), ('NaN previous root position y', 'prev_root_pos', (1,), NAN),
             ('NaN root rotation y', 'body_rot', (0, 1), NAN), ('NaN root rotation w', 'body_rot', (0, 3), NAN),
             ('NaN tar_dir x', 'tar_dir', (0,), NAN), ('NaN tar_face_dir y', 'tar_face_dir', (1,), NAN), ('NaN tar_speed', 'tar_speed', (), NAN),
             ('NaN location target x', 'tar_pos_loc', (0,), NAN), ('NaN reach target z', 'tar_pos_reach', (2,), NAN),
             ('NaN target position x', 'tar_states', (0,), NAN), ('NaN target position z', 'tar_states', (2,), NAN),
             ('NaN target rotation z', 'tar_states', (5,), NAN), ('NaN target rotation w', 'tar_states', (6,), NAN),
             ('NaN target velocity x', 'tar_states', (7,), NAN), ('NaN target angular velocity y', 'tar_states', (11,), NAN),
             ('NaN reach body y', 'body_pos', (E.REACH_BODY_ID, 1), NAN),
             ('+inf root position x', 'body_pos', (0, 0), INF), ('-inf root position y', 'body_pos', (0, 1), -INF),
             ('+inf target position x', 'tar_states', (0,), INF), ('-inf location target y', 'tar_pos_loc', (1,), -INF),
             ('+inf reach target x', 'tar_pos_reach', (0,), INF), ('-inf target position y', 'tar_states', (1,), -INF)]


def same_pattern(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isposinf(a), torch.isposinf(b)) and \
        torch.equal(torch.isneginf(a), torch.isneginf(b))


def task_group():
    with patched(DT=DT_EXACT):
        g = torch.Generator().manual_seed(20263)
        ties = strike_ties()
        n_tie = sum(len(v) for v in ties.values())
        n_gen, n_exact = 64, 14
        n = n_gen + n_exact + n_tie + len(NONFINITE)
        I = E.draw_with_margins(n, g, False)
        planted = exact_rows(I, n_gen)
        r = n_gen + n_exact
        tie_rows = []
        for k in (-1, 0, 1):
            for z, w in ties[k]:
                I['tar_states'][r, 3:7] = torch.tensor([0.0, 0.0, z, w])
                planted.append((r, f'tie: strike tar_rot_err = float32(0.2) {("- ulp", "", "+ ulp")[k + 1]}'))
                tie_rows.append(r)
                r += 1
        assert len(ties[-1]) >= 1 and len(ties[1]) >= 1, 'no straddling pair of tie values found'
        nf0 = r
        # no override hides the planted operand: the location target 1 m away (pos_err 1 >= 0.5), the strike target nearly upright
        # (tar_rot_err 0.9 >= 0.2)
        I['tar_pos_loc'][nf0:] = I['body_pos'][nf0:, 0, :2] + torch.tensor([0.8, 0.6])
        I['tar_states'][nf0:, 3:7] = E.unit(torch.tensor([0.1, -0.2, 0.2, 1.0]))
        for what, key, idx, val in NONFINITE:
            I[key][(r,) + idx] = val
            planted.append((r, 'non-finite: ' + what))
            r += 1
        # drop a non-finite row on which the two runs differ in their NaN / infinity pattern
        O32, O64 = run(I, torch.float32), run(I, torch.float64)
        bad = [k for k in range(nf0, n) if not all(same_pattern(O32[f][k], O64[f][k]) for f in TASK_FUNCS)]
        if bad:
            keep = torch.tensor([k for k in range(n) if k not in bad])
            I = {k: (v[keep] if (v.dim() > 0 and v.shape[0] == n) else v) for k, v in I.items()}
            old = {int(k): j for j, k in enumerate(keep.tolist())}
            planted = [(old[k], w) for k, w in planted if k in old]
            n = len(keep)
            O32, O64 = run(I, torch.float32), run(I, torch.float64)
        dropped = [NONFINITE[k - nf0][0] for k in bad]
        M32, M64 = masks(I, O32, torch.float32), masks(I, O64, torch.float64)
        D32, D64 = decisions(I, torch.float32), decisions(I, torch.float64)
        rest = [k for k in range(n) if k not in tie_rows]
        for k in TASK_MASKS:
            assert torch.equal(M32[k][rest], M64[k][rest]), f'the f32 and the f64 run disagree on {k} outside the tie rows'
            cnt = [int(M32[k][:n_gen].sum()), int((~M32[k][:n_gen]).sum())]
            assert min(cnt) >= 4, (k, cnt)
        # the exact rows: the f32 and the f64 decision quantities are the same numbers
        ex = list(range(n_gen, n_gen + n_exact))
        assert torch.equal(D32['heading_speed'][0][ex].double(), D64['heading_speed'][0][ex]), 'heading_speed is not exact'
        pe64 = D64['location_pos_err'][0][:, 0]
        assert float(pe64[n_gen + 5]) == 0.5 and float(pe64[n_gen + 6]) < 0.5 < float(pe64[n_gen + 7])
        pe = D32['location_pos_err'][0][:, 0]
        assert float(pe[n_gen + 5]) == 0.5 and float(pe[n_gen + 6]) == nxt(0.5, False) and float(pe[n_gen + 7]) == nxt(0.5, True)
        sp = D32['heading_speed'][0][:, 0]
        assert float(sp[n_gen]) == 0.0 and float(sp[n_gen + 1]) == 2.0 ** -5 and float(sp[n_gen + 2]) == -2.0 ** -5
        assert float(D32['location_speed'][0][n_gen + 8, 0]) == 0.0
        v = D32['strike_rot_err'][0][tie_rows, 0]
        want = [x for k in (-1, 0, 1) for x in [{-1: nxt(0.2, False), 0: float(f32(0.2)), 1: nxt(0.2, True)}[k]] * len(ties[k])]
        assert v.tolist() == want, 'the tie rows do not sit on the f32 neighbours of 0.2'
        assert torch.equal(O32['strike_rew'][tie_rows] == 1.0, v < 0.2), 'the f32 run does not branch on the tie quantity'
        assert not E.near_threshold({k: (t[:n_gen] if (t.dim() > 0 and t.shape[0] == n) else t) for k, t in I.items()}, False).any()
        # e_ref: the group's finite non-tie elements and a 4096-row draw of the same distribution
        big = E.draw_with_margins(4096, torch.Generator().manual_seed(20264), False)
        B32, B64 = run(big, torch.float32), run(big, torch.float64)
        e_ref, mref = {}, {}
        for f in TASK_FUNCS:
            skip = tie_rows if f == 'strike_rew' else None
            e_ref[f] = max(max_err(O32[f], O64[f], skip), max_err(B32[f], B64[f]))
            mref[f] = max_ref(O64[f], skip)
        keys = ['prev_root_pos', 'tar_dir', 'tar_face_dir', 'tar_speed',
                'tar_pos_loc', 'tar_pos_reach', 'tar_states']
        inputs = {k: I[k].clone() for k in keys}
        inputs['root_states'] = root_states(I)
        inputs['reach_body_pos'] = I['body_pos'][:, E.REACH_BODY_ID].clone()
        return {'kind': 'task', 'n': n, 'B': E.B, 'contact_body_ids': list(E.CONTACT_BODY_IDS), 'strike_body_ids': list(E.STRIKE_BODY_IDS),
                'max_episode_length': E.MAX_EPISODE_LENGTH, 'dt': DT_EXACT, 'tar_speed': E.TAR_SPEED, 'reach_body_id': E.REACH_BODY_ID,
                'inputs': inputs, 'f32': {f: O32[f].clone() for f in TASK_FUNCS}, 'f64': {f: O64[f].clone() for f in TASK_FUNCS},
                'masks': pack_masks(M32, TASK_MASKS), 'planted': planted, 'tie_rows': tie_rows, 'generic_rows': list(range(n_gen)),
                'exact_rows': ex, 'free_rows': list(range(n_gen)), 'dropped': dropped, 'e_ref': e_ref, 'max_ref': mref, 'wide': False,
                'branch_counts': {k: [int(M32[k].sum()), int((~M32[k]).sum())] for k in TASK_MASKS},
                'note': 'body_pos of the recording: the root at body 0, reach_body_pos at the reach body'}


# =================================================================================================== observation groups
def draw_obs(n, B, g):
    r = lambda *s: torch.randn(*s, generator=g)
    root_pos = r(n, 3) * torch.tensor([3.0, 3.0, 0.3]) + torch.tensor([0.0, 0.0, 0.9])
    pos = root_pos.unsqueeze(1) + r(n, B, 3) * torch.tensor([0.5, 0.5, 0.35])
    pos[:, 0] = root_pos
    rot = E.unit(r(n, B, 4))
    for _ in range(50):
        # the heading is atan2 of the root's rotated x axis: a drawn root whose axis is within 0.05 of the vertical is drawn again,
        # the ill-conditioned headings are planted by name (obs_ill_conditioned)
        x, y, z, w = rot[:, 0].double().unbind(-1)
        flat = torch.hypot(1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z)) < HEADING_MARGIN
        if not flat.any():
            break
        rot[flat, 0] = E.unit(r(int(flat.sum()), 4))
    return {'body_pos': pos, 'body_rot': rot, 'body_vel': r(n, B, 3) * 2, 'body_ang_vel': r(n, B, 3) * 3}


def tilt(down, angle):
    """The x axis straight up (down) and then tilted by `angle` about z: the heading hangs on a vector of length sin(angle)."""
    s = math.sqrt(0.5)
    q = torch.tensor([0.0, s if down else -s, 0.0, s], dtype=torch.float64)          # about y by +-90 degrees
    t = torch.tensor([math.sin(angle / 2), 0.0, 0.0, math.cos(angle / 2)], dtype=torch.float64)   # then about x: off the vertical
    x1, y1, z1, w1 = t
    x2, y2, z2, w2 = q
    return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]).float()


def obs_plants(B):
    s = 0.7071067811865476
    P = [('identity root rotation', lambda I, r: I['body_rot'].__setitem__((r, 0), torch.tensor([0.0, 0.0, 0.0, 1.0]))),
         ('root half turn about z', lambda I, r: I['body_rot'].__setitem__((r, 0), torch.tensor([0.0, 0.0, 1.0, 0.0]))),
         ('root x axis straight down', lambda I, r: I['body_rot'].__setitem__((r, 0), torch.tensor([0.0, s, 0.0, s]))),
         ('root x axis straight up', lambda I, r: I['body_rot'].__setitem__((r, 0), torch.tensor([0.0, -s, 0.0, s]))),
         ('root quaternion of norm 0.5', lambda I, r: I['body_rot'].__setitem__((r, 0), I['body_rot'][r, 0] * 0.5)),
         ('root quaternion of norm 2', lambda I, r: I['body_rot'].__setitem__((r, 0), I['body_rot'][r, 0] * 2.0))]
    for field in ('body_pos', 'body_rot', 'body_vel', 'body_ang_vel'):
        for b in sorted({0, min(1, B - 1), B - 1}):
            P.append((f'NaN in {field} of body {b}', lambda I, r, f=field, b=b: I[f].__setitem__((r, b, 1), NAN)))
    P.append(('+inf in a body position', lambda I, r: I['body_pos'].__setitem__((r, B - 1, 0), INF)))
    P.append(('-inf in a body position', lambda I, r: I['body_pos'].__setitem__((r, 0, 2), -INF)))
    return P


def run_obs(I, dtype):
    J = cast(I, dtype)
    return {(lr, rh): H.compute_humanoid_observations_max(J['body_pos'], J['body_rot'], J['body_vel'], J['body_ang_vel'], lr, rh)
            for lr, rh in FLAGS}


def obs_group(n, B, seed, plants, offset=0, count=12, with_big=True, note=''):
    g = torch.Generator().manual_seed(31000 + seed)
    I = draw_obs(n, B, g)
    planted = []
    for r in range(min(n, count, len(plants))):
        what, f = plants[(offset + r) % len(plants)]
        f(I, r)
        planted.append((r, what))
    O32, O64 = run_obs(I, torch.float32), run_obs(I, torch.float64)
    for k in FLAGS:
        assert same_pattern(O32[k], O64[k]), ('the runs differ in their NaN / infinity pattern', n, B, k)
    e = max(max_err(O32[k], O64[k]) for k in FLAGS)
    if with_big:
        big = draw_obs(4096, B, torch.Generator().manual_seed(32000 + seed))
        b32, b64 = run_obs(big, torch.float32), run_obs(big, torch.float64)
        e = max(e, max(max_err(b32[k], b64[k]) for k in FLAGS))
    o_rot = 1 + 3 * (B - 1)
    cols = [0] + list(range(o_rot, o_rot + 6))
    rest = [c for c in range(15 * B - 2) if c not in cols]
    out = {}
    for tag, O in (('f32', O32), ('f64', O64)):
        base = O[(True, True)]
        d = {'obs_max': base.clone(), 'obs_max_flag_cols': {}}
        for k in FLAGS:
            same = O[k][:, rest].view(torch.int32 if O[k].dtype == torch.float32 else torch.int64)
            assert torch.equal(same, base[:, rest].view(same.dtype)), 'flag combinations differ outside the seven columns'
            d['obs_max_flag_cols'][k] = O[k][:, cols].clone()
        out[tag] = d
    return {'kind': 'obs', 'n': n, 'B': B, 'contact_body_ids': [], 'strike_body_ids': [], 'max_episode_length': 300.0, 'inputs': I,
            'f32': out['f32'], 'f64': out['f64'], 'masks': torch.zeros(0, n, dtype=torch.bool), 'planted': planted, 'tie_rows': [], 'free_rows': list(range(len(planted), n)),
            'obs_max_flag_cols': cols, 'e_ref': {'obs_max': e}, 'max_ref': {'obs_max': max(max_ref(O64[k]) for k in FLAGS)},
            'wide': False, 'note': note, 'branch_counts': {}}


def obs_groups():
    G = {}
    shapes = [(1, 1), (17, 2), (33, 5), (16, 17), (15, 24), (17, 64)]
    off = 0
    covered = set()
    for k, (n, B) in enumerate(shapes):
        P = obs_plants(B)
        grp = obs_group(n, B, k, P, offset=off)
        G[f'obs_n{n}_b{B}'] = grp
        covered |= {w.replace(f'body {B - 1}', 'body B-1') for _, w in grp['planted']}
        off += len(grp['planted'])
    P17 = obs_plants(17)
    assert len({w for w, _ in P17}) == 20 and sum(len(g['planted']) for g in G.values()) >= 2 * len(P17)
    for w in ('identity root rotation', 'root half turn about z', 'root x axis straight down', 'root x axis straight up',
              'root quaternion of norm 0.5', 'root quaternion of norm 2', '+inf in a body position', '-inf in a body position'):
        assert w in covered, w
    for field in ('body_pos', 'body_rot', 'body_vel', 'body_ang_vel'):
        for b in ('body 0', 'body 1', 'body B-1'):
            assert any(w.startswith(f'NaN in {field} of {b}') for w in covered), (field, b)
    # the ill-conditioned rows: the vertical x axis tilted by 1e-4 and 1e-3 rad; and the rows of magnitude 1e3
    ill = [(f'root x axis straight {"down" if d else "up"} tilted by {a} rad', lambda I, r, d=d, a=a: I['body_rot'].__setitem__((r, 0), tilt(d, a)))
           for d in (True, False) for a in (1e-4, 1e-3)]
    G['obs_ill_conditioned'] = obs_group(4, 5, 50, ill, count=4, with_big=False, note='heading from a vector of length 1e-4 / 1e-3')

    def far(I, r):
        root = torch.tensor([1e3, -2e3, 1.0])
        I['body_pos'][r] = root + (I['body_pos'][r] - I['body_pos'][r, 0]).clamp(-1.0, 1.0) * 0.5
        I['body_pos'][r, 0] = root
    large = [('root at (1e3, -2e3, 1), the bodies within a metre', far),
             ('velocities of 1e3', lambda I, r: (I['body_vel'].__setitem__(r, I['body_vel'][r] * 500.0), I['body_ang_vel'].__setitem__(r, I['body_ang_vel'][r] * 333.0)))]
    G['obs_large'] = obs_group(2, 17, 51, large, count=2, with_big=False, note='2^-23 max |ref| alone is 1.2e-4 at 1e3')
    return G


# =================================================================================================== the file
def allowance(grp, name):
    return 2.0 * grp['e_ref'][name] + 2.0 ** -23 * grp['max_ref'][name] + 1e-7


def float_elements(grp):
    if grp['kind'] == 'obs':
        return grp['f64']['obs_max'].numel() + 3 * grp['n'] * 7
    if grp['kind'] == 'task':
        return sum(grp['f64'][f].numel() for f in TASK_FUNCS)
    return 0


def build():
    groups = {}
    groups.update(reset_groups())
    groups['tasks'] = task_group()
    groups.update(obs_groups())
    total = wide = 0
    for name, grp in groups.items():
        over = any(allowance(grp, f) > WIDE_BAR for f in grp['e_ref'])
        grp['wide'] = bool(over)
        assert not over or name in ('obs_ill_conditioned', 'obs_large'), (name, {f: allowance(grp, f) for f in grp['e_ref']})
        total += float_elements(grp)
        wide += float_elements(grp) if over else 0
    assert wide <= WIDE_SHARE * total, (wide, total)
    return {'groups': groups, 'order': list(groups), 'margin': MARGIN, 'wide_bar': WIDE_BAR, 'wide_share': WIDE_SHARE,
            'float_elements': total, 'wide_elements': wide, 'reset_masks': RESET_MASKS, 'task_masks': TASK_MASKS}


def main():
    G = build()
    path = os.path.join(ROOT, 'tests', 'golden', 'env_edges.pt')
    torch.save(G, path)
    print('wrote', path, os.path.getsize(path), 'bytes;', G['wide_elements'], 'of', G['float_elements'], 'float elements in wide groups')
    for name in G['order']:
        grp = G['groups'][name]
        print(f'  {name:24s} n {grp["n"]:3d} B {grp["B"]:2d} planted {len(grp["planted"]):3d} ties {len(grp["tie_rows"]):2d} wide {grp["wide"]}',
              {f: f'{v:.3g}' for f, v in grp['e_ref'].items()})
    print('  dropped non-finite rows:', G['groups']['tasks']['dropped'])


if __name__ == '__main__':
    main()
