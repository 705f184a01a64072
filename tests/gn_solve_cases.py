"""The normal equations and updates the solve-stage tests run (tests/test_gn_solve_ref.py on the CPU, tests/test_gpu_gn_solve.py on the
GPU). Everything is seeded and built once per process; what the sets must cover is asserted from the restatement alone
(tests/gn_solve_ref.py) in test_gn_solve_ref.py, not assumed here."""
import functools
import math

import numpy as np

import gn_solve_ref as ref

Case = ref.collections.namedtuple("Case", "name H B kind")
ALL_PIVOT_PAIRS = frozenset((k, r) for k in range(6) for r in range(k, 6))  # 21 (step, pivot row) choices


def _mirror(H):
    """Exactly symmetric: the kernels see the upper triangle only."""
    return np.triu(H) + np.triu(H, 1).T


@functools.lru_cache(maxsize=None)
def pivot_cases():
    """Symmetric 6×6 matrices, positive semi-definite (JᵀJ of a Jacobian with badly scaled columns) and indefinite, picked greedily from a
    seeded stream: a candidate stays when its factorisation takes a (step, pivot row) choice no earlier member took."""
    rng = np.random.RandomState(20261)
    out, seen, kinds = [], set(), set()
    for trial in range(4000):
        kind = "psd" if trial % 2 == 0 else "indefinite"
        scale = 10.0 ** rng.uniform(-1.5, 1.5, 6)
        if kind == "psd":
            J = rng.randn(12, 6) * scale
            H = _mirror(J.T @ J)
        else:
            A = rng.randn(6, 6) * scale
            H = _mirror(A + A.T)
        B = rng.randn(6) * 10.0 ** rng.uniform(-2, 1)
        pairs = set(enumerate(ref.lu6(H.tolist(), B.tolist()).pivots))
        if not pairs <= seen or kind not in kinds:
            out.append(Case("pivot%02d_%s" % (len(out), kind), H, B, kind))
            seen |= pairs
            kinds.add(kind)
        if seen == ALL_PIVOT_PAIRS and len(kinds) == 2:
            break
    return tuple(out)


@functools.lru_cache(maxsize=None)
def singular_cases():
    """det(H) == 0.0 exactly. `structural k`: row and column k are zero, so the pivot of step k is a zero that was there from the start.
    `cancel k`: a block [[s, s], [s, s]] on rows k − 1, k with nothing else in those rows — step k − 1 eliminates with f = 1 and leaves an
    exact zero as the pivot of step k. Around them a random symmetric rest keeps the later steps pivoting on real numbers.
    `two zeros`: steps 0 and 2. `underflow`: every pivot is 1e-60, nothing is singular, and the product underflows to 0.0."""
    rng = np.random.RandomState(20262)
    out = []

    def rest():
        A = rng.randn(6, 6)
        return _mirror(A + A.T + 3.0 * np.diag(rng.rand(6)))

    for k in range(6):
        H = rest()
        H[k, :] = 0.0
        H[:, k] = 0.0
        out.append(Case("structural%d" % k, H, rng.randn(6), "singular"))
    for k in range(1, 6):
        H = rest()
        for i in (k - 1, k):
            H[i, :] = 0.0
            H[:, i] = 0.0
        H[k - 1:k + 1, k - 1:k + 1] = 0.75 * 2.0 ** (k - 2)
        out.append(Case("cancel%d" % k, H, rng.randn(6), "singular"))
    H = rest()
    for k in (0, 2):
        H[k, :] = 0.0
        H[:, k] = 0.0
    out.append(Case("two_zeros", H, rng.randn(6), "singular"))
    out.append(Case("underflow", 1e-60 * np.eye(6), 1e-60 * rng.randn(6), "singular"))
    return tuple(out)


def regular_case(seed=0):
    """A well-conditioned JᵀJ with a small right-hand side."""
    rng = np.random.RandomState(20263 + seed)
    J = rng.randn(50, 6)
    return Case("regular%d" % seed, _mirror(J.T @ J), rng.randn(6) * 0.1, "psd")


UNIT_QS = (
    ("identity", (0.0, 0.0, 0.0, 1.0)),
    ("half", (0.5, -0.5, 0.5, 0.5)),  # exactly unit: 4 · ¼
)


@functools.lru_cache(maxsize=None)
def update_cases():
    """(name, q_in, t_in, dx): rotation angles 0, just below and at the Taylor threshold 1e-10, 1e-3, 1, π and 2π − 1e-6 — about the x axis
    (theta is then |dx[0]| exactly) and about (1, −2, 3)/√14 — on q_in = identity, an exactly unit q, a generic normalised q and the same
    off-unit by 1e-12."""
    g = np.array([0.1, -0.2, 0.3, 0.9])
    g = g / np.linalg.norm(g)
    qs = UNIT_QS + (("generic", tuple(g)), ("off_unit", tuple(g * (1.0 + 1e-12))))
    thetas = (("0", 0.0), ("below", math.nextafter(ref.TAYLOR_BELOW, 0.0)), ("at", ref.TAYLOR_BELOW), ("1e-3", 1e-3), ("1", 1.0), ("pi", math.pi),
              ("2pi-", 2.0 * math.pi - 1e-6))
    axis = np.array([1.0, -2.0, 3.0]) / math.sqrt(14.0)
    out = []
    for qn, q in qs:
        for tn, th in thetas:
            for an, w in (("x", np.array([th, 0.0, 0.0])), ("mixed", th * axis + 0.0)):  # + 0.0: no −0.0 in a right-hand side (the substitution would hand back +0.0)
                out.append(("%s_%s_%s" % (qn, tn, an), q, (1.5, -2.25, 40.0), tuple(w) + (0.125, -3e-3, 7.0)))
    return tuple(out)


def identity_row(dx, eff=100):
    """The one-row partial whose solution is dx itself, bit for bit (H = I: every product of the substitution is a zero)."""
    return ref.pack_row(np.eye(6), dx, eff)


@functools.lru_cache(maxsize=None)
def norm_split_dx(running_sum_smaller):
    """A dx whose |dx| differs in the last bit between the library's association and the plain running sum — the running sum giving the
    smaller (or the larger) of the two — found by seeded search: → (dx [6], |dx| in the library's association, |dx| summed left to right)."""
    rng = np.random.RandomState(20264)
    for _ in range(100000):
        dx = [float(v) for v in rng.randn(6) * 1e-3]
        a, b = ref.norm6(dx), ref.norm6_left_to_right(dx)
        if a != b and (b < a) == running_sum_smaller:
            return tuple(dx), a, b
    raise AssertionError("no dx separates the two associations")


def spread_rows(rng, n_scans, blocks):
    """[n_scans, blocks, 32] block partials of magnitudes 2^-20 … 2^20 with mixed signs, small whole effective counts, NaN in the four
    spare columns."""
    p = rng.choice([-1.0, 1.0], (n_scans, blocks, ref.ACC_W)) * (1.0 + rng.rand(n_scans, blocks, ref.ACC_W)) * 2.0 ** rng.randint(-20, 21, (n_scans, blocks, ref.ACC_W))
    p[:, :, 27] = rng.randint(0, 50, (n_scans, blocks))
    p[:, :, 28:] = np.nan
    return p


def trig_update_error(update):
    """max |q − q_ld| over the sin/cos members of update_cases() for update(q, t, dx) → q: the worst component error against the
    long-double restatement."""
    worst = 0.0
    for name, q, t, dx in update_cases():
        if ref.apply_update_f64(q, t, dx).taylor:
            continue
        q_ld, _ = ref.apply_update_ld(q, t, dx)
        worst = max(worst, float(np.abs(np.asarray(update(q, t, dx), dtype=np.float64).astype(ref.LD) - q_ld).max()))
    return worst
