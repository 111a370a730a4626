"""Seeded case sets for the alignment tests (tests/test_align_cpu.py, tests/test_gpu_align.py): float64 CPU tensors.

* ``regular``: problems that determine their rotation well - ``check_regular`` asserts gap >= 0.01, the cloud at most 1e3 spreads from
  the origin (spread: the weighted rms radius of src) and at least 4 points carrying weight.  Random rotations with every third
  angle within 1e-1 .. 1e-6 of pi, scales 0.2 .. 5, noise 0 .. 0.3 spread, zero weights, masks, and every fifth target mirrored.
* ``degenerate``: exact sets that do not determine a rotation, in coordinates that are multiples of 1/8 so that every sum is exact.
* ``outliers``: J = 30, noise 0.01, six joints displaced by N(0, 5^2).
"""
import math

import torch

import align_ref as ref

MIN_GAP_REGULAR = 0.01
MAX_OFFSET_SPREADS = 1e3


def _gen(*seed):
    g = torch.Generator()
    g.manual_seed(int(sum(s * m for s, m in zip(seed, (1000003, 10007, 101, 1))) % (2 ** 31)))
    return g


def rotation(axis, angle):
    """Rodrigues, float64: axis (3) (normalised here), angle in radians."""
    k = axis / axis.norm()
    K = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def probes(B, seed):
    """Seeded weights of the scalar the gradient tests differentiate: sum(R pR) + sum(t pt) + sum(s ps)."""
    g = _gen(seed, 77)
    r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64) * 2.0 - 1.0  # noqa: E731
    return {"R": r(B, 3, 3), "t": r(B, 3), "s": r(B)}


def _problem(J, g, b, w, mask):
    """One candidate: (src, dst, truth) with J points."""
    u = lambda lo, hi: lo + (hi - lo) * float(torch.rand((), generator=g, dtype=torch.float64))  # noqa: E731
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    spread = 10.0 ** u(-1.3, 1.7)
    offset = spread * 10.0 ** u(0.0, 2.3) * torch.nn.functional.normalize(n(3), dim=0)
    src = spread * n(J, 3) + offset
    angle = math.pi - 10.0 ** u(-6.0, -1.0) if b % 3 == 2 else u(0.0, math.pi)
    R = rotation(n(3), angle)
    s = 10.0 ** u(math.log10(0.2), math.log10(5.0))
    t = 10.0 * spread * n(3)
    noise = (0.0, 1e-3, 0.05, 0.3)[b % 4] * spread * s
    dst = s * src @ R.T + t + noise * n(J, 3)
    if b % 5 == 3:  # a mirrored target: no proper rotation fits it, and a proper rotation must still come back
        c = dst.mean(0)
        dst = (dst - c) * torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64) + c
    dead = ~((w > 0) & (mask != 0))
    src = torch.where((dead & (torch.arange(J) % 2 == 0))[:, None], torch.full_like(src, 1e6), src)  # a joint without weight is not read
    return src, dst, dict(R=R, t=t, s=s)


def regular(B, J, seed=0, weights="BJ", masked=True, min_points=4):
    """``B`` regular problems of ``J >= 4`` points: dict(src, dst (B,J,3), weights (B,J) / (J) / None, mask (B,J) uint8 / None).
    ``weights``: "BJ", "J" or None.  Candidates that miss the conditions are drawn again (seeded: the set is the same every time)."""
    assert J >= min_points
    g0 = _gen(seed, B, J)
    wJ = None
    if weights == "J":
        wJ = 0.2 + 1.8 * torch.rand(J, generator=g0, dtype=torch.float64)
        if J > 6:
            wJ[torch.randperm(J, generator=g0)[: J // 5]] = 0.0
    srcs, dsts, ws, ms = [], [], [], []
    for b in range(B):
        for attempt in range(200):
            g = _gen(seed, B, J, 1 + b + 1000 * attempt)
            w = torch.ones(J, dtype=torch.float64)
            if weights == "BJ":
                w = 0.2 + 1.8 * torch.rand(J, generator=g, dtype=torch.float64)
                if J > 6:
                    w[torch.randperm(J, generator=g)[: J // 5]] = 0.0
            elif weights == "J":
                w = wJ
            m = torch.ones(J, dtype=torch.uint8)
            if masked and J > 6:
                m[torch.randperm(J, generator=g)[: J // 6]] = 0
            src, dst, _ = _problem(J, g, b, w, m)
            if _conditions(src, dst, w * m, min_points)[0]:
                break
        else:
            raise AssertionError(f"no regular problem found for b={b}")
        srcs.append(src), dsts.append(dst), ws.append(w), ms.append(m)
    st = lambda xs, tail: torch.stack(xs) if xs else torch.zeros((0,) + tail, dtype=torch.float64)  # noqa: E731
    out = dict(src=st(srcs, (J, 3)), dst=st(dsts, (J, 3)), weights=None, mask=None)
    if weights == "BJ":
        out["weights"] = st(ws, (J,))
    elif weights == "J":
        out["weights"] = wJ
    if masked:
        out["mask"] = torch.stack(ms) if ms else torch.zeros(0, J, dtype=torch.uint8)
    return out


def _conditions(src, dst, w, min_points=4):
    """(ok, gap, offset in spreads, points with weight) of one problem under the effective weights ``w`` (J)."""
    keep = w > 0
    n = int(keep.sum())
    if n < min_points:
        return False, 0.0, float("inf"), n
    wk, xs = w[keep], src[keep]
    W = wk.sum()
    mx = (wk[:, None] * xs).sum(0) / W
    spread = math.sqrt(float((wk * ((xs - mx) ** 2).sum(1)).sum() / W))
    x = ref.solve_one(src, dst, w)
    off = float(mx.norm()) / spread if spread > 0 else float("inf")
    gap = float(x.gap)
    return x.status == ref.OK and gap >= MIN_GAP_REGULAR and off <= MAX_OFFSET_SPREADS, gap, off, n


def check_regular(src, dst, weights=None, mask=None):
    """Assert the regular set's conditions on float64 (B,J,3) inputs as a test will pass them (after any cast)."""
    w = ref.effective_weights(src, dst, weights, mask)
    for b in range(src.shape[0]):
        ok, gap, off, n = _conditions(src[b], dst[b], w[b])
        assert n >= 4, f"problem {b}: {n} points carry weight"
        assert gap >= MIN_GAP_REGULAR, f"problem {b}: gap {gap}"
        assert off <= MAX_OFFSET_SPREADS, f"problem {b}: the cloud lies {off} spreads from the origin"
        assert ok


def wave_edge(B, J, seed=0, weights="BJ"):
    """The problems of the wave-edge shapes, any J >= 0: the regular set for J >= 4; for J == 3 the same generator under the gap and
    offset conditions alone (three points determine a rotation, the set's fourth point is what they lack); for J < 3 random points,
    which determine none.  dict as ``regular``."""
    if J >= 4:
        return regular(B, J, seed, weights)
    if J == 3:
        return regular(B, J, seed, weights, min_points=3)
    g = _gen(seed, B, J, 9)
    out = dict(src=3.0 * torch.randn(B, J, 3, generator=g, dtype=torch.float64) + 5.0, dst=torch.randn(B, J, 3, generator=g, dtype=torch.float64),
               weights=None, mask=torch.ones(B, J, dtype=torch.uint8))
    if weights == "BJ":
        out["weights"] = 0.2 + torch.rand(B, J, generator=g, dtype=torch.float64)
    elif weights == "J":
        out["weights"] = 0.2 + torch.rand(J, generator=g, dtype=torch.float64)
    return out


def _eighths(g, *shape):
    return torch.randint(-64, 65, shape, generator=g).to(torch.float64) / 8.0


def degenerate():
    """[(name, dict(src, dst (1,J,3), weights, mask), expected status)]: inputs that determine no rotation.  Coordinates are
    multiples of 1/8 below 2^4 and the weights are 1: every sum the kernels and the restatement take is exact."""
    g = _gen(5, 5)
    out = []
    p = torch.tensor([1.5, -2.0, 0.25], dtype=torch.float64)
    out.append(("all_equal", dict(src=p.expand(1, 5, 3).clone(), dst=_eighths(g, 1, 5, 3)), ref.DEGENERATE))
    out.append(("one_point", dict(src=_eighths(g, 1, 1, 3), dst=_eighths(g, 1, 1, 3)), ref.DEGENERATE))
    out.append(("two_points", dict(src=_eighths(g, 1, 2, 3), dst=_eighths(g, 1, 2, 3)), ref.DEGENERATE))
    k = torch.tensor([-3.0, -1.0, 0.0, 1.0, 2.0, 5.0], dtype=torch.float64)
    line = k[:, None] * torch.tensor([1.0, 2.0, -0.5], dtype=torch.float64) + torch.tensor([3.0, 0.0, 1.0], dtype=torch.float64)
    out.append(("collinear", dict(src=line[None].clone(), dst=_eighths(g, 1, 6, 3)), ref.DEGENERATE))
    out.append(("two_after_mask", dict(src=_eighths(g, 1, 6, 3), dst=_eighths(g, 1, 6, 3),
                                       mask=torch.tensor([[0, 1, 0, 0, 1, 0]], dtype=torch.uint8)), ref.DEGENERATE))
    out.append(("all_masked", dict(src=_eighths(g, 1, 5, 3), dst=_eighths(g, 1, 5, 3), mask=torch.zeros(1, 5, dtype=torch.uint8)), ref.EMPTY))
    out.append(("zero_weights", dict(src=_eighths(g, 1, 5, 3), dst=_eighths(g, 1, 5, 3), weights=torch.zeros(5, dtype=torch.float64)),
                ref.EMPTY))
    out.append(("no_joints", dict(src=torch.zeros(1, 0, 3, dtype=torch.float64), dst=torch.zeros(1, 0, 3, dtype=torch.float64)), ref.EMPTY))
    nan = _eighths(g, 1, 4, 3)
    nan_dst = _eighths(g, 1, 4, 3)
    nan[0, 0, 1] = float("nan")
    nan_dst[0, 1, 2] = float("inf")
    out.append(("two_after_nan", dict(src=nan, dst=nan_dst), ref.DEGENERATE))
    return [(n, dict(dict(weights=None, mask=None), **d), s) for n, d, s in out]


def with_nan(J=9, seed=3):
    """A regular problem (1,J,3) with a NaN in one src joint and an infinity in one dst joint: both joints drop out."""
    c = regular(1, J, seed, weights=None, masked=False)
    c["src"][0, 2, 1] = float("nan")
    c["dst"][0, 5, 0] = float("-inf")
    return c


def outliers(seed):
    """dict(src, dst (1,30,3), truth): dst = R src + t + 0.01 noise with six joints displaced by N(0, 5^2) on top."""
    g = _gen(seed, 30, 6)
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    src = n(30, 3)
    R = rotation(n(3), math.pi * float(torch.rand((), generator=g, dtype=torch.float64)))
    t = n(3)
    dst = src @ R.T + t + 0.01 * n(30, 3)
    idx = torch.randperm(30, generator=g)[:6]
    dst[idx] += 5.0 * n(6, 3)
    return dict(src=src[None], dst=dst[None], R=R, t=t, idx=idx)


def transform_error(x, case):
    """The largest coordinate difference between the src points under the estimated and under the true transform."""
    src = case["src"][0]
    return float((ref.apply_transform(src, x.R[0].detach(), x.t[0].detach(), x.s[0].detach()) - (src @ case["R"].T + case["t"])).abs().max())
