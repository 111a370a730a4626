"""A float64 torch restatement of smilify_amd.align by a DIFFERENT algorithm: weighted Kabsch / Umeyama through ``torch.linalg.svd``
with the determinant fix, gradients from autograd.  The kernels use Horn's quaternion method, a Jacobi eigen-decomposition and a
closed-form gradient (include/smilfit.h); the two share the statement of the problem, the weight rule and the status rule only.

Every function takes float64 tensors on any device (a float32 input is upcast exactly by the caller) and works one problem at a
time: the status rule branches in Python, and a degenerate problem never reaches the decomposition.  The status rule takes its
eigenvalue gap from ``torch.linalg.eigvalsh`` of Horn's matrix N."""
from collections import namedtuple

import torch

OK, DEGENERATE, EMPTY = 0, 1, 2
SENTINEL = 1e-6

Transform = namedtuple("Transform", "R t s status gap rms")


def effective_weights(src, dst, weights=None, mask=None):
    """(B,J) float64: weights (J) or (B,J) x (mask != 0), 0 where a coordinate of either point is not finite."""
    B, J = src.shape[:2]
    w = torch.ones(B, J, dtype=torch.float64, device=src.device)
    if weights is not None:
        w = w * weights.to(torch.float64)
    if mask is not None:
        w = w * (mask != 0).to(torch.float64)
    finite = torch.isfinite(src).all(-1) & torch.isfinite(dst).all(-1)
    return torch.where(finite, w, torch.zeros_like(w)).detach()


def horn_matrix(M):
    """N (4,4) of the moment matrix M (3,3), M[a][b] = sum w x_a y_b."""
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = M[0], M[1], M[2]
    return torch.stack([
        torch.stack([xx + yy + zz, yz - zy, zx - xz, xy - yx]),
        torch.stack([yz - zy, xx - yy - zz, xy + yx, zx + xz]),
        torch.stack([zx - xz, xy + yx, -xx + yy - zz, yz + zy]),
        torch.stack([xy - yx, zx + xz, yz + zy, -xx - yy + zz])])


def solve_one(src, dst, w, with_scale=True, min_gap=1e-10):
    """One problem: src, dst (J,3), w (J) constant weights -> Transform of 0-dim / small tensors; differentiable in src and dst."""
    kw = dict(dtype=torch.float64, device=src.device)
    eye, zero, one = torch.eye(3, **kw), torch.zeros((), **kw), torch.ones((), **kw)
    keep = w > 0
    W = w[keep].sum()
    if int(keep.sum()) == 0 or float(W) == 0.0:
        return Transform(eye, torch.zeros(3, **kw), one, EMPTY, zero, zero)
    wk, xs, ys = w[keep], src[keep], dst[keep]
    mx, my = (wk[:, None] * xs).sum(0) / W, (wk[:, None] * ys).sum(0) / W
    x, y = xs - mx, ys - my
    M = (wk[:, None] * x).T @ y
    vx = (wk * (x * x).sum(1)).sum()
    lam = torch.linalg.eigvalsh(horn_matrix(M.detach()))  # ascending
    big = max(float(lam[3]), -float(lam[0]))
    gap = (lam[3] - lam[2]) / big if big > 0.0 else zero

    def rms_of(R, s):
        r = s * x @ R.T - y
        return torch.sqrt((wk * (r * r).sum(1)).sum() / W).detach()

    if float(vx.detach()) == 0.0 or not big > 0.0 or not float(gap) > min_gap:
        return Transform(eye, (my - mx).detach(), one, DEGENERATE, gap, rms_of(eye, one))
    # y ~ R x: M = sum w x y^T = U S V^T, R = V D U^T with D = diag(1, 1, det(V U^T))
    U, S, Vh = torch.linalg.svd(M)
    d = torch.sign(torch.linalg.det(Vh.T @ U.T)).detach()
    D = torch.stack([one, one, d])
    R = Vh.T @ torch.diag(D) @ U.T
    s = (S * D).sum() / vx if with_scale else one
    t = my - s * (R @ mx)
    return Transform(R, t, s, OK, gap, rms_of(R.detach(), s.detach()))


def similarity_transform(src, dst, weights=None, mask=None, with_scale=True, min_gap=1e-10, robust_iters=0, robust_scale=None):
    """src, dst (B,J,3) float64 -> (Transform of stacked (B,...) tensors, final weights (B,J)).  The robust loop re-solves
    ``robust_iters`` times with w = w0 / sqrt(1 + r^2 / robust_scale^2), r under the solve before; the gradient takes the final
    weights as constants."""
    assert src.dtype == torch.float64 and dst.dtype == torch.float64
    B = src.shape[0]
    w0 = effective_weights(src, dst, weights, mask)
    out, w_final = [], []
    for b in range(B):
        w = w0[b]
        x = solve_one(src[b], dst[b], w, with_scale, min_gap)
        for _ in range(robust_iters):
            with torch.no_grad():
                keep = w0[b] > 0
                r = x.s * src[b] @ x.R.T + x.t - dst[b]
                r2 = torch.where(keep, (r * r).sum(1), torch.zeros_like(w))
                w = torch.where(keep, w0[b] / torch.sqrt(1.0 + r2 / robust_scale ** 2), torch.zeros_like(w))
            x = solve_one(src[b], dst[b], w, with_scale, min_gap)
        out.append(x)
        w_final.append(w)
    kw = dict(dtype=torch.float64, device=src.device)
    stack = lambda xs, shape: torch.stack(xs) if xs else torch.zeros((0,) + shape, **kw)  # noqa: E731
    return Transform(stack([o.R for o in out], (3, 3)), stack([o.t for o in out], (3,)), stack([o.s for o in out], ()),
                     torch.tensor([o.status for o in out], dtype=torch.int32, device=src.device),
                     stack([o.gap for o in out], ()), stack([o.rms for o in out], ())), stack(w_final, (src.shape[1],))


def rigid_transform(src, dst, **kw):
    return similarity_transform(src, dst, with_scale=False, **kw)


def apply_transform(points, R, t, s):
    return s[..., None, None] * points @ R.transpose(-1, -2) + t[..., None, :]


def joint_errors(pred, target, mask=None, align="none", sentinel=True, scale=1.0, min_gap=1e-10):
    """(dist (B,J), valid (B,J) bool, status (B) int32) of float64 pred, target (B,J,3)."""
    valid = torch.isfinite(pred).all(-1) & torch.isfinite(target).all(-1)
    if mask is not None:
        valid = valid & (mask != 0)
    if sentinel:
        valid = valid & (torch.sqrt((torch.where(torch.isfinite(target), target, torch.zeros_like(target)) ** 2).sum(-1)) > SENTINEL)
    if align == "none":
        status = torch.where(valid.any(1), OK, EMPTY).to(torch.int32)
        diff = pred - target
    else:
        x, _ = similarity_transform(pred, target, mask=valid, with_scale=align == "similarity", min_gap=min_gap)
        # t = my - s R mx in every status: the aligned difference over the centred points, which does not cancel against the offset
        w = valid.to(torch.float64)[..., None]
        W = w.sum(1).clamp(min=1.0)
        mx = (w * torch.where(valid[..., None], pred, torch.zeros_like(pred))).sum(1) / W
        my = (w * torch.where(valid[..., None], target, torch.zeros_like(target))).sum(1) / W
        status = x.status
        diff = x.s[:, None, None] * (pred - mx[:, None]) @ x.R.transpose(1, 2) - (target - my[:, None])
    d = scale * torch.sqrt((diff ** 2).sum(-1))
    return torch.where(valid, d, torch.zeros_like(d)).detach(), valid, status


def pooled(dist, valid):
    n = valid.sum()
    return dist.sum() / n if int(n) > 0 else dist.sum() * 0.0


def mpjpe(pred, target, mask=None, sentinel=True, scale=1.0):
    return pooled(*joint_errors(pred, target, mask, "none", sentinel, scale)[:2])


def pa_mpjpe(pred, target, mask=None, with_scale=True, sentinel=True, scale=1.0, min_gap=1e-10):
    return pooled(*joint_errors(pred, target, mask, "similarity" if with_scale else "rigid", sentinel, scale, min_gap)[:2])


def value_and_grads(src, dst, probes, wrt=("src", "dst"), **kw):
    """The transform of float64 src, dst and the gradients of sum_k (out_k * probes[k]) over R, t, s with respect to ``wrt``.
    Returns (Transform, final weights, {name: gradient})."""
    leaves = {"src": src.detach().clone().requires_grad_("src" in wrt), "dst": dst.detach().clone().requires_grad_("dst" in wrt)}
    x, w = similarity_transform(leaves["src"], leaves["dst"], **kw)
    obj = (x.R * probes["R"]).sum() + (x.t * probes["t"]).sum() + (x.s * probes["s"]).sum()
    grads = {}
    if obj.requires_grad:
        got = torch.autograd.grad(obj, [leaves[k] for k in wrt], allow_unused=True)
        grads = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(wrt, got)}
    else:
        grads = {k: torch.zeros_like(leaves[k]) for k in wrt}
    return Transform(*(v.detach() for v in x)), w, grads
