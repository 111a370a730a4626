"""TEST INFRASTRUCTURE ONLY: a float64 restatement of what ``smilify_amd/csrc/fit.hip`` computes.

Plain torch, float64 throughout, gradients by autograd.  Written from the formulas (``oracle/fitter_ref.py``
states the same ones in float32, window by window): the loss of an iteration is the SUM OVER WINDOWS OF THE
WINDOW MEAN plus the three frame-to-frame terms, so a frame's mean-type terms are divided by the size of its
own window.  ``tests/test_fit_ref_cpu.py`` pins this file against the oracle, the reference goldens and
``torch.optim.Adam`` without a GPU; ``tests/test_gpu_fit_kernels.py`` pins the kernels against it.

Objective slots (``include/smilfit.h``): 0 joint, 1 limit, 2 pose, 3 splay, 4 betas, 5 sil_reproj,
6 temporal joints, 7 temporal global rotation, 8 temporal translation.
Weights are in the reference's order: w_j2d, w_reproj, w_betas, w_pose, w_limit, w_splay.
"""
from __future__ import annotations

import torch

F64 = torch.float64
U32 = 2.0 ** -24  # unit roundoff of float32


def _d(x):
    return None if x is None else torch.as_tensor(x).detach().to("cpu", F64)


def window_sizes(N, window, frame0=0, N_total=None):
    """(N,) float64: the size of the window that holds each local frame (the last window may be partial)."""
    N_total = N if N_total is None else N_total
    w = window if window > 0 else N_total
    gi = torch.arange(frame0, frame0 + N)
    start = torch.div(gi, w, rounding_mode="floor") * w
    return torch.minimum(torch.full_like(start, w), N_total - start).to(F64)


def windows_starting_in(N, window, frame0=0, N_total=None):
    """Number of windows whose FIRST frame lies in [frame0, frame0 + N)."""
    N_total = N if N_total is None else N_total
    w = window if window > 0 else N_total
    return sum(1 for s in range(0, N_total, w) if frame0 <= s < frame0 + N)


def _grad(term, leaf):
    if not term.requires_grad:
        return torch.zeros_like(leaf)
    (g,) = torch.autograd.grad(term, leaf, allow_unused=True, retain_graph=True)
    return torch.zeros_like(leaf) if g is None else g


def priors_and_temporal(pose, trans, betas, mean_betas, prec, mask, weights, w_temp, limit, window, frame0=0, N_total=None,
                        halo_prev=None, halo_next=None, train=(True, True, True), upstream=None):
    """The limit / pose / splay / shape priors and the temporal terms of frames [frame0, frame0 + N) of an N_total sequence.

    pose (N,J,3) = [global rotation ; joint rotations], mask (J,3), trans (N,3); halo rows (3J+3,) = the neighbouring frame's
    [pose row ; trans] (needed for the temporal terms of a shard).  ``train`` = (global, joints, trans) flags: a frozen block
    gets zero gradient rows, objectives are unchanged.  ``upstream`` = (d_pose, d_trans) to accumulate: added BEFORE mask and
    train are applied.  Returns objs (9,), d_pose, d_trans, d_betas and abs_pose / abs_trans / abs_betas: for every gradient
    element the sum of the absolute values of its contributions (the companion a rounding bound needs)."""
    pose, trans, mask = _d(pose), _d(trans), _d(mask)
    N, J = pose.shape[0], pose.shape[1]
    N_total = N if N_total is None else N_total
    P3 = 3 * J
    w_j2d, w_reproj, w_betas, w_pose, w_limit, w_splay = [float(w) for w in weights]
    w_temp, limit = float(w_temp), float(limit)
    bw = window_sizes(N, window, frame0, N_total)[:, None]  # (N,1)
    maskrow = torch.cat([mask.reshape(P3), torch.ones(3, dtype=F64)])
    rows = torch.cat([pose.reshape(N, P3), trans], 1) * maskrow  # masked values, (N, 3J+3)
    objs = torch.zeros(9, dtype=F64)
    contrib = []  # gradient contributions w.r.t. the masked values, each (N, 3J+3)

    def widen(gj):  # joint-rotation block -> full row
        return torch.cat([torch.zeros(N, 3, dtype=F64), gj, torch.zeros(N, 3, dtype=F64)], 1)

    # priors on the joint rotations (everything but the root), each with a leaf of its own so that its contribution is separate
    for slot, active in ((1, w_limit > 0), (2, w_pose > 0), (3, w_splay > 0)):
        if not active:
            continue
        x = rows[:, 3:P3].clone().requires_grad_()
        if slot == 1:  # mean over b_w * (J-1) * 3 of the two hinges; torch.max against zeros halves the gradient at a tie
            z = torch.zeros_like(x)
            term = (w_limit * (torch.max(x - limit, z) + torch.max(-limit - x, z)) / (bw * (P3 - 3))).sum()
        elif slot == 2:  # identity-precision pose prior, root excluded, mean over b_w * 3J
            term = (w_pose * x ** 2 / (bw * P3)).sum()
        else:  # splay: SUM over the x and z components
            term = w_splay * (x.reshape(N, J - 1, 3)[:, :, [0, 2]] ** 2).sum()
        objs[slot] = term.detach()
        contrib.append(widen(_grad(term, x)))

    # temporal terms: pair (g, g+1) belongs to the earlier frame; a frame's gradient sees both of its pairs
    if w_temp > 0:
        has_prev, has_next = frame0 > 0, frame0 + N < N_total
        if has_prev and halo_prev is None or has_next and halo_next is None:
            raise ValueError("a shard needs its halo rows for the temporal terms")
        xa, xb = rows.clone().requires_grad_(), rows.clone().requires_grad_()  # as the earlier / the later frame of a pair
        pre = [_d(halo_prev)[None] * maskrow] if has_prev else []
        post = [_d(halo_next)[None] * maskrow] if has_next else []
        ea, eb = torch.cat(pre + [xa] + post, 0), torch.cat(pre + [xb] + post, 0)
        norm = torch.cat([torch.full((3,), 3.0), torch.full((P3 - 3,), float(P3 - 3)), torch.full((3,), 3.0)]).to(F64)
        pair = w_temp * (ea[:-1] - eb[1:]) ** 2 / norm  # (pairs, 3J+3); pair k's earlier frame is extended row k
        own = pair[1:] if has_prev else pair
        objs[7], objs[6], objs[8] = own[:, :3].sum().detach(), own[:, 3:P3].sum().detach(), own[:, P3:].sum().detach()
        if own.numel():
            contrib.append(_grad(own.sum(), xa))
        if pair.numel():
            contrib.append(_grad(pair.sum(), xb))  # includes the pair owned by the previous shard's last frame

    up = torch.zeros(N, P3 + 3, dtype=F64)
    if upstream is not None:
        up = torch.cat([_d(upstream[0]).reshape(N, P3), _d(upstream[1])], 1)
    trainrow = torch.cat([torch.full((3,), float(bool(train[0]))), torch.full((P3 - 3,), float(bool(train[1]))),
                          torch.full((3,), float(bool(train[2])))]).to(F64)
    total = up + sum(contrib) if contrib else up
    total_abs = up.abs() + sum(c.abs() for c in contrib) if contrib else up.abs()
    g = total * maskrow * trainrow
    g_abs = total_abs * maskrow.abs() * trainrow

    # shape prior: w_betas * mean(((betas - mean) @ prec)^2), the same for every window, once per window that starts here
    nB = 0 if betas is None else int(_d(betas).numel())
    d_betas, abs_betas = torch.zeros(nB, dtype=F64), torch.zeros(nB, dtype=F64)
    if w_betas > 0 and nB > 0:
        b, mb, P = _d(betas).clone().requires_grad_(), _d(mean_betas), _d(prec).reshape(nB, nB)
        n_win = windows_starting_in(N, window, frame0, N_total)
        term = n_win * w_betas * (torch.matmul(b - mb, P) ** 2).mean()
        objs[4] = term.detach()
        d_betas = _grad(term, b)
        abs_betas = n_win * w_betas * 2.0 / nB * (P.abs() @ ((b.detach() - mb).abs() @ P.abs()))
    return dict(objs=objs, d_pose=g[:, :P3].reshape(N, J, 3), d_trans=g[:, P3:], d_betas=d_betas,
                abs_pose=g_abs[:, :P3].reshape(N, J, 3), abs_trans=g_abs[:, P3:], abs_betas=abs_betas)


def _select(proj, canon, Jc):
    return proj[:, :Jc] if canon is None else proj[:, torch.as_tensor(canon, dtype=torch.long)]


def joint_term(proj, target, visibility, w_j2d, views, window, canon=None, frame0=0, N_total=None):
    """2-D joint loss.  proj (N*views, J, 2) over all model joints, ``canon`` the list of annotated ones (None: the first Jc),
    target (N*views, Jc, 2), visibility (N*views, Jc).  Per window the mean over b_w * views * Jc * 2 entries; an invisible entry
    contributes nothing but is counted in the denominator.  Returns (objective, d_proj, abs_proj)."""
    proj = _d(proj).clone().requires_grad_()
    target, vis = _d(target), _d(visibility) != 0
    n_img, Jc = target.shape[0], target.shape[1]
    bw = window_sizes(n_img // views, window, frame0, N_total).repeat_interleave(views)[:, None, None]
    sq = (_select(proj, canon, Jc) - target) ** 2 * vis[:, :, None]
    term = (float(w_j2d) * sq / (bw * views * Jc * 2)).sum()
    g = _grad(term, proj)
    return term.detach(), g, g.abs()  # one contribution per element


def window_terms(pose, mask, betas, mean_betas, prec, weights, limit, window, frame0=0, N_total=None, proj=None, target=None,
                 visibility=None, views=1, canon=None, loss_img=None, pix_scale=None):
    """(windows, 6) = [joint, limit, pose, splay, betas, sil_reproj] of every window of a shard that starts on a window boundary."""
    pose = _d(pose)
    N = pose.shape[0]
    N_total = N if N_total is None else N_total
    w = window if window > 0 else N_total
    if frame0 % w:
        raise ValueError("the shard starts inside a window")
    rows = []
    for s in range(0, N, w):
        n = min(w, N - s)
        f0 = frame0 + s
        r = priors_and_temporal(pose[s:s + n], torch.zeros(n, 3), betas, mean_betas, prec, mask, weights, 0.0, limit, window, f0, N_total)
        row = torch.zeros(6, dtype=F64)
        row[1:5] = r["objs"][1:5]
        if proj is not None and float(weights[0]) > 0:
            sl = slice(s * views, (s + n) * views)
            row[0] = joint_term(proj[sl], target[sl], visibility[sl], weights[0], views, window, canon, f0, N_total)[0]
        if loss_img is not None:
            sl = slice(s * views, (s + n) * views)
            row[5] = (_d(loss_img)[sl] * _d(pix_scale)[sl]).sum()
        rows.append(row)
    return torch.stack(rows)


def pix_scale(N, views, S, w_reproj, window, frame0=0, N_total=None):
    """(N*views,): w_reproj / (b_w * views * S^2) for every image."""
    return float(w_reproj) / (window_sizes(N, window, frame0, N_total).repeat_interleave(views) * views * S * S)


def fov_reduce(d_fov_img, fov_deg):
    """d_fov[c] = d tan-half-angle chain applied to the sum of the images that use fov row c (image n uses row n % nFov).
    Returns (d_fov, abs companion)."""
    x, fov = _d(d_fov_img), _d(fov_deg)
    k = fov.numel()
    t = torch.tan(fov * (torch.pi / 180.0) / 2.0)
    f = -(torch.pi / 360.0) * (1.0 + t * t) / t
    cols = x.reshape(-1, k)
    return f * cols.sum(0), f.abs() * cols.abs().sum(0)


def adam_iter(param, grads, lr, beta1=0.5, beta2=0.999, eps=1e-8, exp_avg=None, exp_avg_sq=None, step0=0):
    """``torch.optim.Adam`` (single-tensor form, no amsgrad, no weight decay) step by step in float64.  ``grads`` is an iterable
    of gradients; yields (param, exp_avg, exp_avg_sq) after every step (fresh tensors).  ``step0`` steps were taken before."""
    p = _d(param).clone()
    m = torch.zeros_like(p) if exp_avg is None else _d(exp_avg).clone()
    v = torch.zeros_like(p) if exp_avg_sq is None else _d(exp_avg_sq).clone()
    t = int(step0)
    for g in grads:
        g = _d(g)
        t += 1
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
        yield p, m, v


def adam(param, grads, lr, beta1=0.5, beta2=0.999, eps=1e-8, exp_avg=None, exp_avg_sq=None, step0=0):
    """List of (param, exp_avg, exp_avg_sq) after every step of ``adam_iter``."""
    return list(adam_iter(param, grads, lr, beta1, beta2, eps, exp_avg, exp_avg_sq, step0))
