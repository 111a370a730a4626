"""The autograd side of the drop-in ``SMALFitter.forward`` / ``get_temporal``, the state a fitter caches (``FitState``, the epoch
served to ``forward`` among it) and the parts its three fingerprints - target signature, epoch key, graph key - are assembled from.

Ownership: the autograd nodes never hold the fitter strongly.  ``_FitWindow`` and ``_TemporalTerm`` keep only the gradients
the kernels produced; ``_EpochEval`` - whose outputs the fitter caches - keeps a weak reference, and its ``backward`` raises a
clear error if it needs a fitter (windows weighted differently) that no longer exists."""
import weakref
from collections import Counter

import torch


class _WindowLoss(torch.Tensor):
    """The scalar loss ``forward`` returns.  The reference's driver does ``acc_loss += loss.mean()`` once per window
    (optimize_to_joints.py:156): on a 0-dim tensor ``mean()`` is the identity, but as a torch op it is a kernel launch and an autograd
    node per window, forward and backward - a quarter of the host time of an epoch of the loop at 52 windows.  Here it returns the tensor
    itself (same value, same gradient); every other operation gives a plain ``torch.Tensor`` at plain-tensor cost."""

    __torch_function__ = torch._C._disabled_torch_function_impl

    def mean(self, *args, **kwargs):
        return self


class _FitWindow(torch.autograd.Function):
    """(loss, objs) of one window; gradients were computed by the kernels in forward."""

    @staticmethod
    def forward(ctx, fitter, frames, weights, w_temp, betas, log_beta_scales, betas_trans, pose, trans, fov):
        objs, grads = fitter._loss_and_grads(frames, weights, w_temp)
        ctx.grads = grads
        total = objs[:9].sum()
        return total.as_subclass(_WindowLoss), objs.clone()

    @staticmethod
    def backward(ctx, g_total, _g_objs):
        g = ctx.grads
        s = lambda t: None if t is None else t * g_total  # noqa: E731
        return (None, None, None, None, s(g["betas"]), s(g["log_beta_scales"]), s(g["betas_trans"]), s(g["pose"]), s(g["trans"]), s(g["fov"]))


class _TemporalTerm(torch.autograd.Function):
    """(joint, global, translation) temporal terms; rows of the pose gradient belong to exactly one of them."""

    @staticmethod
    def forward(ctx, fitter, w_temp, pose, trans):
        objs, grads = fitter._loss_and_grads(None, [0.0] * 6, w_temp, window=None)
        ctx.grads = grads
        return objs[6].clone(), objs[7].clone(), objs[8].clone()

    @staticmethod
    def backward(ctx, g_joint, g_global, g_trans):
        g = ctx.grads
        d_pose = torch.cat([g["pose"][:, :1] * g_global, g["pose"][:, 1:] * g_joint], dim=1)
        return None, None, d_pose, g["trans"] * g_trans


class _EpochEval(torch.autograd.Function):
    """Every window of an epoch in ONE evaluation: one loss scalar per window + the terms (windows, 6).  The per-window ``forward``
    calls of the reference's driver hand these out; autograd brings every window's upstream gradient to ONE backward per epoch (each
    window is an output of this node: no select / scatter nodes in between).  With the same upstream gradient on every window (the
    driver adds the window losses with weight 1) the whole-batch gradients are the answer; windows whose upstream gradient differs
    (left out, weighted differently) are handled exactly - see ``backward``."""

    @staticmethod
    def forward(ctx, fitter, weights, window, betas, log_beta_scales, betas_trans, pose, trans, fov):
        _, grads = fitter._loss_and_grads(None, weights, 0.0, window=window, window_terms=True)
        objs_win = grads.pop("_objs_win")
        ctx.fitter, ctx.weights, ctx.window, ctx.grads = weakref.ref(fitter), weights, window, grads
        ctx.layout = (fitter.num_images, fitter.views, fitter._cache.block.shared)
        ctx.key = epoch_key(fitter, tuple(weights))
        ctx.set_materialize_grads(False)  # (a window nobody used arrives as None, not as a zero tensor)
        ctx.mark_non_differentiable(objs_win)
        return (*(t_.as_subclass(_WindowLoss) for t_ in objs_win.sum(1).unbind(0)), objs_win)

    @staticmethod
    def backward(ctx, *upstream):
        # sum_j g_j G_j.  Rows of per-frame parameters belong to one window each: they are scaled by their window's upstream value
        # (exact, also for a window left out: its rows are exactly zero).  Shared parameters (betas, a shared fov or scale table):
        # c G_total + sum_{g_j != c} (g_j - c) G_j with c the most frequent upstream value - nothing to correct in the driver's loop,
        # one direct evaluation per deviating window otherwise (the window an epoch's first call evaluated on its own, ...).
        W, (N, views, in_block) = ctx.window, ctx.layout
        g_win = upstream[:-1]
        used = [t for t in g_win if t is not None]
        if not used:
            return (None,) * 9
        it = iter(torch.stack(used).tolist())  # (the one host sync of an epoch's backward)
        vals = [0.0 if t is None else next(it) for t in g_win]
        c = Counter(vals).most_common(1)[0][0]
        deviating = [(j, gj) for j, gj in enumerate(vals) if gj != c]
        if deviating:
            g_losses = torch.tensor(vals, dtype=torch.float32, device=used[0].device)
            per_row = lambda t, rep: t * g_losses.repeat_interleave(rep)[:t.shape[0]].reshape((-1,) + (1,) * (t.dim() - 1))  # noqa: E731
        out, shared = {}, []
        for k, v in ctx.grads.items():
            if v is None:
                out[k] = None
            elif not deviating:
                out[k] = v if c == 1.0 else v * c
            elif k not in in_block:
                out[k] = per_row(v, W * views if k == "fov" else W)
            else:
                out[k] = v * c
                shared.append(k)
        if deviating and shared:
            f = ctx.fitter()
            if f is None:
                raise RuntimeError("SMALFitter: backward() through differently weighted window losses after their fitter was deleted")
            if epoch_key(f, tuple(ctx.weights)) != ctx.key:
                raise RuntimeError("SMALFitter: backward() through window losses after the parameters, targets or cameras they were "
                                   "evaluated with have changed")
            for j, gj in deviating:
                _, gw = f._loss_and_grads(list(range(j * W, min(N, (j + 1) * W))), ctx.weights, 0.0)
                for k in shared:
                    out[k] = out[k] + gw[k] * (gj - c)
        return (None, None, None, out["betas"], out["log_beta_scales"], out["betas_trans"], out["pose"], out["trans"], out["fov"])


PARAM_NAMES = ("betas", "log_beta_scales", "betas_trans", "global_rotation", "joint_rotations", "trans", "fov")
# ---- fingerprint parts: each spelled once ----------------------------------------------------------------------------
versioned = lambda t: None if t is None else (t.data_ptr(), t._version)  # noqa: E731  (same buffer, not edited in place)
addressed = lambda t: None if t is None else (t.data_ptr(), tuple(t.shape))  # noqa: E731  (what a captured launch bakes in)
weights_part = lambda weights: tuple(float(w) for w in weights)  # noqa: E731
masks_part = lambda f: versioned(f.global_mask) + versioned(f.rotation_mask)  # noqa: E731
cameras_part = lambda renderer, stamp: (stamp(renderer.cameras.R), stamp(renderer.cameras.T), stamp(renderer.cameras.aspect_ratio),  # noqa: E731
                                        stamp(getattr(renderer.cameras, "principal_point", None)))
raster_part = lambda renderer: bytes(renderer.raster_settings)  # noqa: E731  (the whole struct: blur, sigma, K, clipping plane, tie rule)


def params_part(f, versions: bool):
    """Which parameters train; ``versions``: also their identity and in-place version counter (``optimizer.step()`` bumps it)."""
    P = f._parameters
    if versions:
        return tuple([(id(p), p._version, p.requires_grad) for p in [P[n] for n in PARAM_NAMES]])
    return tuple([P[n].requires_grad for n in PARAM_NAMES])


def targets_part(f):
    """(identity, in-place version) of every target tensor: the reference driver edits ``target_visibility`` in place
    (optimize_to_joints.py:135-138), which no attribute hook can see; torch's version counter can."""
    tv, tj, si = f.target_visibility, f.target_joints, f.sil_imgs
    return (id(tv), tv._version, id(tj), tj._version, id(si), None if si is None else si._version, tuple(f.config.CANONICAL_MODEL_JOINTS))


def epoch_key(f, wts):
    """Everything a cached epoch depends on: the parameters (identity + in-place version counter: ``optimizer.step()`` and
    ``param[...] = x`` bump it), which of them train, loss weights, targets, masks, cameras and rasteriser settings.  Edits that
    bypass the counter (``param.data[...] = x``) need ``invalidate_epoch()``.  (Called once per ``forward``: plain attribute reads.)"""
    rend = f.renderer
    return (wts, params_part(f, True), targets_part(f), masks_part(f), cameras_part(rend, versioned), raster_part(rend),
            f.propagate_scaling, f.rgb_only, torch.is_grad_enabled())  # (an evaluation under no_grad carries no graph)


# attribute of the fitter -> the reason its re-assignment invalidates with
INVALIDATED_BY = dict(target_visibility="targets", target_joints="targets", sil_imgs="targets", global_mask="tables",
                      rotation_mask="tables", renderer="tables", propagate_scaling="tables")


class FitState:
    """Everything a ``SMALFitter`` caches, in one plain object (``fitter._cache``; plain, so that writes do not pass through
    ``nn.Module.__setattr__``): each item is declared here with what it depends on, ``invalidate(reason)`` is the one way any of
    it is dropped, ``serve`` answers a ``forward`` from the cached epoch."""

    def __init__(self):
        # device copies of the targets; depend on the target tensors and CANONICAL_MODEL_JOINTS (``targets_part``, stored in
        # ``target_signature`` at upload) and on ``targets_dirty`` (edits no version counter sees: ``invalidate_targets``)
        self.sil = self.sil_sum = self.tj = self.vis = self.canon = self.target_signature = None
        self.canon_identity, self.targets_dirty = False, True
        self.mask = None  # (masks_part, (J,3) table): address and in-place version of global_mask / rotation_mask
        self.pix_scale = None  # (key, per-image silhouette weight): loss weight and window layout (``SMALFitter._pix_scale``)
        self.block = None  # fit_eval.SharedBlock of the most recent evaluation (what ranks sum; which gradients live in it)
        self.clip_depth = None  # engine.ClipDepth of the most recent silhouette launch (``straddling_faces`` reads its counters)
        self.warned_straddling = False  # the clipping-plane warning is given once per fitter
        self.epoch = None  # dict(key, losses, objs_win, served) of the cached epoch: everything in ``epoch_key``
        self.win_lists = None  # ((N, W), the windows of an epoch as lists): frames held and window size
        self.graph = None  # the captured iteration (fit_graph.capture): everything in ``graph_key``, and the stage
        self.adam, self.adam_step, self.adam_hyper = {}, 0, None  # per-parameter moments / steps taken / hyper-parameters of the stage
        self.adam_t = None  # device mirror of ``adam_step`` that a captured iteration increments
        self.halo_buf = None  # (prev, next) persistent rows the first graph of a multi-rank step reads

    def invalidate(self, reason: str) -> None:
        """``"targets"``: a target tensor was replaced or edited (re-upload, cached epoch dropped).  ``"tables"``: masks, cameras,
        renderer or ``propagate_scaling`` replaced (the captured iteration holds the old addresses; cached epoch dropped).
        ``"stage"``: new optimiser stage (new Adam state, the captured iteration belongs to the old one).  ``"parameters"``:
        parameters written through ``.data``, where no version counter moves (cached epoch dropped)."""
        assert reason in ("targets", "tables", "stage", "parameters"), reason
        if reason in ("tables", "stage"):
            self.graph = None
        if reason == "stage":
            self.adam, self.adam_step = {}, 0
        else:
            self.epoch = None
            self.targets_dirty |= reason == "targets"

    def serve(self, f, batch_range, wts):
        """``(loss, terms)`` of the window ``batch_range`` from the cached epoch, or None when this call has to be evaluated on its own.
        Policy: the first window requested under a new parameter state is evaluated directly (a caller that only ever asks for one
        window per state - stochastic mini-batches - never pays for a whole batch); the second one switches the epoch to the
        whole-batch evaluation, and once an epoch has been served that way the next one starts with it at its first window."""
        W = int(f.batch_size) if f.batch_size else 0
        N = f.num_images
        n = len(batch_range)
        if not f.epoch_cache or W <= 0 or n == 0 or N <= W:
            return None
        j0 = int(batch_range[0])
        if j0 % W or n != min(W, N - j0) or f.frame0 % W:
            return None
        wl = self.win_lists
        if wl is None or wl[0] != (N, W):
            wl = self.win_lists = ((N, W), [list(range(j, min(N, j + W))) for j in range(0, N, W)])
        if (batch_range if type(batch_range) is list else [int(b) for b in batch_range]) != wl[1][j0 // W]:
            return None
        key = epoch_key(f, wts)
        ep = self.epoch
        if ep is None or ep["key"] != key:
            eager = ep is not None and ep["losses"] is not None  # the last state saw a second window: it was served from one evaluation
            ep = self.epoch = dict(key=key, losses=None, objs_win=None, served=0)
            if not eager:
                return None
        if ep["losses"] is None:  # second window of this state (or an eager first one): evaluate them all now
            out = _EpochEval.apply(f, list(wts), W, f.betas, f.log_beta_scales, f.betas_trans, f._pose_leaf(), f.trans, f.fov)
            ep["losses"], ep["objs_win"] = out[:-1], out[-1]
        ep["served"] += 1
        return ep["losses"][j0 // W], ep["objs_win"][j0 // W]  # (a tuple of scalars: no autograd node per window)
