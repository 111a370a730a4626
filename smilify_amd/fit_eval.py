"""The fused evaluation behind ``SMALFitter._loss_and_grads``, as named steps.  Every arithmetic step is a HIP kernel of
``libsmilfit.so``; this module only selects rows and hands out buffers."""
import torch

from . import engine
from ._lib import N_OBJS


class SharedBlock:
    """Everything the kernels ADD into, in one buffer with one zero fill: ``[10 loss terms | d_betas | d_fov | shared scale-table
    gradients | per-image fov sums]``.  All that ranks have to SUM sits in one contiguous ``tensor`` at the front; the fov gradient
    is in it when fov is shared (a per-image fov belongs to its rank), a scale table's when the table is shared and trains.
    ``shared`` names the parameters whose gradient lives in the block."""

    def __init__(self, f, ls_shared: bool, bt_shared: bool, n_img: int):
        J, nB = f.device_model.J, f.device_model.nB
        n_fov = f.fov.numel() if f.fov.numel() in (1, f.views) else 0
        n_ls = 3 * J if (ls_shared and f.log_beta_scales.requires_grad) else 0
        n_bt = 3 * J if (bt_shared and f.betas_trans.requires_grad) else 0
        o_fov, o_ls, o_bt, n_shared = N_OBJS + nB, N_OBJS + nB + n_fov, N_OBJS + nB + n_fov + n_ls, N_OBJS + nB + n_fov + n_ls + n_bt
        a = torch.zeros(n_shared + n_img, dtype=torch.float32, device=f.device)
        self.tensor, self.objs, self.d_betas, self.d_fov_img = a[:n_shared], a[:N_OBJS], a[N_OBJS:o_fov], a[n_shared:]
        self.d_fov, self.d_ls, self.d_bt = a[o_fov:o_ls], a[o_ls:o_bt].view(n_ls // 3, 3), a[o_bt:n_shared].view(n_bt // 3, 3)  # (empty when not in the block)
        self.shared = frozenset(n for n, k in (("betas", 1), ("fov", n_fov), ("log_beta_scales", n_ls), ("betas_trans", n_bt)) if k)


class Evaluation:
    """One evaluation: the steps run in launch order and leave what later steps read on the object.  ``frames`` / ``images`` / ``table`` /
    ``camera`` / ``scatter`` are the one index-select-or-pass-through rule (``idx`` None = all frames of this rank) for everything stored per
    frame, per image, as a shared-or-per-frame table or as a camera table, and the way back to full-size gradients."""

    def __init__(self, f, frames, weights, w_temp, window):
        """Frame selection, the selected parameter rows, the kernels' configuration, the shared block, the cameras."""
        self.f, dm, dev = f, f.device_model, f.device
        if frames is None:
            self.idx, self.n, frame0, n_total = None, f.num_images, f.frame0, f.n_frames_total
        else:  # (a window has no temporal term; get_temporal covers the sequence)
            fl = list(frames)
            self.idx, self.n, frame0, n_total, w_temp = torch.tensor(fl, dtype=torch.long, device=dev), len(fl), 0, len(fl), 0.0
        w, n = [float(x) for x in weights], self.n
        w[1] = 0.0 if f.rgb_only else w[1]
        self.w_j2d, self.w_reproj = w[0], w[1]  # (they decide which kernels run)
        self.pose, self.trans = self.frames(f._pose.detach()).contiguous(), self.frames(f.trans.detach()).contiguous()
        self.mask = f._mask_table()
        (self.ls, self.ls_shared), (self.bt, self.bt_shared) = self.table(f.log_beta_scales), self.table(f.betas_trans)
        self.betas = f.betas.detach().contiguous()
        self.fc = engine.fit_config(n, dm.J, dm.nB, window if window is not None else n_total, w, w_temp, frame0, n_total, f.config.JOINT_LIMIT,
                                    f.global_rotation.requires_grad, f.joint_rotations.requires_grad, f.trans.requires_grad)
        self.blk = f._cache.block = SharedBlock(f, self.ls_shared, self.bt_shared, n * f.views)
        # cameras: one table row per view, per image or shared; fov may be the trainable parameter.  The image rows of ``idx`` are
        # computed HERE, behind the parameter selects and the block's zero fill: ``images`` / ``camera`` need them, and the order of the
        # launches is part of what a captured iteration and the kernel traces pin - do not move this to the top
        cam, fov = f.renderer.cameras, f.fov.detach().reshape(-1).contiguous()
        self.img_idx = None if self.idx is None else (self.idx[:, None] * f.views + torch.arange(f.views, device=dev)[None]).reshape(-1)
        pp = f.renderer._principal()
        self.cams = engine.CameraSet(self.camera(cam.R), self.camera(cam.T), self.camera(fov),
                                     None if cam.aspect_ratio is None else self.camera(cam.aspect_ratio.reshape(-1)), f.views, f.image_size,
                                     None if pp is None else self.camera(pp))
        self.lbs = self.g_lbs = self.d_fov_sel = self.yx = self.tj = self.vis = self.d_yx = self.d_ndc = self.d_ndc_scale = None
        self.loss_img = self.pscale = self.cd = None  # (all of these stay None when no term needs the mesh)

    def frames(self, t):
        return t if self.idx is None else t.index_select(0, self.idx)

    def images(self, t):
        return (t if self.idx is None else t.index_select(0, self.img_idx)).contiguous()

    def table(self, p: torch.Tensor):
        """(tensor, shared?) for a parameter that is either one shared row or one row per frame."""
        if p.shape[0] == 1:
            return p.detach()[0].contiguous(), True
        if p.shape[0] != self.f.num_images:
            raise ValueError(f"parameter with {p.shape[0]} rows for {self.f.num_images} frames")
        return self.frames(p.detach()).contiguous(), False

    def camera(self, t):
        """Only per-image camera tables follow the selection."""
        k, n_img = t.shape[0], self.f.num_images * self.f.views
        if k in (1, self.f.views) or self.idx is None:
            return t.contiguous()
        if k != n_img:
            raise ValueError(f"camera table with {k} rows for {n_img} images")
        return self.images(t)

    def scatter(self, rows, like):
        return rows if self.idx is None else torch.zeros_like(like).index_copy_(0, self.idx, rows)

    def run(self, halo_prev, halo_next, halo, window_terms):
        if self.w_j2d > 0 or self.w_reproj > 0:
            self.forward_and_losses()
            self.backward_to_world()
        return self.blk.objs, self.epilogue_and_grads(halo_prev, halo_next, halo, window_terms)

    def forward_and_losses(self):
        """Skinning + projection, then the joint loss and the fused silhouette loss with their image-plane gradients."""
        f, cams, w_j2d, w_reproj = self.f, self.cams, self.w_j2d, self.w_reproj
        c, dm, views, S = f._cache, f.device_model, f.views, f.image_size
        # the rotation masks are applied inside the pose kernels (theta_mask): no masked copy of the pose
        lbs = self.lbs = engine.lbs_forward(dm, self.betas, self.pose, trans=self.trans, logscale=self.ls, btrans=self.bt, shared_beta=True,
                                            logscale_shared=self.ls_shared, btrans_shared=self.bt_shared, propagate_scaling=f.propagate_scaling,
                                            allow_limb_scaling=f.config.ALLOW_LIMB_SCALING, trans_after_joints=True, theta_mask=self.mask,
                                            project=dict(cams=cams, ndc=w_reproj > 0, yx=w_j2d > 0) if engine.FUSED_LBS_FORWARD else None)
        ndc = None
        if engine.FUSED_LBS_FORWARD:  # projected by the skinning kernel (vertices -> NDC, joints -> pixels)
            ndc, self.yx = lbs.get("ndc"), lbs.get("yx")
        elif w_j2d > 0 and w_reproj > 0:  # vertices -> NDC and joints -> pixels in one launch
            ndc, self.yx = engine.project_verts_and_joints(cams, lbs["verts"], lbs["joints"])
        elif w_j2d > 0:
            _, self.yx = engine.project(cams, lbs["joints"], want_ndc=False)
        else:
            ndc, _ = engine.project(cams, lbs["verts"], want_yx=False)
        if w_j2d > 0:
            self.tj, self.vis, self.d_yx = self.images(c.tj), self.images(c.vis), torch.empty_like(self.yx)
            engine.joint_loss(self.fc, views, c.canon.numel(), None if c.canon_identity else c.canon, self.yx, self.tj, self.vis, self.blk.objs, self.d_yx)
        if w_reproj > 0:
            tgt, tsum = self.images(c.sil), self.images(c.sil_sum)
            self.pscale = f._pix_scale(self.fc, views, S)
            # (the vertex gradient stays as the tile kernel accumulated it: the projection backward decodes it while it reads; the depth
            # gradients of edges cut at the clipping plane travel beside d_ndc in persistent buffers: a captured iteration replays the pointers)
            self.cd = c.clip_depth = engine.clip_depth_for(dm, self.n * views)
            self.loss_img, self.d_ndc, _, self.d_ndc_scale = engine.silhouette_l1_fused(dm, ndc, S, tgt, tsum, self.pscale, f.renderer.raster_settings,
                                                                                        packed_out=True, clip_depth=self.cd)

    def backward_to_world(self):
        """Image-plane gradients -> world space and on through the skinning backward: inside it (one kernel per frame, no (B,V,3)
        vertex gradient in memory) where the library offers it, else by the projection backward first."""
        f, cams, blk, lbs, dm = self.f, self.cams, self.blk, self.lbs, self.f.device_model
        d_ndc, d_yx, d_scale, d_fov_img = self.d_ndc, self.d_yx, self.d_ndc_scale, blk.d_fov_img
        ndc_up = d_verts = d_joints = None
        if engine.FUSED_LBS_BACKWARD and engine.lbs_backward_ndc_supported(dm, dm.nB if f.betas.requires_grad else 0, f.views):
            ndc_up = dict(cams=cams, d_ndc=d_ndc, d_ndc_scale=d_scale, d_yx=d_yx, d_fov_img=d_fov_img, clip_depth=self.cd)
        elif d_yx is not None and d_ndc is not None:
            d_verts, d_joints = engine.project_backward_verts_and_joints(cams, lbs["verts"], d_ndc, lbs["joints"], d_yx, d_fov_img, d_ndc_scale=d_scale)
        elif d_yx is not None:
            d_joints, _ = engine.project_backward(cams, lbs["joints"], d_yx=d_yx, d_fov_img=d_fov_img)
        else:
            d_verts, _ = engine.project_backward(cams, lbs["verts"], d_ndc=d_ndc, d_fov_img=d_fov_img, d_ndc_scale=d_scale)
        if d_verts is not None and d_ndc is not None and self.cd is not None:
            engine.clip_depth_backward(cams, self.cd, d_verts)
        n_fov = cams.fov.numel()  # (the epilogue reduces the per-image fov sums into d_fov_sel: the block's slot when the sizes agree)
        self.d_fov_sel = blk.d_fov if blk.d_fov.numel() == n_fov else torch.empty(n_fov, dtype=torch.float32, device=f.device)
        # (the shared shape gradient is added straight into d_betas, as the shape prior's; shared scale tables' gradients land in their slots)
        self.g_lbs = engine.lbs_backward(dm, lbs, d_verts, d_joints, need_beta=f.betas.requires_grad, need_logscale=f.log_beta_scales.requires_grad,
                                         need_btrans=f.betas_trans.requires_grad, need_trans=f.trans.requires_grad, d_beta_accum=blk.d_betas,
                                         out_logscale=blk.d_ls if blk.d_ls.numel() else None, out_btrans=blk.d_bt if blk.d_bt.numel() else None,
                                         ndc_upstream=ndc_up)

    def epilogue_and_grads(self, halo_prev, halo_next, halo, window_terms: bool):
        """Priors + temporal terms + silhouette objective + fov reduction in one launch (a pending halo is waited for right in front of
        it, the only reader of the rows), every window's own six terms if asked for, then the full-size gradient of every parameter
        (zero rows outside the selection, None for parameters that do not train)."""
        f, blk, g, fov_sel, dev = self.f, self.blk, self.g_lbs, self.d_fov_sel, self.f.device
        c, J = f._cache, f.device_model.J
        accumulate = g is not None and g["d_theta"] is not None
        d_pose = g["d_theta"] if accumulate else torch.empty(self.n, J, 3, dtype=torch.float32, device=dev)
        d_trans = g["d_trans"] if accumulate and g["d_trans"] is not None else torch.zeros(self.n, 3, dtype=torch.float32, device=dev)
        if halo is not None:  # an ``optimize.PendingHalo``: the messages travelled while skinning and rasteriser ran
            halo_prev, halo_next = halo.wait()
        engine.fit_epilogue(self.fc, self.pose, self.trans, self.betas, f.mean_betas, f.betas_prec, self.mask, blk.objs, d_pose, d_trans, blk.d_betas,
                            halo_prev=halo_prev, halo_next=halo_next, accumulate=accumulate, loss_img=self.loss_img, pix_scale=self.pscale,
                            cams=self.cams if fov_sel is not None else None, d_fov_img=blk.d_fov_img if fov_sel is not None else None, d_fov=fov_sel)
        objs_win = None
        if window_terms:  # (the drop-in forward() serves the windows of an epoch from one evaluation)
            objs_win = engine.window_terms(self.fc, f.views, c.canon.numel(), None if c.canon_identity else c.canon, self.yx if self.w_j2d > 0 else None,
                                           self.tj, self.vis, self.pose, self.mask, blk.objs, self.loss_img, self.pscale)
        if fov_sel is not None and (f.fov.numel() in (1, f.views) or self.idx is None):
            d_fov = fov_sel
        else:
            d_fov = blk.d_fov if blk.d_fov.numel() else torch.zeros_like(f.fov.detach().reshape(-1))
            if fov_sel is not None:  # per-image fov, window of frames: scatter the selected images' gradients
                d_fov.index_add_(0, self.img_idx, fov_sel)

        def table_grad(p, key, shared, slot):
            if not p.requires_grad:
                return None
            if g is None or g[key] is None:  # (a shared table keeps its - zero - slot of the shared block)
                return slot.view(p.shape) if slot.numel() else torch.zeros_like(p)
            return g[key].reshape(p.shape) if shared else self.scatter(g[key], p)

        grads = dict(betas=blk.d_betas if f.betas.requires_grad else None, pose=self.scatter(d_pose, f._pose), trans=self.scatter(d_trans, f.trans),
                     log_beta_scales=table_grad(f.log_beta_scales, "d_logscale", self.ls_shared, blk.d_ls),
                     betas_trans=table_grad(f.betas_trans, "d_btrans", self.bt_shared, blk.d_bt), fov=d_fov.reshape(f.fov.shape) if f.fov.requires_grad else None)
        if objs_win is not None:
            grads["_objs_win"] = objs_win
        return grads
