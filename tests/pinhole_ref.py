"""TEST INFRASTRUCTURE ONLY.  float64 reference of cameras with a principal point (pytorch3d's ``PerspectiveCameras`` in NDC):
``oracle.render_ref.project_to_ndc`` evaluated in float64, the shift ``x_ndc + px``, ``y_ndc + py`` added, then the oracle's screen
transform and its ``SoftSilhouette``.  The oracle itself is used as it is.

Tables (R, T, fov, aspect, principal) with k rows are indexed ``image % k`` like the library's; ``rows`` expands one to N images.
"""
import numpy as np
import torch

from oracle import render_ref


def rows(table, N):
    """(k, ...) -> (N, ...), image n takes row n % k; None stays None."""
    if table is None:
        return None
    table = torch.as_tensor(table)
    return table[torch.arange(N) % table.shape[0]]


def project_to_ndc(points, R, T, fov_deg, aspect=None, principal=None):
    """points (N,P,3) world, one table row per image -> (x_ndc + px, y_ndc + py, z_view), float64, differentiable in points and fov."""
    d = lambda t: None if t is None else torch.as_tensor(t).double()  # noqa: E731
    ndc = render_ref.project_to_ndc(d(points), d(R), d(T), d(fov_deg), d(aspect))
    if principal is None:
        return ndc
    pp = d(principal).reshape(-1, 2)
    return torch.cat([ndc[..., :2] + pp[:, None, :], ndc[..., 2:]], dim=-1)


def ndc_to_screen(ndc, S):
    """(y_s, x_s) pixels, x_s = S/2 - (S/2) x_ndc: the screen transform does not know about the principal point."""
    return torch.stack([S / 2.0 - (S / 2.0) * ndc[..., 1], S / 2.0 - (S / 2.0) * ndc[..., 0]], dim=-1)


def project_points_screen(points, R, T, fov_deg, S, aspect=None, principal=None):
    return ndc_to_screen(project_to_ndc(points, R, T, fov_deg, aspect, principal), S)


def render_silhouette(verts, faces, R, T, fov_deg, S, aspect=None, principal=None):
    """verts (N,V,3), one camera per image -> (N,1,S,S) soft silhouette (float32, as the oracle's rasteriser takes and gives it)."""
    ndc = project_to_ndc(verts, R, T, fov_deg, aspect, principal).float()
    return render_ref.SoftSilhouette.apply(ndc, faces.to(torch.int32), S, render_ref.BLUR_RADIUS, render_ref.SIGMA, render_ref.FACES_PER_PIXEL)[:, None]


class PinholeRenderer:
    """Callable like ``render_ref.OracleRenderer`` (``fitter_ref.fit_losses(renderer=)`` takes one), with a principal-point table;
    every table is expanded to the batch by ``rows``."""

    def __init__(self, image_size, R, T, fov, aspect=None, principal=None):
        self.image_size, self.R, self.T, self.fov, self.aspect, self.principal = image_size, R, T, fov, aspect, principal

    def __call__(self, vertices, points, faces, joints_only=False):
        n = vertices.shape[0]
        tab = [rows(t, n) for t in (self.R, self.T, self.fov.reshape(-1), None if self.aspect is None else self.aspect.reshape(-1), self.principal)]
        proj = project_points_screen(points, tab[0], tab[1], tab[2], self.image_size, tab[3], tab[4]).to(points.dtype)
        if joints_only:
            return None, proj
        f = faces[0] if faces.dim() == 3 else faces
        return render_silhouette(vertices, f, tab[0], tab[1], tab[2], self.image_size, tab[3], tab[4]), proj


def pinhole_pixels(X, R_cv, t_cv, K):
    """(u, v) of the OpenCV pinhole model u = fx x / z + cx, v = fy y / z + cy, float64."""
    Xc = np.asarray(X, np.float64) @ np.asarray(R_cv, np.float64).T + np.asarray(t_cv, np.float64)
    return K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]
