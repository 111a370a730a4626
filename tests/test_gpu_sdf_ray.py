"""The spatial-diameter ray cast on the GPU (csrc/raycast.hip, smilify_amd/sdf.py) against the float64 restatement
(tests/sdf_ray_ref.py): hand meshes on which float32 is exact, the shapes at which the kernel takes another path, real meshes with
the rays a float32 evaluation may decide differently set aside, the two K-nearest steps, and the tool end to end."""
import os

import numpy as np
import pytest
import torch

import sdf_ray_ref as R
from conftest import GOLDEN, MODEL_FILES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = R.U
TILE, SPLIT = 256, 1024  # faces per LDS tile; a face range is split from 2 * SPLIT faces on when the rays leave the GPU idle


def gpu_cast(v, f, o, own, d, t_min, d_lo, d_hi, cap, want_ray_t=True):
    from smilify_amd import engine

    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dt)).to(DEV)  # noqa: E731
    diam, ray_t = engine.ray_diameters(t(v, np.float32), t(f, np.int32), t(o, np.float32), t(own, np.int32), t(d, np.float32), float(t_min),
                                       float(d_lo), float(d_hi), int(cap), want_ray_t=want_ray_t)
    return diam.cpu().numpy(), None if ray_t is None else ray_t.cpu().numpy()


def exact(v, f, o, own, d, t_min, d_lo, d_hi, cap):
    """Both outputs equal the float64 reference bit for bit (whose values are float32 numbers); returns (diam, ray_t)."""
    c = R.cast(v, f, o, own, d, t_min)
    want_d = R.diameters(c["t"], d_lo, d_hi, cap)
    assert np.array_equal(c["t"].astype(np.float32).astype(np.float64), c["t"]), "the case is not exact in float32"
    diam, ray_t = gpu_cast(v, f, o, own, d, t_min, d_lo, d_hi, cap)
    assert np.array_equal(ray_t, c["t"].astype(np.float32)), (ray_t, c["t"])
    assert np.array_equal(diam, want_d.astype(np.float32)), (diam, want_d)
    return diam, ray_t, c


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
NESTED = R.merge(R.box(-4.0, 4.0), R.box(-1.0, 1.0))


def test_exact_largest_hit_of_nested_boxes():
    o = np.array([[0.25, 0.5, -0.25], [0.0, 0.0, 0.0]])
    d = np.stack([AXES, AXES * np.array([2.0, 0.5, 4.0, 1.0, 0.25, 8.0])[:, None]])  # (not normalised: t scales with 1 / |d|)
    diam, ray_t, _ = exact(*NESTED, o, [-1, -1], d, 2.0 ** -10, 0.0, 100.0, 100)
    assert ray_t[0].tolist() == [3.75, 4.25, 3.5, 4.5, 4.25, 3.75]  # the outer box, not the inner one at 0.75 ..
    # sample 1: every ray runs through the middle of a side, which lies on the diagonal shared by the side's two triangles
    assert ray_t[1].tolist() == [2.0, 8.0, 1.0, 4.0, 16.0, 0.5]
    assert diam[0] == np.float32(np.mean([3.75, 4.25, 3.5, 4.5, 4.25, 3.75]))
    # the inner box alone from the same origins: 0.75 .. (nearest = largest: one hit per ray)
    _, inner, _ = exact(*R.box(-1.0, 1.0), o[:1], [-1], d[:1], 2.0 ** -10, 0.0, 100.0, 100)
    assert inner[0].tolist() == [0.75, 1.25, 0.5, 1.5, 1.25, 0.75]


def test_exact_edge_vertex_and_parallel_faces():
    """A ray along an edge of a box: it enters and leaves through corner vertices (u = v = 0, u = 1, v = 1 are inclusive) and runs
    inside the planes of two sides (a = 0: never hit)."""
    v, f = R.box(2.0, 4.0)
    o = np.array([[0.0, 2.0, 2.0], [0.0, 3.0, 2.0], [0.0, 3.0, 3.0]])  # through a corner, through the middle of an edge, through a side's diagonal
    d = np.broadcast_to(np.array([[1.0, 0, 0], [-1.0, 0, 0]]), (3, 2, 3))
    _, ray_t, _ = exact(v, f, o, [-1, -1, -1], d, 2.0 ** -10, 0.0, 100.0, 100)
    assert ray_t.tolist() == [[4.0, -1.0]] * 3


def test_exact_t_min_and_own_face():
    v, f = NESTED
    o = np.array([[1.0 - 2.0 ** -10, 0.25, 0.5]])  # 2^-10 inside the inner box's side x = 1
    d = AXES[None, :2]
    _, at, _ = exact(v, f, o, [-1], d, 2.0 ** -10, 0.0, 100.0, 100)   # t > t_min is strict: the inner side is not hit, the outer is
    _, below, c = exact(v, f, o, [-1], d, 2.0 ** -11, 0.0, 100.0, 100)
    assert at.tolist() == below.tolist() == [[3.0 + 2.0 ** -10, 5.0 - 2.0 ** -10]]
    inner = R.box(-1.0, 1.0)
    _, at, _ = exact(*inner, o, [-1], d, 2.0 ** -10, 0.0, 100.0, 100)
    _, below, ci = exact(*inner, o, [-1], d, 2.0 ** -11, 0.0, 100.0, 100)
    assert at.tolist() == [[-1.0, 2.0 - 2.0 ** -10]] and below.tolist() == [[2.0 ** -10, 2.0 - 2.0 ** -10]]
    # the sample's own face is never hit: without the outer face the ray falls back to the inner box
    own = int(c["face"][0, 0])
    _, without, _ = exact(v, f, o, [own], d, 2.0 ** -11, 0.0, 100.0, 100)
    assert without.tolist() == [[2.0 ** -10, 5.0 - 2.0 ** -10]]
    _, without, _ = exact(*inner, o, [int(ci["face"][0, 0])], d, 2.0 ** -11, 0.0, 100.0, 100)
    assert without.tolist() == [[-1.0, 2.0 - 2.0 ** -10]]


def test_exact_single_triangle_and_small_a():
    s = 2.0 ** -10  # a = |d| s^2: 2^-20 = 9.5e-7 is below 1e-6, 2^-19 above
    v = np.array([[0, 0, 0], [s, 0, 0], [0, s, 0]], np.float64)
    f = np.array([[0, 1, 2]])
    o = np.array([[s / 4, s / 4, 1.0], [s / 4, s / 4, -1.0]])
    d = np.array([[[0, 0, -1.0], [0, 0, -2.0], [0, 0, 1.0]], [[0, 0, 1.0], [0, 0, 2.0], [0, 0, -2.0]]])
    diam, ray_t, _ = exact(v, f, o, [-1, -1], d, 2.0 ** -10, 0.25, 100.0, 100)
    assert ray_t.tolist() == [[-1.0, 0.5, -1.0], [-1.0, 0.5, -1.0]] and diam.tolist() == [0.5, 0.5]
    diam, ray_t, _ = exact(v, f, o, [0, 0], d, 2.0 ** -10, 0.25, 100.0, 100)  # the only face is the sample's own: d_lo
    assert (ray_t == -1.0).all() and diam.tolist() == [0.25, 0.25]


def test_exact_thresholds_and_cap():
    o = np.array([[0.0, 0.5, 0.25]])  # to the outer box: 4, 4, 3.5, 4.5, 3.75, 4.25
    args = (*NESTED, o, [-1], AXES[None])
    diam, ray_t, _ = exact(*args, 2.0 ** -10, 3.5, 4.25, 100)  # d_lo and d_hi are excluded at equality
    assert ray_t.tolist() == [[4.0, 4.0, 3.5, 4.5, 3.75, 4.25]] and diam[0] == np.float32(11.75 / 3)
    for cap, want in ((1, 4.0), (2, 4.0), (3, 11.75 / 3), (6, 11.75 / 3), (7, 11.75 / 3)):
        assert exact(*args, 2.0 ** -10, 3.5, 4.25, cap)[0][0] == np.float32(want)
    assert exact(*args, 2.0 ** -10, 3.0, 4.125, 3)[0][0] == np.float32((4.0 + 4.0 + 3.5) / 3)  # in ray order, not by size
    assert exact(*args, 2.0 ** -10, 5.0, 6.0, 3)[0][0] == np.float32(5.0)                       # hits, none valid: d_lo


def soup(F, seed):
    """F random triangles of edge ~0.4 in the unit cube (float32)."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(0, 1, (F, 1, 3))
    v = (c + rng.uniform(-0.2, 0.2, (F, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * F).reshape(F, 3)


def compare(name, v, f, o, own, d, t_min, d_lo, d_hi, diag, cap, ref=None, max_amb_rays=None, max_amb_samples=None):
    """One GPU call against float64: every non-ambiguous ray agrees in hit / no hit and within its bound; the diameters of samples
    without an ambiguous ray agree within 8 * 2^-24 relative; the outputs do not depend on ray_t being asked for, and a second call
    returns the same bits."""
    c = ref["cast"] if ref else R.cast(v, f, o, own, d, t_min, d_lo, d_hi, diag)
    want = ref["diam"] if ref else R.diameters(c["t"], d_lo, d_hi, cap)
    diam, ray_t = gpu_cast(v, f, o, own, d, t_min, d_lo, d_hi, cap)
    diam2, none = gpu_cast(v, f, o, own, d, t_min, d_lo, d_hi, cap, want_ray_t=False)
    diam3, ray_t3 = gpu_cast(v, f, o, own, d, t_min, d_lo, d_hi, cap)
    assert none is None and np.array_equal(diam, diam2) and np.array_equal(diam, diam3) and np.array_equal(ray_t, ray_t3)
    amb = c["ambiguous"]
    clear = ~amb
    err = np.abs(ray_t.astype(np.float64) - c["t"])
    hit = c["t"] >= 0
    rel = np.abs(diam.astype(np.float64) - want) / np.abs(want)
    ok = ~amb.any(1)
    print(f"[sdf-ray] {name}: {int(amb.sum())} of {amb.size} rays ambiguous, {int((~ok).sum())} of {len(ok)} samples hold one; "
          f"hit share {hit.mean():.3f}; max ray error / bound {np.max(err[clear & hit] / c['bound'][clear & hit], initial=0):.3g}; "
          f"max diameter rel err {np.max(rel[ok], initial=0) / U:.2f} x 2^-24; hit decisions that differ among the ambiguous: "
          f"{int(((ray_t >= 0) != hit)[amb].sum())}")
    assert np.array_equal((ray_t >= 0)[clear], hit[clear])
    assert (err[clear & hit] <= c["bound"][clear & hit]).all()
    assert (rel[ok] <= 8 * U).all()
    if max_amb_rays is not None:
        assert amb.sum() <= max_amb_rays * amb.size and (~ok).sum() <= max_amb_samples * len(ok)
    return diam, ray_t, c


@pytest.mark.parametrize("F,S,Rn,cap", [
    (TILE - 1, 63, 1, 1), (TILE, 64, 1, 1), (TILE + 1, 65, 1, 3),                 # either side of the LDS tile, of a wave
    (2 * SPLIT - 1, 255, 1, 1), (2 * SPLIT, 256, 1, 1), (2 * SPLIT + 1, 257, 1, 1),  # of a face-range split, of a workgroup
    (3 * SPLIT + 28, 3, 100, 3),                                                  # three splits, the last one short; R > 64
    (700, 1, 30, 100), (700, 1, 70, 3), (700, 9, 30, 15), (3, 40, 7, 1),
])
def test_shapes(F, S, Rn, cap):
    v, f = soup(F, 100 + F)
    rng = np.random.RandomState(F + S)
    o = rng.uniform(0.2, 0.8, (S, 3)).astype(np.float32)
    d = rng.randn(S, Rn, 3).astype(np.float32)
    own = rng.randint(0, F, S)
    diag, d_lo, d_hi, t_min = R.thresholds(v)
    d_hi = np.float32(2.5 * d_hi)  # (half the diagonal: the soup has no inside, most largest hits are far away)
    _, ray_t, c = compare(f"soup F={F} S={S} R={Rn} cap={cap}", v, f, o, own, d, t_min, d_lo, d_hi, diag, cap)
    assert c["ambiguous"].mean() <= 0.05
    if F > 100 and S * Rn >= 60:  # the winners are spread over the face range: its first and last tile hold some
        won = c["face"][c["face"] >= 0]
        assert won.min() < TILE and won.max() >= F - TILE


@pytest.mark.parametrize("name", ["fixture", "atta", "stick"])
def test_real_meshes(name):
    case = R.condition_case(name)
    compare(name, case["verts"], case["faces"], case["origins"], case["face_idx"], case["dirs"], case["t_min"], case["d_lo"], case["d_hi"],
            case["diag"], case["cap"], ref=case, max_amb_rays=0.01, max_amb_samples=0.10)


@pytest.mark.parametrize("name", ["all", "sampled"])
def test_fixture_recorded_directions(name):
    """The reference's own run: the same samples and directions give its float32 diameters to 1e-5 of the diagonal."""
    from smilify_amd import sdf
    from smilify_amd.mesh3d import Meshes

    g, o, c, want = R.fixture_case(name)
    v, f = g["verts"], g["faces"]
    diag, d_lo, d_hi, t_min = R.thresholds(v)
    S = len(o)
    diam, _, _ = compare("fixture " + name, v, f, o, g[name + "_face_idx"], g[name + "_dirs"], t_min, d_lo, d_hi, diag, max(S // 2, 1),
                         ref=dict(cast=c, diam=want), max_amb_rays=0.01, max_amb_samples=0.10)
    ok = ~c["ambiguous"].any(1)
    err = np.abs(diam.astype(np.float64) - g[name + "_diam"])
    print(f"[sdf-ray] fixture {name}: max |diameter - reference| / diag {err[ok].max() / diag:.3g} ({err[~ok].max(initial=0) / diag:.3g} among the others)")
    assert (err[ok] <= 1e-5 * diag).all()
    if name == "all":  # through the public function: the same origins and thresholds are formed from the mesh
        mesh = Meshes(verts=[torch.from_numpy(v).to(DEV)], faces=[torch.from_numpy(f).to(DEV)])
        for n in (-1, len(f)):
            pts, dm = sdf.compute_sdf(mesh, num_samples=n, num_rays=int(g["num_rays"]), directions=torch.from_numpy(g["all_dirs"]))
            assert np.abs(pts.cpu().numpy() - g["all_points"]).max() <= 4 * U * np.abs(v).max()
            assert (np.abs(dm.cpu().numpy().astype(np.float64) - g["all_diam"])[ok] <= 1e-5 * diag).all()


def test_compute_sdf_seed_modes_and_errors():
    from smilify_amd import sdf
    from smilify_amd.mesh3d import Meshes

    g = np.load(os.path.join(GOLDEN, "sdf_ray_ref.npz"))
    v, f = torch.from_numpy(g["verts"]).to(DEV), torch.from_numpy(g["faces"]).to(DEV)
    mesh = Meshes(verts=[v], faces=[f])
    torch.manual_seed(int(g["seed"]))
    pts, dm = sdf.compute_sdf(mesh, num_samples=-1, num_rays=int(g["num_rays"]))
    # all-faces mode under the reference's seed: its directions, hence (to the last bits of the rays' values) its diameters
    _, _, c, _ = R.fixture_case("all")
    ok = ~c["ambiguous"].any(1)
    assert np.abs(pts.cpu().numpy() - g["all_points"]).max() <= 4 * U * np.abs(g["verts"]).max()
    assert (np.abs(dm.cpu().numpy().astype(np.float64) - g["all_diam"])[ok] <= 1e-5 * R.thresholds(g["verts"])[0]).all()
    out = []
    for _ in range(2):
        torch.manual_seed(5)
        out.append(sdf.compute_sdf(mesh, num_samples=40, num_rays=8))
    assert out[0][0].shape == (40, 3) and out[0][1].shape == (40,) and out[0][1].is_cuda
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][1], sdf.compute_sdf(mesh, num_samples=40, num_rays=8)[1])
    lo, hi = (float(x) for x in R.thresholds(g["verts"])[1:3])
    assert ((out[0][1] >= lo) & (out[0][1] < hi)).all()
    flat = f.clone()
    flat[3, 2] = flat[3, 1]  # a face without a normal
    with pytest.raises(ValueError, match="face 3"):
        sdf.compute_sdf(Meshes(verts=[v], faces=[flat]), num_samples=-1)
    with pytest.raises(ValueError):
        sdf.compute_sdf(mesh, num_samples=-1, num_rays=4, directions=torch.zeros(3, 4, 3))
    with pytest.raises(ValueError):
        sdf.compute_sdf(mesh, num_samples=0)


@pytest.fixture(scope="module")
def cloud():
    rng = np.random.RandomState(11)
    pts = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    val = (0.3 + 0.2 * np.sin(3 * pts[:, 0]) + 0.05 * rng.rand(300)).astype(np.float32)
    verts = rng.uniform(-1, 1, (170, 3)).astype(np.float32)
    return pts, val, verts


@pytest.mark.parametrize("k", [1, 10, 50, 64])
def test_smooth_and_assign(cloud, k):
    """Against float64 where the neighbour set is determined.  smooth_distances takes its mean in float64 and rounds once: 2^-24
    relative (asserted: 2 * 2^-24).  assign_vertex_sdf: the kernel's float32 squared distances carry <= 6 * 2^-24 relative (three
    differences, squares, two sums), the weights 1 / (sqrt(d2) + 1e-6) half of that, the normalised weights <= 6 * 2^-24, so the weighted
    mean <= 6 * 2^-24 max|value|; the min-max scaling takes two such errors in the numerator and two in the denominator:
    24 * 2^-24 max|value| / (max - min), plus the float32 rounding of the result (asserted: 32 * 2^-24 max|value| / (max - min) +
    2 * 2^-24)."""
    from smilify_amd import sdf

    pts, val, verts = cloud
    P, Vl, X = (torch.from_numpy(a).to(DEV) for a in (pts, val, verts))
    sm = sdf.smooth_distances(P, Vl, k=k)
    want, det = R.smooth(pts, val, k)
    assert sm.dtype == torch.float32 and sm.shape == (300,) and det.mean() > 0.9
    rel = np.abs(sm.cpu().numpy().astype(np.float64) - want) / np.abs(want)
    print(f"[sdf-ray] smooth k={k}: max rel err {rel[det].max() / U:.2f} x 2^-24")
    assert (rel[det] <= 2 * U).all()
    if k == 1:
        assert torch.equal(sm, Vl)  # the point itself
    vs = sdf.assign_vertex_sdf(X, P, sm, k=k)
    smn = sm.cpu().numpy()
    wantv, detv, raw = R.vertex_values(verts, pts, smn, k)
    tol = 32 * U * np.abs(smn).max() / (raw.max() - raw.min()) + 2 * U
    err = np.abs(vs.cpu().numpy().astype(np.float64) - wantv)
    print(f"[sdf-ray] assign k={k}: max abs err {err[detv].max():.3g} (bound {tol:.3g}) on {int(detv.sum())} of {len(detv)} rows")
    assert vs.dtype == torch.float32 and detv.all(), "min-max scaling couples every row: the case needs determined neighbour sets"
    assert (err <= tol).all() and float(vs.min()) == 0.0 and float(vs.max()) == 1.0


def test_smooth_and_assign_edges(cloud):
    from smilify_amd import sdf

    pts, val, verts = cloud
    P, Vl, X = (torch.from_numpy(a[:40]).to(DEV) for a in (pts, val, verts))
    sm = sdf.smooth_distances(P, Vl, k=40)  # k = N: every point sees every value
    assert (np.abs(sm.cpu().numpy().astype(np.float64) - val[:40].astype(np.float64).mean()) <= 2 * U * val[:40].mean()).all()
    assert torch.equal(sdf.assign_vertex_sdf(X, P, torch.full((40,), 0.37, device=DEV), k=10), torch.zeros(40, device=DEV))
    vs = sdf.assign_vertex_sdf(X, P, Vl, k=40)
    assert float(vs.min()) == 0.0 and float(vs.max()) == 1.0
    for fn, args in ((sdf.smooth_distances, (P, Vl)), (sdf.assign_vertex_sdf, (X, P, Vl))):
        for k in (41, 65, 0):  # k > N, k > SMIL_KNN_MAX_K
            with pytest.raises(ValueError):
                fn(*args, k=k)
    Pl, Vll = (torch.from_numpy(a).to(DEV) for a in (pts, val))
    with pytest.raises(ValueError, match="SMIL_KNN_MAX_K"):
        sdf.smooth_distances(Pl, Vll, k=100)  # the reference's default


def _write_obj(path, v, f):
    with open(path, "w") as fh:
        for p in v.tolist():
            fh.write(f"v {p[0]} {p[1]} {p[2]}\n")
        for q in (f + 1).tolist():
            fh.write(f"f {q[0]} {q[1]} {q[2]}\n")


def test_end_to_end(tmp_path):
    """smilify_amd.sdf writes what fit3d --use_sdf reads: the scan's and the model's values, then one Stage step with the term."""
    import pickle

    from smilify_amd import fit3d, sdf
    from smilify_amd.mesh3d import load_meshes

    d = np.load(os.path.join(GOLDEN, "atta_worker_mesh.npz"))
    (tmp_path / "scans" / "sub").mkdir(parents=True)
    obj = tmp_path / "scans" / "sub" / "atta.obj"
    _write_obj(obj, d["verts"].astype(np.float64), d["faces"].astype(np.int64))
    out = tmp_path / "out"
    sdf.main(sdf.build_parser().parse_args([str(tmp_path / "scans"), "--output_dir", str(out), "--num_samples", "500", "--model",
                                            MODEL_FILES["stick"], "--seed", "3"]))
    data = out / "data"
    stem = os.path.splitext(os.path.basename(MODEL_FILES["stick"]))[0]
    assert sorted(os.listdir(data)) == sorted(f"{n}_sdf.{e}" for n in ("atta", stem) for e in ("npz", "pkl"))
    with open(data / "atta_sdf.pkl", "rb") as fh:
        rec = pickle.load(fh)
    assert set(rec) == {"sample_points", "smoothed_diameters", "vertex_sdf", "verts", "faces", "mesh_file", "num_vertices", "num_faces",
                        "num_samples", "num_rays", "k_smoothing"}
    assert rec["sample_points"].shape == (500, 3) and rec["num_vertices"] == len(d["verts"]) and not rec["vertex_sdf"].is_cuda
    with open(out / "combined_sdf_results.pkl", "rb") as fh:
        assert list(pickle.load(fh)) == ["atta"]
    tv = fit3d.load_sdf_values("atta.obj", str(data), DEV)
    sv = fit3d.load_sdf_values(stem, str(data), DEV)
    model = fit3d.SMAL3DFitter(batch_size=1, device=DEV, model_path=MODEL_FILES["stick"])
    assert tv.shape == (len(d["verts"]),) and sv.shape == (model.smal_model.tables.V,)
    for x in (tv, sv):
        assert torch.isfinite(x).all() and float(x.min()) == 0.0 and float(x.max()) == 1.0 and float(x.std()) > 0.01
    assert torch.equal(tv, rec["vertex_sdf"].to(DEV))
    os.remove(data / "atta_sdf.npz")
    assert torch.equal(fit3d.load_sdf_values("atta.obj", str(data), DEV), tv)  # the .pkl alone
    _, target = load_meshes(mesh_files=[str(obj)], device=DEV)
    stage = fit3d.Stage(1, "init", model, target, loss_weights=dict(w_sdf=0.5), sdf_values=[tv], source_sdf_values=sv)
    stage.optimizer.zero_grad()
    loss, comps = stage.step(0)
    assert "sdf" in comps and torch.isfinite(comps["sdf"]) and float(comps["sdf"].detach()) > 0 and torch.isfinite(loss)
    # the same seed gives the same files
    sdf.main(sdf.build_parser().parse_args([str(tmp_path / "scans"), "--output_dir", str(tmp_path / "again"), "--num_samples", "500",
                                            "--seed", "3"]))
    assert torch.equal(fit3d.load_sdf_values("atta", str(tmp_path / "again" / "data"), DEV), tv)
