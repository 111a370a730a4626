// HardPhong colour rendering for gfx950: the reference Renderer's colour branch.
//
// Replaces (reference): smal_fitter/p3d_renderer.py:54-70,148-150 - MeshRasterizer(blur_radius=0, faces_per_pixel=1, bin_size=0) on the
// same FoVPerspectiveCameras + HardPhongShader(lights=PointLights(location=[[0, 0, 3]])) with default Materials and BlendParams, over
// Meshes(verts, faces, TexturesVertex(MESH_COLOR / 255)).  The arithmetic restates pytorch3d 0.7.x (un-vendored):
// rasterize_meshes.cu (naive kernel, K = 1), clip.py (clip_faces / convert_clipped_rasterization_to_original_faces),
// meshes.py (verts_normals_packed), shading.py (phong_shading), lighting.py (diffuse / specular), blending.py (hard_rgb_blend).
//
//  * k_vertex_normals   thread per (frame, vertex): the sum of the (2 x area) normals of the vertex's faces, gathered through the
//                       vertex -> face CSR of smil_model_create in ascending face order (no atomics: bit-reproducible), normalised
//                       with eps 1e-6.  World space, per frame.
//  * k_raster_setup     (raster.hip, blur 0) per-face tile boxes and depth ranges, binned per-tile face lists, touched-tile work items
//                       by cost class, faces that cross z_clip cut into their front parts (smil_colour_setup).
//  * k_colour_background  the whole output as background (1, 1, 1) / pix_to_face -1.
//  * k_colour_tiles     (the sweep: raster_hard.h, shared with fragments.hip) one wave per 8x8 tile, lane = pixel.  The tile's list is read 64 entries at a time; a face whose nearest vertex
//                       is farther than every pixel's current hit is not fetched at all.  The others are gathered in parallel (lane =
//                       face: vertex ids through the clip tables, affine forms of the three perspective-correct barycentric numerators
//                       relative to the tile centre) and then evaluated one after the other by all 64 pixels (readlane).  A pixel keeps
//                       the smallest (depth, parent face, part): the naive kernel's order with clip_faces' numbering.  The winner is
//                       shaded in registers and written as planar RGB.
//
// Semantics: strictly inside (all perspective-corrected barycentrics > 0), unclipped barycentrics, pz >= 0, no
// culling; barycentrics of a cut face's part mapped back to the original face (each part vertex is a known barycentric point of it).
// colour = (0.5 + 0.3 relu(n.d)) MESH_COLOR (b0 + b1 + b2) + 0.2 (relu(v.r) [n.d > 0])^64, background (1, 1, 1).  No gradient.
#include <algorithm>

#include "common.h"
#include "raster_hard.h"

#define COLOUR_WAVES_PER_CU 28  // single-wave workgroups per CU of the tile kernel's grid (7 per SIMD: what its 65 VGPRs allow)
#define N_EPS 1e-6f              // F.normalize eps of the normals and the light / view directions

// ---------------------------------------------------------------------------------------------
// per-frame vertex normals (Meshes.verts_normals_packed)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_vertex_normals(const float *__restrict__ verts, const int *__restrict__ faces,
                                                        const int *__restrict__ vf_ptr, const int *__restrict__ vf_face, int V,
                                                        float *__restrict__ normals) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float *X = verts + (size_t)blockIdx.y * V * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int e = vf_ptr[v]; e < vf_ptr[v + 1]; ++e) {
        const int f = vf_face[e];
        const float *a = X + 3 * faces[3 * f], *b = X + 3 * faces[3 * f + 1], *c = X + 3 * faces[3 * f + 2];
        // cross(v2 - v1, v0 - v1), as meshes.py forms it
        const float ux = c[0] - b[0], uy = c[1] - b[1], uz = c[2] - b[2];
        const float wx = a[0] - b[0], wy = a[1] - b[1], wz = a[2] - b[2];
        nx += uy * wz - uz * wy;
        ny += uz * wx - ux * wz;
        nz += ux * wy - uy * wx;
    }
    const float inv = 1.0f / fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), N_EPS);
    float *o = normals + ((size_t)blockIdx.y * V + v) * 3;
    o[0] = nx * inv; o[1] = ny * inv; o[2] = nz * inv;
}

// ---------------------------------------------------------------------------------------------
// background
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_colour_background(float *__restrict__ image, size_t n_image, int *__restrict__ p2f, size_t n_p2f) {
    // (plain 4-byte stores: a slice of a batch need not start on a 16-byte boundary)
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_image; i += stride) image[i] = 1.0f;
    if (p2f)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_p2f; i += stride) p2f[i] = -1;
}

// ---------------------------------------------------------------------------------------------
// rasterise (K = 1) + HardPhong
// ---------------------------------------------------------------------------------------------
struct ColourArgs {
    ColourSetup cs;
    const float *verts_ndc;    // (N,V,3)
    const float *verts_world;  // (frames,V,3)
    const float *normals;      // (frames,V,3)
    const int *faces;          // (F,3)
    SmilCameras cam;
    float rgb[3];
    float *image;              // (N,3,S,S)
    int *pix_to_face;          // (N,S,S) or NULL
    int N, V, F, S, tiles_x, views;
    float z_clip;
};

// (the sweep: raster_hard.h; here the HardPhong epilogue of a pixel with a hit)
__global__ void __launch_bounds__(64) k_colour_tiles(ColourArgs a) {
    const int S = a.S, V = a.V;
    hard_tile_sweep(a, [&](int img, size_t pix, int orig, int P0, int P1, int P2, const float (&b)[3], float) {
        const int frame = img / a.views;
        const float *Xw = a.verts_world + (size_t)frame * V * 3;
        const float *Nw = a.normals + (size_t)frame * V * 3;
        const int Pi[3] = {P0, P1, P2};
        float X[3] = {0.f, 0.f, 0.f}, Nn[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                X[q] = fmaf(b[c], Xw[3 * Pi[c] + q], X[q]);
                Nn[q] = fmaf(b[c], Nw[3 * Pi[c] + q], Nn[q]);
            }
        const float bsum = b[0] + b[1] + b[2];
        // camera centre C = -T R^T (X_view = X_world R + T)
        const float *R = a.cam.R + (size_t)(img % a.cam.nR) * 9;
        const float *T = a.cam.T + (size_t)(img % a.cam.nT) * 3;
        float C[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) C[q] = -(T[0] * R[3 * q] + T[1] * R[3 * q + 1] + T[2] * R[3 * q + 2]);
        const float L[3] = {0.f, 0.f, 3.f};
        float d[3], v[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) { d[q] = L[q] - X[q]; v[q] = C[q] - X[q]; }
        const float in_ = 1.0f / fmaxf(sqrtf(Nn[0] * Nn[0] + Nn[1] * Nn[1] + Nn[2] * Nn[2]), N_EPS);
        const float id_ = 1.0f / fmaxf(sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), N_EPS);
        const float iv_ = 1.0f / fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), N_EPS);
#pragma unroll
        for (int q = 0; q < 3; ++q) { Nn[q] *= in_; d[q] *= id_; v[q] *= iv_; }
        const float cosang = Nn[0] * d[0] + Nn[1] * d[1] + Nn[2] * d[2];
        const float diffuse = 0.3f * fmaxf(cosang, 0.f);
        float vr = 0.f;
#pragma unroll
        for (int q = 0; q < 3; ++q) vr += v[q] * (-d[q] + 2.0f * cosang * Nn[q]);
        float al = cosang > 0.f ? fmaxf(vr, 0.f) : 0.f;
#pragma unroll
        for (int q = 0; q < 6; ++q) al *= al;  // ^64
        const float spec = 0.2f * al;
        const float amb_diff = (0.5f + diffuse) * bsum;
        float *o = a.image + (size_t)img * 3 * S * S + pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * S * S] = amb_diff * a.rgb[c] + spec;
        if (a.pix_to_face) a.pix_to_face[(size_t)img * S * S + pix] = orig;
    });
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// the setup's tables (raster.hip), then vertex normals of up to N frames
static size_t colour_layout(const SmilModel *m, int N, int S, char *base, float **normals) {
    Workspace w{base};
    w.take<char>(smil_colour_setup_bytes(m, N, S));
    *normals = w.take<float>((size_t)N * m->V * 3);
    return w.used;
}

extern "C" size_t smil_colour_workspace_bytes(const SmilModel *m, int32_t N, int32_t S) {
    float *normals;
    return (m && N > 0 && S > 0) ? colour_layout(m, N, S, nullptr, &normals) : 0;
}

extern "C" int smil_render_colour(const SmilModel *m, const SmilCameras *cam, const float *verts_world, const float *verts_ndc,
                                  const float rgb[3], float *image, int32_t *pix_to_face, void *workspace, void *stream_) {
    SMIL_REQUIRE(m && cam && verts_world && verts_ndc && rgb && image && workspace, "smil_render_colour: null argument");
    SMIL_REQUIRE(cam->N > 0 && cam->views > 0 && cam->N % cam->views == 0 && cam->S > 0, "smil_render_colour: bad sizes N=%d views=%d S=%d",
                 cam->N, cam->views, cam->S);
    SMIL_REQUIRE(cam->R && cam->T && cam->nR > 0 && cam->nT > 0, "smil_render_colour: camera tables missing");
    for (int k : {cam->nR, cam->nT})
        SMIL_REQUIRE(k == 1 || k == cam->views || k == cam->N, "smil_render_colour: camera table of %d rows for %d images, %d views", k, cam->N,
                     cam->views);
    hipStream_t stream = (hipStream_t)stream_;
    const int N = cam->N, S = cam->S, V = m->V, frames = N / cam->views;
    ColourArgs a;
    int rc = smil_colour_setup(m, verts_ndc, N, S, 0.5f * SMIL_ZNEAR, workspace, stream, &a.cs);
    if (rc) return rc;
    float *normals;
    colour_layout(m, N, S, (char *)workspace, &normals);
    hipLaunchKernelGGL(k_vertex_normals, dim3(ceil_div(V, 256), frames), dim3(256), 0, stream, verts_world, m->faces, m->vf_ptr, m->vf_face, V,
                       normals);
    SMIL_LAUNCH_CHECK();
    {
        const size_t n_img = (size_t)N * 3 * S * S, n_p2f = (size_t)N * S * S;
        const unsigned int grid = (unsigned int)std::min<size_t>((n_img + 255) / 256, (size_t)256 * 64);
        hipLaunchKernelGGL(k_colour_background, dim3(grid), dim3(256), 0, stream, image, n_img, (int *)pix_to_face, pix_to_face ? n_p2f : 0);
        SMIL_LAUNCH_CHECK();
    }
    a.verts_ndc = verts_ndc; a.verts_world = verts_world; a.normals = normals; a.faces = m->faces; a.cam = *cam;
    a.rgb[0] = rgb[0]; a.rgb[1] = rgb[1]; a.rgb[2] = rgb[2];
    a.image = image; a.pix_to_face = pix_to_face;
    a.N = N; a.V = V; a.F = m->F; a.S = S; a.tiles_x = ceil_div(S, TILE); a.views = cam->views; a.z_clip = 0.5f * SMIL_ZNEAR;
    hipLaunchKernelGGL(k_colour_tiles, dim3((unsigned int)smil_device_limits().cus * COLOUR_WAVES_PER_CU), dim3(64), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
