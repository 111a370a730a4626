// Triangle meshes of visual hulls: surface nets on the lattice of voxel centres, for gfx950.  The specification is at
// include/smilfit.h ("Hull meshes"); tests/hull_mesh_ref.py restates it in numpy.
//
// Names.  Sample (i, j, k) is inside iff occ != 0, the lattice padded by one layer of outside samples.  Cube (i, j, k), every index in
// -1 .. G-1, has the shifted coordinates (a, b, c) = (i+1, j+1, k+1) and the linear index a + Cx (b + Cy c), C = G + 1.  Its `cfg` holds
// bit dx + 2 dy + 4 dz iff corner sample (i+dx, j+dy, k+dz) is inside; it is active - owns a vertex - iff cfg is neither 0 nor 255.
// A frame's cubes are padded to whole workgroups of MESH_BLOCK_WORDS words of 64 cubes, so a word and a workgroup stay inside a frame.
//
//  * k_mesh_classify   streams the occupancy once: a wave per 64 consecutive cubes, 8 corner bytes per lane (the 8 cubes around a
//                      sample share them through the caches), __ballot of "active" -> the word's 64-bit mask, ballots of the three owned
//                      sign-changing edges -> its quad count.  A workgroup of 4 waves takes MESH_BLOCK_WORDS = 32 words, leaves the
//                      words' exclusive prefixes inside the workgroup packed in 32 bits (vertices low, quads high) and its two totals.
//  * hull_scan         (hull_grid.h; the kernel is visual_hull.hip's k_hull_scan) the workgroups' totals -> exclusive prefixes (the
//                      totals behind the last), the frames' offsets out: one workgroup for the vertices, one for the quads.
//  * mesh_vertex_id    the only lookup the later kernels need: prefix[workgroup] + prefix[word] + popcount(mask[word] & lower lanes) -
//                      12 bytes per 64 cubes of workspace instead of a dense index grid; its three loads do not depend on each other.
//  * k_mesh_emit       the same walk, a word whose mask is 0 skipped (a wave-uniform test): the corners again, the start position
//                      (the exact sum of the sign-changing edges' midpoints, one division), cfg and the cube index per vertex, and the
//                      faces of the owned edges at prefix + popcounts of the ballots: ascending cube, then axis, whatever the scheduling.
//  * k_mesh_relax      one lane per vertex, Jacobi: reads one float64 buffer, writes the other.
//  * k_mesh_finish     one lane per vertex: the world position rounded once to float32 and, if asked, the area-weighted normal as a
//                      gather over the quads of the cube's sign-changing edges.
// Pure gathers and ballots: no atomics, two calls give the same bits.  Every float64 step is written in the specification's order with
// contraction off.  Global indices are 64-bit (N Cx Cy Cz may exceed 2^31); a frame holds fewer than 2^31 cubes, so what stays inside a
// frame is 32-bit.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "hull_grid.h"

#define MESH_BLOCK_WORDS 32                                // words of 64 cubes per workgroup
#define MESH_WAVE_WORDS (MESH_BLOCK_WORDS / (HULL_THREADS / 64))
#define MESH_BLOCK_CUBES (MESH_BLOCK_WORDS * 64)
#define MESH_MAX_BLOCKS (1LL << 28)                        // N x workgroups of a frame: the per-vertex launches stay below 2^31 blocks

struct MeshGrid {
    int Gx, Gy, Gz, Cx, Cy;
    unsigned cubes;     // of a frame, < 2^31
    unsigned blocks;    // workgroups of a frame
    long long vox;      // samples of a frame
    const unsigned long long *mask;  // (N blocks 32) the words' active lanes
    const unsigned *wpre;            // (N blocks 32) a word's exclusive prefix inside its workgroup: vertices | quads << 16
    const long long *vpre, *qpre;    // (N blocks + 1) the workgroups' exclusive prefixes, the total last
    long long all_blocks;            // N blocks
};

// The caller sized the outputs from the offsets of the count call; the write's kernels store nothing unless its figures are the
// workspace's own (a wave-uniform test of two loads), so a wrong figure can never become an index behind a buffer's end.
__device__ __forceinline__ bool mesh_counts_agree(const MeshGrid &g, long long n_verts, long long n_faces) {
    return g.vpre[g.all_blocks] == n_verts && 2 * g.qpre[g.all_blocks] == n_faces;
}

// cfg of cube (a, b, c): the 8 corner bytes, an index outside the grid reading "outside" without a load
__device__ __forceinline__ unsigned mesh_cfg(const unsigned char *o, const MeshGrid &g, int a, int b, int c) {
    unsigned cfg = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int i = a - 1 + (d & 1), j = b - 1 + (d >> 1 & 1), k = c - 1 + (d >> 2);
        const bool in = i >= 0 && i < g.Gx && j >= 0 && j < g.Gy && k >= 0 && k < g.Gz;
        const unsigned char v = in ? o[(size_t)i + (size_t)g.Gx * ((size_t)j + (size_t)g.Gy * (size_t)k)] : (unsigned char)0;
        cfg |= (v ? 1u : 0u) << d;
    }
    return cfg;
}

__device__ __forceinline__ void mesh_decode(unsigned cube, const MeshGrid &g, int &a, int &b, int &c) {
    const unsigned t = cube / (unsigned)g.Cx, q = t / (unsigned)g.Cy;
    a = (int)(cube - t * (unsigned)g.Cx); b = (int)(t - q * (unsigned)g.Cy); c = (int)q;
}

// the packed vertex of cube `cube` of the frame whose first word is `word0` (the cube must be active)
__device__ __forceinline__ long long mesh_vertex_id(const MeshGrid &g, long long word0, unsigned cube) {
    const long long w = word0 + (cube >> 6);
    const unsigned long long m = g.mask[w];
    const unsigned p = g.wpre[w];
    const long long base = g.vpre[w / MESH_BLOCK_WORDS];
    return base + (p & 0xFFFFu) + __popcll(m & ((1ULL << (cube & 63)) - 1ULL));
}

// ---- classify ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HULL_THREADS) k_mesh_classify(const unsigned char *occ, MeshGrid g, unsigned long long *mask, unsigned *wpre,
                                                                long long *vcount, long long *qcount) {
    __shared__ unsigned s_v[MESH_BLOCK_WORDS], s_q[MESH_BLOCK_WORDS];
    const long long frame = (long long)(blockIdx.x / g.blocks);
    const unsigned blk = blockIdx.x % g.blocks;
    const unsigned char *o = occ + (size_t)frame * (size_t)g.vox;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 2
    for (int q = 0; q < MESH_WAVE_WORDS; ++q) {
        const int word = wave * MESH_WAVE_WORDS + q;
        const unsigned cube = (blk * MESH_BLOCK_WORDS + word) * 64u + lane;
        unsigned cfg = 0;
        if (cube < g.cubes) {
            int a, b, c;
            mesh_decode(cube, g, a, b, c);
            cfg = mesh_cfg(o, g, a, b, c);
        }
        const unsigned long long m = __ballot(cfg != 0 && cfg != 255);
        const unsigned lower = cfg & 1;
        const int quads = __popcll(__ballot((cfg >> 1 & 1) != lower)) + __popcll(__ballot((cfg >> 2 & 1) != lower)) +
                          __popcll(__ballot((cfg >> 4 & 1) != lower));
        if (lane == 0) {
            mask[(long long)blockIdx.x * MESH_BLOCK_WORDS + word] = m;
            s_v[word] = (unsigned)__popcll(m);
            s_q[word] = (unsigned)quads;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned v = 0, qd = 0;  // (at most 2 048 vertices and 6 144 quads: 16 bits each)
    for (int w = 0; w < MESH_BLOCK_WORDS; ++w) {
        wpre[(long long)blockIdx.x * MESH_BLOCK_WORDS + w] = v | qd << 16;
        v += s_v[w]; qd += s_q[w];
    }
    vcount[blockIdx.x] = v;
    qcount[blockIdx.x] = qd;
}

// ---- emit -------------------------------------------------------------------------------------------------------------------
struct MeshEmit {
    double *pos;            // (n_verts,3) start positions, index coordinates
    unsigned char *cfg;     // (n_verts)
    long long *vcube;       // (n_verts) frame x padded cubes of a frame + cube
    long long *faces;       // (n_faces,3) frame-local
    long long n_verts, n_faces;
};

__global__ void __launch_bounds__(HULL_THREADS) k_mesh_emit(const unsigned char *occ, MeshGrid g, MeshEmit e) {
    const long long frame = (long long)(blockIdx.x / g.blocks);
    const unsigned blk = blockIdx.x % g.blocks;
    const unsigned char *o = occ + (size_t)frame * (size_t)g.vox;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long word0 = frame * g.blocks * MESH_BLOCK_WORDS;
    const long long vbase = g.vpre[blockIdx.x], qbase = g.qpre[blockIdx.x], vframe = g.vpre[frame * g.blocks];
    const unsigned long long below = (1ULL << lane) - 1ULL;
    if (!mesh_counts_agree(g, e.n_verts, e.n_faces)) return;
#pragma unroll 1
    for (int q = 0; q < MESH_WAVE_WORDS; ++q) {
        const long long w = (long long)blockIdx.x * MESH_BLOCK_WORDS + wave * MESH_WAVE_WORDS + q;
        const unsigned long long m = g.mask[w];
        if (m == 0) continue;  // (wave-uniform; an owned sign-changing edge makes its cube active: no face is lost)
        const unsigned pre = g.wpre[w];
        const bool active = m >> lane & 1;
        const unsigned cube = (blk * MESH_BLOCK_WORDS + wave * MESH_WAVE_WORDS + q) * 64u + lane;
        int a = 0, b = 0, c = 0;
        unsigned cfg = 0;
        if (active) {
            mesh_decode(cube, g, a, b, c);
            cfg = mesh_cfg(o, g, a, b, c);
        }
        const long long vid = vbase + (pre & 0xFFFFu) + __popcll(m & below);
        if (active) {
            // the 12 edges: axis t = x, y, z, u = (t+1) % 3, v = (t+2) % 3, (ou, ov) = (0,0), (1,0), (0,1), (1,1).  Every midpoint is
            // (i, j, k) + a multiple of 0.5: the sum is exact in any order
            int n = 0;
            double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int u = (t + 1) % 3, v = (t + 2) % 3;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ou = k & 1, ov = k >> 1, bit = (ou << u) + (ov << v);
                    if ((cfg >> bit & 1) != (cfg >> (bit + (1 << t)) & 1)) {
                        ++n;
                        s[t] += 0.5; s[u] += ou; s[v] += ov;
                    }
                }
            }
            const double dn = (double)n;
            e.pos[3 * vid] = (dn * (double)(a - 1) + s[0]) / dn;
            e.pos[3 * vid + 1] = (dn * (double)(b - 1) + s[1]) / dn;
            e.pos[3 * vid + 2] = (dn * (double)(c - 1) + s[2]) / dn;
            e.cfg[vid] = (unsigned char)cfg;
            e.vcube[vid] = (long long)blockIdx.x * MESH_BLOCK_CUBES + (wave * MESH_WAVE_WORDS + q) * 64 + lane;
        }
        // faces: the owned edges from the minimum corner along +x, +y, +z
        const unsigned lower = cfg & 1;
        const bool own[3] = {(cfg >> 1 & 1) != lower, (cfg >> 2 & 1) != lower, (cfg >> 4 & 1) != lower};
        const unsigned long long bx = __ballot(own[0]), by = __ballot(own[1]), bz = __ballot(own[2]);
        long long quad = qbase + (pre >> 16) + __popcll(bx & below) + __popcll(by & below) + __popcll(bz & below);
        const long long mine = vid - vframe;
        const int stride[3] = {1, g.Cx, g.Cx * g.Cy};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (!own[t]) continue;
            const int u = (t + 1) % 3, v = (t + 2) % 3;
            // the four cubes around the edge, (du, dv) = (-1,-1), (0,-1), (0,0), (-1,0); the edge's inside sample lies in the grid, so
            // they all exist
            long long id[4];
            id[0] = mesh_vertex_id(g, word0, cube - stride[u] - stride[v]) - vframe;
            id[1] = mesh_vertex_id(g, word0, cube - stride[v]) - vframe;
            id[2] = mine;
            id[3] = mesh_vertex_id(g, word0, cube - stride[u]) - vframe;
            if (!lower) { const long long x = id[0], y = id[1]; id[0] = id[3]; id[1] = id[2]; id[2] = y; id[3] = x; }
            long long *f = e.faces + 6 * quad;
            f[0] = id[0]; f[1] = id[1]; f[2] = id[2];
            f[3] = id[0]; f[4] = id[2]; f[5] = id[3];
            ++quad;
        }
    }
}

// ---- relax ------------------------------------------------------------------------------------------------------------------
struct MeshVerts {
    const unsigned char *cfg;
    const long long *vcube;
    long long n_verts, n_faces;
};

// the vertex's frame, cube and the frame's first word
__device__ __forceinline__ void mesh_locate(const MeshGrid &g, long long vcube, unsigned &frame, unsigned &cube, long long &word0) {
    const unsigned gblock = (unsigned)(vcube / MESH_BLOCK_CUBES);  // (N blocks <= 2^28)
    const unsigned f = gblock / g.blocks;
    frame = f;
    cube = (gblock - f * g.blocks) * MESH_BLOCK_CUBES + (unsigned)(vcube % MESH_BLOCK_CUBES);
    word0 = (long long)f * g.blocks * MESH_BLOCK_WORDS;
}

__global__ void __launch_bounds__(HULL_THREADS) k_mesh_relax(MeshGrid g, MeshVerts mv, const double *src, double *dst, double weight) {
#pragma clang fp contract(off)
    const long long vid = (long long)blockIdx.x * HULL_THREADS + threadIdx.x;
    if (!mesh_counts_agree(g, mv.n_verts, mv.n_faces) || vid >= mv.n_verts) return;
    long long word0;
    unsigned frame, cube;
    mesh_locate(g, mv.vcube[vid], frame, cube, word0);
    const unsigned cfg = mv.cfg[vid];
    int abc[3];
    mesh_decode(cube, g, abc[0], abc[1], abc[2]);
    const int stride[3] = {1, g.Cx, g.Cx * g.Cy};
    const double p[3] = {src[3 * vid], src[3 * vid + 1], src[3 * vid + 2]};
    // neighbours -x, +x, -y, +y, -z, +z: across a face whose 4 samples are not all of one kind (both cubes are then active)
    const unsigned face_bits[6] = {0x55, 0xAA, 0x33, 0xCC, 0x0F, 0xF0};
    long long nb[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const unsigned f = cfg & face_bits[d];
        const bool mixed = f != 0 && f != face_bits[d];
        nb[d] = mixed ? mesh_vertex_id(g, word0, (d & 1) ? cube + stride[d >> 1] : cube - stride[d >> 1]) : -1;
    }
    double s[3] = {0.0, 0.0, 0.0};
    int n = 0;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        if (nb[d] < 0) continue;
        s[0] += src[3 * nb[d]]; s[1] += src[3 * nb[d] + 1]; s[2] += src[3 * nb[d] + 2];
        ++n;
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        double r = p[t];
        if (n) {
            const double mean = s[t] / (double)n;
            const double step = weight * (mean - p[t]);
            r = p[t] + step;
            const double lo = (double)(abc[t] - 1), hi = (double)abc[t];
            r = fmin(fmax(r, lo), hi);
        }
        dst[3 * vid + t] = r;
    }
}

// ---- finish -----------------------------------------------------------------------------------------------------------------
struct MeshOut {
    const double *origin, *voxel;  // device copies of the caller's tables
    int n_origin, n_voxel;
    float *verts, *normals;
};

template <bool NORMALS>
__global__ void __launch_bounds__(HULL_THREADS) k_mesh_finish(MeshGrid g, MeshVerts mv, MeshOut out, const double *pos) {
#pragma clang fp contract(off)
    const long long vid = (long long)blockIdx.x * HULL_THREADS + threadIdx.x;
    if (!mesh_counts_agree(g, mv.n_verts, mv.n_faces) || vid >= mv.n_verts) return;
    long long word0;
    unsigned frame, cube;
    mesh_locate(g, mv.vcube[vid], frame, cube, word0);
    const double *org = out.origin + 3 * (frame % out.n_origin);
    const double voxel = out.voxel[frame % out.n_voxel];
    const double p[3] = {pos[3 * vid], pos[3 * vid + 1], pos[3 * vid + 2]};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const double h = (p[t] + 0.5) * voxel;
        out.verts[3 * vid + t] = (float)(org[t] + h);
    }
    if (!NORMALS) return;
    const unsigned cfg = mv.cfg[vid];
    const int stride[3] = {1, g.Cx, g.Cx * g.Cy};
    const double me[3] = {p[0] * voxel, p[1] * voxel, p[2] * voxel};
    double nrm[3] = {0.0, 0.0, 0.0};
    // the 12 edges in the order of the start positions; a sign-changing one names a quad around it
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int u = (t + 1) % 3, v = (t + 2) % 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ou = k & 1, ov = k >> 1, bit = (ou << u) + (ov << v);
            const unsigned lower = cfg >> bit & 1;
            if (lower == (cfg >> (bit + (1 << t)) & 1)) continue;
            // the quad's cubes (du, dv) = (-1,-1), (0,-1), (0,0), (-1,0) from the edge, (ou + du, ov + dv) from this cube
            double P[4][3];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int eu = ou + ((m == 0 || m == 3) ? -1 : 0), ev = ov + (m < 2 ? -1 : 0);
                if (eu == 0 && ev == 0) {
                    P[m][0] = me[0]; P[m][1] = me[1]; P[m][2] = me[2];
                } else {
                    const long long id = mesh_vertex_id(g, word0, cube + eu * stride[u] + ev * stride[v]);
                    P[m][0] = pos[3 * id] * voxel; P[m][1] = pos[3 * id + 1] * voxel; P[m][2] = pos[3 * id + 2] * voxel;
                }
            }
            int self = ou ? (ov ? 0 : 3) : (ov ? 1 : 2);
            int order[4] = {0, 1, 2, 3};
            if (!lower) { order[0] = 3; order[1] = 2; order[2] = 1; order[3] = 0; self = 3 - self; }
            // triangles (q0,q1,q2) and (q0,q2,q3): the first holds q0, q1, q2, the second q0, q2, q3
#pragma unroll
            for (int tri = 0; tri < 2; ++tri) {
                if (self == (tri ? 1 : 3)) continue;
                const double *p0 = P[order[0]], *p1 = P[order[tri ? 2 : 1]], *p2 = P[order[tri ? 3 : 2]];
                const double a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
                const double b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
                nrm[0] += a[1] * b[2] - a[2] * b[1];
                nrm[1] += a[2] * b[0] - a[0] * b[2];
                nrm[2] += a[0] * b[1] - a[1] * b[0];
            }
        }
    }
    const double len = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
#pragma unroll
    for (int t = 0; t < 3; ++t) out.normals[3 * vid + t] = len == 0.0 ? 0.0f : (float)(nrm[t] / len);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct MeshWorkspace {
    HullWorkspace h;
    long long *vpre, *qpre;
    unsigned long long *mask;
    unsigned *wpre;
    size_t bytes;
};

static MeshWorkspace mesh_layout(void *base, const SmilHullGrid *g, long long all_blocks) {
    MeshWorkspace w;
    w.h = hull_layout(base, g, 2 * (all_blocks + 1));
    w.vpre = w.h.counts;
    w.qpre = base ? w.h.counts + all_blocks + 1 : nullptr;
    Workspace ws{base ? (char *)base + w.h.bytes : nullptr};
    w.mask = ws.take<unsigned long long>((size_t)all_blocks * MESH_BLOCK_WORDS);
    w.wpre = ws.take<unsigned>((size_t)all_blocks * MESH_BLOCK_WORDS);
    w.bytes = w.h.bytes + ws.used;
    return w;
}

static int check_mesh_grid(const char *who, const SmilHullGrid *g, bool tables, MeshGrid *out) {
    long long vox;
    if (int rc = check_hull_grid(who, g, tables, &vox)) return rc;
    SMIL_REQUIRE(g->n_origin >= 1 && g->n_voxel_size >= 1, "%s: the grid's table sizes lay out the workspace: %d, %d", who, g->n_origin,
                 g->n_voxel_size);
    const long long slice = ((long long)g->Gx + 1) * ((long long)g->Gy + 1);
    SMIL_REQUIRE(slice <= 0x7FFFFFFFLL / ((long long)g->Gz + 1),
                 "%s: a frame of %d x %d x %d voxels has 2^31 or more cubes and could hold 2^31 vertices", who, g->Gx, g->Gy, g->Gz);
    const long long cubes = slice * ((long long)g->Gz + 1);
    const long long blocks = hull_chunks(cubes, MESH_BLOCK_CUBES);
    SMIL_REQUIRE(blocks <= MESH_MAX_BLOCKS / g->N, "%s: N=%d frames of %lld cubes exceed the grid", who, g->N, cubes);
    *out = MeshGrid{g->Gx, g->Gy, g->Gz, g->Gx + 1, g->Gy + 1, (unsigned)cubes, (unsigned)blocks, vox, nullptr, nullptr, nullptr, nullptr,
                    blocks * g->N};
    return SMIL_OK;
}

static void mesh_bind(MeshGrid *d, const MeshWorkspace &w) {
    d->mask = w.mask; d->wpre = w.wpre; d->vpre = w.vpre; d->qpre = w.qpre;
}

extern "C" size_t smil_hull_mesh_workspace_bytes(const SmilHullGrid *g) {
    MeshGrid d;
    if (check_mesh_grid("smil_hull_mesh_workspace_bytes", g, false, &d)) return 0;
    return mesh_layout(nullptr, g, d.all_blocks).bytes;
}

extern "C" int smil_hull_mesh_count(const SmilHullGrid *g, const uint8_t *occ, int64_t *vert_offsets, int64_t *face_offsets, void *workspace,
                                    void *stream_) {
    MeshGrid d;
    if (int rc = check_mesh_grid("smil_hull_mesh_count", g, false, &d)) return rc;
    SMIL_REQUIRE(occ && vert_offsets && face_offsets && workspace, "smil_hull_mesh_count: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    const MeshWorkspace w = mesh_layout(workspace, g, d.all_blocks);
    mesh_bind(&d, w);
    hipLaunchKernelGGL(k_mesh_classify, dim3((unsigned)d.all_blocks), dim3(HULL_THREADS), 0, stream, (const unsigned char *)occ, d, w.mask, w.wpre,
                       w.vpre, w.qpre);
    SMIL_LAUNCH_CHECK();
    // vertices, and quads of two triangles each; the totals stay behind the prefixes (mesh_counts_agree)
    const HullScanJob jobs[2] = {{w.vpre, (long long *)vert_offsets, 1, 1}, {w.qpre, (long long *)face_offsets, 2, 1}};
    return hull_scan(jobs, 2, d.all_blocks, (long long)d.blocks, g->N, stream);
}

struct MeshScratch { double *pos[2]; long long *vcube; unsigned char *cfg; size_t bytes; };
static MeshScratch mesh_scratch(void *base, long long n_verts, int n_steps) {
    Workspace ws{(char *)base};
    MeshScratch s;
    s.pos[0] = ws.take<double>(3 * (size_t)n_verts);
    s.pos[1] = ws.take<double>(n_steps > 0 ? 3 * (size_t)n_verts : 0);
    s.vcube = ws.take<long long>((size_t)n_verts);
    s.cfg = ws.take<unsigned char>((size_t)n_verts);
    s.bytes = ws.used;
    return s;
}

extern "C" size_t smil_hull_mesh_scratch_bytes(int64_t n_verts, int32_t n_steps) {
    if (n_verts < 0 || n_verts > ((int64_t)1 << 40) || n_steps < 0) return 0;
    return mesh_scratch(nullptr, n_verts, n_steps).bytes;
}

extern "C" int smil_hull_mesh_write(const SmilHullGrid *g, const uint8_t *occ, void *workspace, void *scratch, int64_t n_verts, int64_t n_faces,
                                    const double *weights, int32_t n_steps, float *verts, float *normals, int64_t *faces, void *stream_) {
    MeshGrid d;
    if (int rc = check_mesh_grid("smil_hull_mesh_write", g, true, &d)) return rc;
    SMIL_REQUIRE(n_steps >= 0, "smil_hull_mesh_write: n_steps=%d is negative", n_steps);
    SMIL_REQUIRE(n_steps == 0 || weights, "smil_hull_mesh_write: null weights with n_steps=%d", n_steps);
    for (int s = 0; s < n_steps; ++s) SMIL_REQUIRE(std::isfinite(weights[s]), "smil_hull_mesh_write: weights[%d]=%g must be finite", s, weights[s]);
    SMIL_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_verts <= d.all_blocks * MESH_BLOCK_CUBES && n_faces <= 6 * d.all_blocks * MESH_BLOCK_CUBES,
                 "smil_hull_mesh_write: n_verts=%lld, n_faces=%lld are not counts of this grid", (long long)n_verts, (long long)n_faces);
    SMIL_REQUIRE(occ && workspace, "smil_hull_mesh_write: null occ or workspace");
    if (n_verts == 0 && n_faces == 0) return SMIL_OK;
    SMIL_REQUIRE(scratch && verts && faces, "smil_hull_mesh_write: null scratch, verts or faces");
    hipStream_t stream = (hipStream_t)stream_;
    const MeshWorkspace w = mesh_layout(workspace, g, d.all_blocks);
    mesh_bind(&d, w);
    HullGridDev tables;
    if (int rc = hull_upload(w.h, g, d.vox, MESH_BLOCK_CUBES, &tables, stream)) return rc;
    const MeshScratch sc = mesh_scratch(scratch, n_verts, n_steps);
    const MeshEmit e{sc.pos[0], sc.cfg, sc.vcube, (long long *)faces, n_verts, n_faces};
    hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)d.all_blocks), dim3(HULL_THREADS), 0, stream, (const unsigned char *)occ, d, e);
    SMIL_LAUNCH_CHECK();
    const MeshVerts mv{sc.cfg, sc.vcube, n_verts, n_faces};
    const dim3 per_vertex((unsigned)hull_chunks(n_verts, HULL_THREADS));
    if (n_verts == 0) return SMIL_OK;
    for (int s = 0; s < n_steps; ++s) {
        hipLaunchKernelGGL(k_mesh_relax, per_vertex, dim3(HULL_THREADS), 0, stream, d, mv, (const double *)sc.pos[s & 1], sc.pos[(s + 1) & 1], weights[s]);
        SMIL_LAUNCH_CHECK();
    }
    const MeshOut out{tables.origin, tables.voxel, tables.n_origin, tables.n_voxel, verts, normals};
    if (normals) hipLaunchKernelGGL(k_mesh_finish<true>, per_vertex, dim3(HULL_THREADS), 0, stream, d, mv, out, (const double *)sc.pos[n_steps & 1]);
    else hipLaunchKernelGGL(k_mesh_finish<false>, per_vertex, dim3(HULL_THREADS), 0, stream, d, mv, out, (const double *)sc.pos[n_steps & 1]);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
