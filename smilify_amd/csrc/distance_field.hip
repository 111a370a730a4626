// Exact Euclidean distance transforms of occupancy grids and masks, and a differentiable sampler of the resulting fields, for gfx950.
// The specification is at include/smilfit.h ("Distance fields").
//
// The transform is the separable min-plus form of the squared distance: d2 = min_k' ( dz^2 + min_j' ( dy^2 + min_i' dx^2 ) ), one pass
// per axis, all in integers, so the result is the definition's to the bit whatever the order of evaluation.  A pass along a line f of
// length L computes g[l] = min_l' f[l'] + (l - l')^2 by an outward search from l that stops as soon as delta^2 >= the best value so
// far (every candidate further out is at least delta^2), over the cells of the line that hold a value at all (edt_range): the work per
// cell is the distance it ends up with, not L, and there is no per-line stack that would tie a line to one lane.  With `border` the
// cells -1 and L of every line are features, which seeds the search with (l + 1)^2 and (L - l)^2: the nearest cell of the one-voxel
// shell around the grid is always straight along an axis.
//
//  * edt_row           the x pass of one row by one wave, 64 cells at a time: a ballot of the chunk's features, the nearest one at or
//                      before a lane by a count of leading zeros, carried from chunk to chunk; then the same from the right.  The
//                      left sweep stores the distance, the right sweep the minimum of the two (each lane re-reads its own store).
//  * k_edt_xy<CELLS>   x and y fused for one z-slice (frame, k) that fits the LDS as 16-bit x distances (Gx Gy <= 65 536: 128 KiB):
//                      the bytes are read once, rows by waves, and the y search of cell (i, j) walks column i of the LDS image -
//                      consecutive lanes on consecutive i, so LDS reads and the int32 stores are contiguous.
//  * k_edt_x           the x pass alone into global memory, for slices that do not fit.
//  * k_edt_line<LINES> a y or z pass in place: a workgroup owns 64 consecutive columns by a whole line (LINES = 32, 128, 256 or 512
//                      cells: 8 to 128 KiB of int32, with 256 to 1 024 threads), loads it with rows of 256 contiguous bytes, searches in LDS and stores over its own input.  For the z
//                      pass a "column" is a cell of the flattened (j, i) plane, so the accesses are contiguous whatever Gx is.
//  * k_edt_line_far    the same pass for lines of more than EDT_MAX_LINE cells: one lane per cell, searching in global memory, from
//                      one buffer into another (the workspace holds the second one).
//  * k_field_sample    one lane per point: float64 on the float32 point, eight (four) gathers, one rounding per output.
// No atomics, no host synchronisation; every linear index is 64-bit.
#include "hull_grid.h"

#define EDT_NONE 0x7FFFFFFFu     // SMIL_EDT_NONE as the unsigned the searches compare
#define EDT_NO16 0xFFFFu         // "no feature in this row" of the 16-bit x distances (a grid extent stays below 46 340)
#define EDT_MAX_SLICE 65536      // cells of the largest z-slice k_edt_xy holds
#define EDT_MAX_LINE 512         // cells of the longest line k_edt_line holds
#define EDT_COLS 64              // columns of a k_edt_line workgroup
#define EDT_THREADS 256

struct EdtArgs {
    const unsigned char *occ;
    int *d2;
    int Gx, Gy;
    int invert, border;
    long long rows;  // N Gz Gy (k_edt_x)
};

// The x pass of one row by one wave.  feat(i): is cell i a feature; ld / st: the row's distances (EDT_NO16: none).
template <typename Feat, typename Ld, typename St>
__device__ __forceinline__ void edt_row(int Gx, int border, Feat feat, Ld ld, St st) {
    const int lane = threadIdx.x & 63;
    const int last = (Gx - 1) & ~63;
    int carry = border ? -1 : -(int)EDT_NO16 - Gx;  // the nearest feature left of the chunk (so far away that min() drops it)
    for (int base = 0; base <= last; base += 64) {
        const int i = base + lane;
        const unsigned long long mask = __ballot(i < Gx && feat(i));
        const unsigned long long below = mask & ((2ull << lane) - 1ull);  // (lane 63: 2 << 63 wraps to 0, minus 1 = every bit)
        const int left = below ? base + 63 - __builtin_clzll(below) : carry;
        if (i < Gx) st(i, min(i - left, (int)EDT_NO16));
        if (mask) carry = base + 63 - __builtin_clzll(mask);
    }
    carry = border ? Gx : 2 * Gx + (int)EDT_NO16;
    for (int base = last; base >= 0; base -= 64) {
        const int i = base + lane;
        const int mine = i < Gx ? ld(i) : (int)EDT_NO16;
        const unsigned long long mask = __ballot(mine == 0);
        const unsigned long long above = mask >> lane;
        const int right = above ? i + __builtin_ctzll(above) : carry;
        if (i < Gx) st(i, min(mine, min(right - i, (int)EDT_NO16)));
        if (mask) carry = base + __builtin_ctzll(mask);
    }
}

// min over l' of f[l'] + (l - l')^2 for cell l of a line of L cells; load(d) reads f[l + d], seed is f[l].  Only the cells lmin .. lmax
// of the line hold a value other than EDT_NONE (edt_range; an empty line: lmin > lmax), so the search starts at the nearest of them
// and ends when it has left them on both sides.
template <typename Load>
__device__ __forceinline__ unsigned edt_search(int l, int L, int lmin, int lmax, int border, unsigned seed, Load load) {
    unsigned best = seed;
    if (border) best = min(best, min((unsigned)(l + 1) * (unsigned)(l + 1), (unsigned)(L - l) * (unsigned)(L - l)));
    for (int dl = l < lmin ? lmin - l : (l > lmax ? l - lmax : 1);; ++dl) {
        const unsigned dd = (unsigned)dl * (unsigned)dl;
        const bool lo = l - dl >= lmin, hi = l + dl <= lmax;
        if (dd >= best || !(lo || hi)) break;
        if (lo) best = min(best, load(-dl) + dd);  // (EDT_NONE + dd stays below 2^32)
        if (hi) best = min(best, load(dl) + dd);
    }
    return best;
}

// the first and the last cell of a line of L cells that holds a value (none(l): cell l does not); L, -1 for a line without any
template <typename None>
__device__ __forceinline__ void edt_range(int L, None none, int &lmin, int &lmax) {
    lmin = 0;
    while (lmin < L && none(lmin)) ++lmin;
    lmax = L - 1;
    while (lmax > lmin && none(lmax)) --lmax;
    if (lmin == L) lmax = -1;
}

__device__ __forceinline__ unsigned edt_square16(unsigned v) { return v == EDT_NO16 ? EDT_NONE : v * v; }

template <int CELLS, int THREADS>
__global__ void __launch_bounds__(THREADS) k_edt_xy(EdtArgs a) {
    __shared__ unsigned short s_dx[CELLS];
    const int Gx = a.Gx, Gy = a.Gy, plane = Gx * Gy;
    const size_t base = (size_t)blockIdx.x * (size_t)plane;  // slice frame * Gz + k
    const unsigned char *o = a.occ + base;
    const bool invert = a.invert != 0;
    for (int j = threadIdx.x >> 6; j < Gy; j += THREADS / 64) {
        unsigned short *row = s_dx + j * Gx;
        const unsigned char *orow = o + (size_t)j * Gx;
        edt_row(Gx, a.border, [&](int i) { return (orow[i] != 0) != invert; }, [&](int i) { return (int)row[i]; },
                [&](int i, int v) { row[i] = (unsigned short)v; });
    }
    __syncthreads();
    // a row has a feature (or the border) or none: every column shows the same rows, and a slice the hull does not reach costs no search
    int jmin, jmax;
    const unsigned short *col = s_dx + threadIdx.x % Gx;
    edt_range(Gy, [&](int j) { return col[j * Gx] == EDT_NO16; }, jmin, jmax);
    for (int c = threadIdx.x; c < plane; c += THREADS) {
        const int j = c / Gx;
        const unsigned short *at = s_dx + c;
        a.d2[base + c] = (int)edt_search(j, Gy, jmin, jmax, a.border, edt_square16(at[0]), [&](int dl) { return edt_square16(at[dl * Gx]); });
    }
}

__global__ void __launch_bounds__(EDT_THREADS) k_edt_x(EdtArgs a) {
    const long long r = (long long)blockIdx.x * (EDT_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= a.rows) return;  // (the whole wave)
    const unsigned char *orow = a.occ + (size_t)r * a.Gx;
    int *row = a.d2 + (size_t)r * a.Gx;
    const bool invert = a.invert != 0;
    // the left sweep leaves distances, the right sweep reads them back (each lane its own) and leaves the squares
    const int lane = threadIdx.x & 63, Gx = a.Gx;
    edt_row(Gx, a.border, [&](int i) { return (orow[i] != 0) != invert; }, [&](int i) { return row[i]; }, [&](int i, int v) { row[i] = v; });
    for (int i = lane; i < Gx; i += 64) row[i] = (int)edt_square16((unsigned)row[i]);
}

struct EdtLineArgs {
    const int *src;
    int *dst;         // k_edt_line: == src
    long long ncol;   // columns, and the distance of a line's cells: Gx (y pass) or Gx Gy (z pass)
    int L;            // cells of a line: Gy or Gz
    long long chunks; // workgroups across the columns
    long long cells;  // N Gx Gy Gz (k_edt_line_far)
    int border;
};

template <int LINES, int THREADS>
__global__ void __launch_bounds__(THREADS) k_edt_line(EdtLineArgs a) {
    __shared__ unsigned s_f[LINES * EDT_COLS];
    const long long outer = (long long)(blockIdx.x / (unsigned long long)a.chunks), chunk = (long long)(blockIdx.x % (unsigned long long)a.chunks);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long col = chunk * EDT_COLS + lane;
    const bool live = col < a.ncol;
    int *line = a.dst + (size_t)outer * (size_t)a.ncol * (size_t)a.L + (size_t)col;
    for (int l = w; live && l < a.L; l += THREADS / 64) s_f[l * EDT_COLS + lane] = (unsigned)line[(size_t)l * (size_t)a.ncol];
    __syncthreads();
    int lmin = a.L, lmax = -1;
    if (live) edt_range(a.L, [&](int l) { return s_f[l * EDT_COLS + lane] == EDT_NONE; }, lmin, lmax);
    for (int l = w; live && l < a.L; l += THREADS / 64) {
        const unsigned *at = s_f + l * EDT_COLS + lane;
        line[(size_t)l * (size_t)a.ncol] = (int)edt_search(l, a.L, lmin, lmax, a.border, at[0], [&](int dl) { return at[dl * EDT_COLS]; });
    }
}

__global__ void __launch_bounds__(EDT_THREADS) k_edt_line_far(EdtLineArgs a) {
    const long long t = (long long)blockIdx.x * EDT_THREADS + threadIdx.x;
    if (t >= a.cells) return;
    const int l = (int)((t / a.ncol) % a.L);
    const int *at = a.src + t;
    a.dst[t] = (int)edt_search(l, a.L, 0, a.L - 1, a.border, (unsigned)at[0], [&](int dl) { return (unsigned)at[(long long)dl * a.ncol]; });
}

// ---- the sampler ------------------------------------------------------------------------------------------------------------
struct FieldArgs {
    HullGridDev g;
    const int *d2_out, *d2_in;
    const float *points;
    int dim;
    long long P, chunks;
    float *value, *grad;
};

struct FieldAxis {
    int i0, i1;
    double t, out;  // the weight of cell i1; u - clamp(u): how far outside the box of cell centres
    bool slope;     // the interpolation has a slope along this axis (not clamped, more than one cell)
};

__device__ __forceinline__ FieldAxis field_axis(double p, double origin, double voxel, int G) {
#pragma clang fp contract(off)
    const double u = (p - origin) / voxel - 0.5, top = (double)(G - 1);
    const double c = u < 0.0 ? 0.0 : (u > top ? top : u);
    FieldAxis a;
    a.i0 = G == 1 ? 0 : min((int)floor(c), G - 2);
    a.i1 = min(a.i0 + 1, G - 1);
    a.t = c - (double)a.i0;
    a.out = u - c;
    a.slope = a.out == 0.0 && G > 1;
    return a;
}

__device__ __forceinline__ double field_cell(const int *d2_out, const int *d2_in, size_t at) {
    const int o = d2_out[at];
    if (o == SMIL_EDT_NONE) return 0.0;  // no hull in this frame: no field, whatever d2_in says
    double r = sqrt((double)o);
    if (d2_in) {
        const int i = d2_in[at];
        r -= i == SMIL_EDT_NONE ? 0.0 : sqrt((double)i);
    }
    return r;
}

__device__ __forceinline__ double field_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    return (1.0 - t) * a + t * b;  // exactly a at t = 0 and b at t = 1
}

__global__ void __launch_bounds__(HULL_THREADS) k_field_sample(FieldArgs a) {
#pragma clang fp contract(off)
    const long long frame = (long long)(blockIdx.x / (unsigned long long)a.chunks), chunk = (long long)(blockIdx.x % (unsigned long long)a.chunks);
    const long long p = chunk * HULL_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const size_t o = (size_t)frame * (size_t)a.P + (size_t)p;
    const float *pt = a.points + (size_t)a.dim * o;
    // (x, y, z) of the point: a 2-D point is (y, x)
    const double px = (double)pt[a.dim == 2 ? 1 : 0], py = (double)pt[a.dim == 2 ? 0 : 1], pz = a.dim == 2 ? 0.0 : (double)pt[2];
    double value = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    if (isfinite(px) && isfinite(py) && isfinite(pz)) {
        const double *org = a.g.origin + 3 * (frame % a.g.n_origin);
        const double voxel = a.g.voxel[frame % a.g.n_voxel];
        const FieldAxis X = field_axis(px, org[0], voxel, a.g.Gx), Y = field_axis(py, org[1], voxel, a.g.Gy);
        FieldAxis Z = field_axis(pz, org[2], voxel, a.g.Gz);
        if (a.dim == 2) Z = FieldAxis{0, 0, 0.0, 0.0, false};
        const size_t base = (size_t)frame * (size_t)a.g.vox, sy = (size_t)a.g.Gx, sz = (size_t)a.g.Gx * (size_t)a.g.Gy;
        double c[2][2][2];
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    c[k][j][i] = field_cell(a.d2_out, a.d2_in, base + (size_t)(k ? Z.i1 : Z.i0) * sz + (size_t)(j ? Y.i1 : Y.i0) * sy + (size_t)(i ? X.i1 : X.i0));
        double v[2], dx[2], dy[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double a0 = field_lerp(c[k][0][0], c[k][0][1], X.t), a1 = field_lerp(c[k][1][0], c[k][1][1], X.t);
            v[k] = field_lerp(a0, a1, Y.t);
            dx[k] = field_lerp(c[k][0][1] - c[k][0][0], c[k][1][1] - c[k][1][0], Y.t);
            dy[k] = a1 - a0;
        }
        const double dist = sqrt(X.out * X.out + Y.out * Y.out + Z.out * Z.out);
        value = voxel * (field_lerp(v[0], v[1], Z.t) + dist);
        gx = X.slope ? field_lerp(dx[0], dx[1], Z.t) : 0.0;
        gy = Y.slope ? field_lerp(dy[0], dy[1], Z.t) : 0.0;
        gz = Z.slope ? v[1] - v[0] : 0.0;
        if (dist > 0.0) { gx += X.out / dist; gy += Y.out / dist; gz += Z.out / dist; }
    }
    a.value[o] = (float)value;
    if (!a.grad) return;
    float *g = a.grad + (size_t)a.dim * o;
    if (a.dim == 2) { g[0] = (float)gy; g[1] = (float)gx; }
    else { g[0] = (float)gx; g[1] = (float)gy; g[2] = (float)gz; }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static int check_edt_grid(const char *who, const SmilHullGrid *g, long long *vox) {
    if (int rc = check_hull_extent(who, g, vox)) return rc;
    const long long sx = (long long)g->Gx + 1, sy = (long long)g->Gy + 1, sz = (long long)g->Gz + 1;
    SMIL_REQUIRE(sx <= 46341 && sy <= 46341 && sz <= 46341 && sx * sx + sy * sy + sz * sz < (1LL << 31),
                 "%s: grid %d x %d x %d: squared distances exceed an int32", who, g->Gx, g->Gy, g->Gz);
    SMIL_REQUIRE(hull_chunks(*vox, EDT_COLS) + g->Gz <= 0x7FFFFFFFLL / g->N, "%s: N=%d frames of %lld voxels exceed the launch grid", who, g->N, *vox);
    return SMIL_OK;
}

static bool edt_fused(const SmilHullGrid *g) { return (long long)g->Gx * g->Gy <= EDT_MAX_SLICE; }
// a pass leaves its result in another buffer
static bool edt_needs_second(const SmilHullGrid *g) { return (!edt_fused(g) && g->Gy > EDT_MAX_LINE) || g->Gz > EDT_MAX_LINE; }

extern "C" size_t smil_hull_edt_workspace_bytes(const SmilHullGrid *g) {
    if (!hull_extent_ok(g)) return 0;
    Workspace ws{nullptr};
    ws.take<int>(edt_needs_second(g) ? (size_t)g->N * (size_t)g->Gx * (size_t)g->Gy * (size_t)g->Gz : 1);
    return ws.used;
}

static int edt_line_pass(int *&cur, int *&other, long long ncol, int L, long long outers, long long cells, int border, hipStream_t stream) {
    EdtLineArgs a{cur, cur, ncol, L, hull_chunks(ncol, EDT_COLS), cells, border};
    const dim3 grid((unsigned)(a.chunks * outers));
    // (more threads where a workgroup's LDS leaves room for fewer workgroups: 16 or more waves a CU at every size)
    if (L <= 32) hipLaunchKernelGGL((k_edt_line<32, 256>), grid, dim3(256), 0, stream, a);
    else if (L <= 128) hipLaunchKernelGGL((k_edt_line<128, 256>), grid, dim3(256), 0, stream, a);
    else if (L <= 256) hipLaunchKernelGGL((k_edt_line<256, 512>), grid, dim3(512), 0, stream, a);
    else if (L <= EDT_MAX_LINE) hipLaunchKernelGGL((k_edt_line<EDT_MAX_LINE, 1024>), grid, dim3(1024), 0, stream, a);
    else {
        a.dst = other;
        hipLaunchKernelGGL(k_edt_line_far, dim3((unsigned)hull_chunks(cells, EDT_THREADS)), dim3(EDT_THREADS), 0, stream, a);
        std::swap(cur, other);
    }
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_hull_edt(const SmilHullGrid *g, const uint8_t *occ, int32_t invert, int32_t border, int32_t *d2, void *workspace,
                             void *stream_) {
    long long vox;
    if (int rc = check_edt_grid("smil_hull_edt", g, &vox)) return rc;
    SMIL_REQUIRE(occ && d2 && workspace, "smil_hull_edt: null occ, d2 or workspace");
    hipStream_t stream = (hipStream_t)stream_;
    const long long plane = (long long)g->Gx * g->Gy, slices = (long long)g->N * g->Gz, cells = vox * g->N;
    SMIL_REQUIRE(hull_chunks(cells, EDT_THREADS) <= 0x7FFFFFFFLL, "smil_hull_edt: %lld voxels exceed the launch grid", cells);
    EdtArgs a{(const unsigned char *)occ, (int *)d2, g->Gx, g->Gy, invert != 0, border != 0, slices * g->Gy};
    int *cur = (int *)d2, *other = (int *)workspace;
    if (edt_fused(g)) {
        if (plane <= 4096) hipLaunchKernelGGL((k_edt_xy<4096, 256>), dim3((unsigned)slices), dim3(256), 0, stream, a);
        else if (plane <= 16384) hipLaunchKernelGGL((k_edt_xy<16384, 1024>), dim3((unsigned)slices), dim3(1024), 0, stream, a);
        else hipLaunchKernelGGL((k_edt_xy<EDT_MAX_SLICE, 1024>), dim3((unsigned)slices), dim3(1024), 0, stream, a);
        SMIL_LAUNCH_CHECK();
    } else {
        SMIL_REQUIRE(hull_chunks(a.rows, EDT_THREADS / 64) <= 0x7FFFFFFFLL, "smil_hull_edt: %lld rows exceed the launch grid", a.rows);
        hipLaunchKernelGGL(k_edt_x, dim3((unsigned)hull_chunks(a.rows, EDT_THREADS / 64)), dim3(EDT_THREADS), 0, stream, a);
        SMIL_LAUNCH_CHECK();
        if (g->Gy > 1 || a.border)  // (a line of one cell still has the border's cells -1 and 1 beside it)
            if (int rc = edt_line_pass(cur, other, g->Gx, g->Gy, slices, cells, a.border, stream)) return rc;
    }
    if (g->Gz > 1 || a.border)
        if (int rc = edt_line_pass(cur, other, plane, g->Gz, g->N, cells, a.border, stream)) return rc;
    if (cur != (int *)d2) SMIL_HIP(hipMemcpyAsync(d2, cur, (size_t)cells * sizeof(int), hipMemcpyDeviceToDevice, stream));
    return SMIL_OK;
}

extern "C" int smil_field_sample(const SmilHullGrid *g, const int32_t *d2_out, const int32_t *d2_in, const float *points, int32_t point_dim,
                                 int64_t P, float *value, float *grad, void *workspace, void *stream_) {
    long long vox;
    if (int rc = check_hull_grid("smil_field_sample", g, true, &vox)) return rc;
    SMIL_REQUIRE(point_dim == 2 || point_dim == 3, "smil_field_sample: point_dim=%d outside {2, 3}", point_dim);
    SMIL_REQUIRE(point_dim == 3 || g->Gz == 1, "smil_field_sample: point_dim=2 needs Gz=1, got %d", g->Gz);
    SMIL_REQUIRE(P >= 0, "smil_field_sample: P=%lld points", (long long)P);
    FieldArgs a;
    a.chunks = hull_chunks(P, HULL_THREADS);
    SMIL_REQUIRE(a.chunks <= 0x7FFFFFFFLL / g->N, "smil_field_sample: N=%d frames of %lld points exceed the launch grid", g->N, (long long)P);
    SMIL_REQUIRE(d2_out && points && value && workspace, "smil_field_sample: null d2_out, points, value or workspace");
    if (P == 0) return SMIL_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = hull_upload(hull_layout(workspace, g, 0), g, vox, 1, &a.g, stream)) return rc;
    a.d2_out = d2_out; a.d2_in = d2_in; a.points = points; a.dim = point_dim; a.P = P; a.value = value; a.grad = grad;
    hipLaunchKernelGGL(k_field_sample, dim3((unsigned)(a.chunks * g->N)), dim3(HULL_THREADS), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
