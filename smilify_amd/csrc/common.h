// Shared internals of libsmilfit (gfx950).  Not installed; the public surface is include/smilfit.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "smilfit.h"

#define WAVE 64
#define BONE_WAVES 8  // waves of the workgroup that walks a frame's bone lists (k_lbs_bwd_ndc: 512 threads)

void smil_set_error(const char *fmt, ...);

#define SMIL_HIP(expr)                                                                              \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            smil_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return SMIL_E_DEVICE;                                                                   \
        }                                                                                           \
    } while (0)

#define SMIL_REQUIRE(cond, ...)              \
    do {                                     \
        if (!(cond)) {                       \
            smil_set_error(__VA_ARGS__);     \
            return SMIL_E_INVALID;           \
        }                                    \
    } while (0)

#define SMIL_LAUNCH_CHECK()                                                                        \
    do {                                                                                            \
        hipError_t _e = hipGetLastError();                                                          \
        if (_e != hipSuccess) {                                                                     \
            smil_set_error("%s:%d: kernel launch failed: %s", __FILE__, __LINE__, hipGetErrorString(_e)); \
            return SMIL_E_DEVICE;                                                                   \
        }                                                                                           \
    } while (0)

// Device-resident model constants.
struct SmilModel {
    int V = 0, F = 0, J = 0, nB = 0;
    int max_depth = 0;
    int max_valence = 0;          // most faces sharing one vertex (bounds the gradient a vertex can receive: k_raster_setup's img_bound)
    bool static_joints = false;
    int jreg_nnz = 0;
    int bone_nnz = 0;
    float *v_template = nullptr;  // (V,3)
    float *shapedirs = nullptr;   // (nB,3V)
    int *faces = nullptr;         // (F,3)
    int *parents = nullptr;       // (J)
    int *depth = nullptr;         // (J)
    uint32_t *skin_idx = nullptr; // (V) four u8 bone ids packed little-endian
    float4 *skin_w = nullptr;     // (V)
    int *jreg_rowptr = nullptr;   // CSR by joint
    int *jreg_col = nullptr;
    float *jreg_val = nullptr;
    int *jreg_colptr = nullptr;   // CSC by vertex (V+1)
    int *jreg_row = nullptr;      // joint ids
    float *jreg_cval = nullptr;
    int2 *jreg_vfirst = nullptr;  // (V) the first CSC entry of every vertex inline: {joint | entries << 16, weight bits} (most have <= 1)
    int *bone_ptr = nullptr;      // skin weights by bone (J+1)
    int *bone_vid = nullptr;
    float *bone_w = nullptr;
    float *J_static = nullptr;    // (J,3)
    float *jreg_shape = nullptr;  // (nB,J,3) = J_regressor @ shapedirs[k]: d beta through the rest joints without a pass over the vertices
    int *bone_order = nullptr;    // (bone_slots) the bone lists dealt to BONE_WAVES waves, longest processing time first: slot w + k BONE_WAVES
                                  // is wave w's k-th bone, -1 behind its last
    int bone_slots = 0;
    float *posedirs = nullptr;    // (9(J-1),3V) or null
    int *vf_ptr = nullptr;        // (V+1) vertex -> face CSR: the faces of vertex v are vf_face[vf_ptr[v] .. vf_ptr[v+1]), ascending
    int *vf_face = nullptr;       // (3F)   (per-frame vertex normals of the colour path, shade.hip: a fixed-order gather, no atomics)
    std::vector<void *> allocations;
};

// What the colour path (shade.hip) takes from the rasteriser's setup kernel (raster.hip), run with blur 0: per-face tile boxes and
// depth ranges, the binned per-tile face lists, the touched-tile work items and the clip tables of faces cut at z_clip.
struct ColourSetup {
    const uint32_t *tbox;     // (N, FT) tile box of every face (4 x u8: tx0, ty0, tx1, ty1; empty when tx0 > tx1)
    const uint32_t *gbox;     // (N, FT / 64) union of the boxes of 64 consecutive faces (tiles whose list was not binned)
    const float2 *fzr;        // (N, FT) nearest / farthest vertex depth
    const uint4 *items;       // work items {image * tiles + tile, first list entry, entries (0xFFFFFFFF: not binned), -}
    const uint32_t *n_class;  // (n_parts, n_classes) items per partition and cost class (device)
    uint32_t *ticket;         // dealing counter, zero at the start of the call
    uint32_t item_cap;        // entries of one item array of one partition
    const uint2 *lists;       // (N, list_cap) {face id, bits of its nearest vertex depth}
    uint32_t list_cap;
    const float *xv;          // (N, clip_vx, 3) new vertices of cut faces (x_ndc, y_ndc, z_clip)
    const int *xf;            // (N, clip_fx, 3) vertex ids of the front parts (>= V: new vertices)
    const int2 *xsrc;         // (N, clip_vx) end points of the edge a new vertex lies on
    const int *xparent;       // (N, clip_fx / 2) the face a cut belongs to
    int FT, FP, clip_vx, clip_fx, n_parts, n_classes;
};
size_t smil_colour_setup_bytes(const SmilModel *m, int N, int S);
int smil_colour_setup(const SmilModel *m, const float *verts_ndc, int N, int S, float z_clip, void *workspace, hipStream_t stream,
                      ColourSetup *out);

// the two paths share the setup kernel's 8x8-pixel tiles and its pixel centres (pixel index i of a flipped axis, S pixels)
constexpr int TILE = 8;
__device__ __forceinline__ float pix_to_ndc(int i, int S) { return -1.0f + (2.0f * (float)i + 1.0f) / (float)S; }

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- argument checks the multi-view entry points share (triangulate.hip, refine.hip, refine_points.hip); SMIL_OK or the error set ----
// (`why`: what the caller keeps in the ONE wave that holds a problem's C views)
static inline int smil_check_views(const char *who, int32_t C, const char *why) {
    if (C > SMIL_TRI_MAX_VIEWS) {
        smil_set_error("%s: C=%d above SMIL_TRI_MAX_VIEWS=%d (%s)", who, C, SMIL_TRI_MAX_VIEWS, why);
        return SMIL_E_UNSUPPORTED;
    }
    return SMIL_OK;
}
static inline int smil_check_grid(const char *who, int64_t N, int32_t Kp, int waves) {
    SMIL_REQUIRE(Kp == 0 || N <= (int64_t)0x7FFFFFFF * waves / Kp, "%s: N Kp = %lld x %d problems exceed the grid", who, (long long)N, Kp);
    return SMIL_OK;
}
static inline int smil_check_f_scale(const char *who, double f_scale) {
    SMIL_REQUIRE(f_scale > 0.0 && std::isfinite(f_scale), "%s: f_scale=%g must be positive and finite", who, f_scale);
    return SMIL_OK;
}

// (project.hip) the camera argument of every entry point that takes one.  frames != 0: the cameras are those of `frames` frames
// x cam->views views (a negative count fails: the caller's own argument was missing)
int check_cameras(const SmilCameras *cam, const char *who, int frames = 0);

// frames of the window that holds local frame `local_frame` (the last one may be short): a frame's loss terms are divided by it
__device__ __forceinline__ int window_size_of(const SmilFitConfig &c, int local_frame) {
    const int gi = c.frame0 + local_frame;
    const int w = c.window > 0 ? c.window : c.N_total;
    const int start = (gi / w) * w;
    return min(w, c.N_total - start);
}

// ---- caller-owned workspaces: every region starts on a 256-byte boundary ----
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Bump allocator over a workspace.  An entry point's ONE layout function takes its regions in order from it: with a null base it
// only adds up their sizes (the *_workspace_bytes functions), with the caller's buffer it carves them.
struct Workspace {
    char *base;       // null: size only
    size_t used = 0;  // bytes taken so far: the total once the layout is done
    template <class T> T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += align256(count * sizeof(T));
        return p;
    }
};

// Compute units and LDS per workgroup (on MI355X all 160 KB of a CU) of the current device, asked once per device (model.hip: one
// mutex-guarded table of SMIL_MAX_DEVICES entries).  256 CUs and 64 KB when the device cannot be asked.
#define SMIL_MAX_DEVICES 16
struct DeviceLimits { int cus; size_t lds_block; };
DeviceLimits smil_device_limits();

// ---- wave-level helpers (wave64) --------------------------------------------------------------
// The value of lane `lane` (wave-uniform) in every lane.
__device__ __forceinline__ int read_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float read_lane(float v, int lane) { return __builtin_bit_cast(float, read_lane(__builtin_bit_cast(int, v), lane)); }
__device__ __forceinline__ unsigned long long read_lane(unsigned long long v, int lane) {
    const uint32_t lo = (uint32_t)read_lane((int)(uint32_t)v, lane), hi = (uint32_t)read_lane((int)(uint32_t)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// Sum over the 64 lanes using DPP within rows of 16 and readlane across rows; result valid in all lanes.
__device__ __forceinline__ float wave_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));  // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)); // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)); // row_mirror
    const int iv = __builtin_bit_cast(int, v);  // (one cast, not four read_lane calls: those schedule lbs.hip's kernels differently)
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return (r0 + r1) + (r2 + r3);
}

// Sum over each row of 16 lanes (four independent sums per wave); result valid in every lane of the row.
__device__ __forceinline__ float row_sum16(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));  // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)); // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)); // row_mirror
    return v;
}

// Every other fold over the 64 lanes is ONE xor butterfly: op(own value, the partner's).  Both partners of an exchange combine the
// same two numbers, so every lane ends with the same bits and the result depends on nothing but the values (the float64 sum of
// triangulate.hip relies on it).  wave_sum(float) above is not one of them: its DPP order defines its bits.
template <class T, class Op> __device__ __forceinline__ T wave_fold(T v, Op op) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) { return wave_fold(v, [](int a, int b) { return a + b; }); }
__device__ __forceinline__ long long wave_sum(long long v) { return wave_fold(v, [](long long a, long long b) { return a + b; }); }
__device__ __forceinline__ double wave_sum(double v) { return wave_fold(v, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ int wave_min(int v) { return wave_fold(v, [](int a, int b) { return min(a, b); }); }
__device__ __forceinline__ long long wave_min(long long v) { return wave_fold(v, [](long long a, long long b) { return b < a ? b : a; }); }
__device__ __forceinline__ float wave_max(float v) { return wave_fold(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ int wave_max(int v) { return wave_fold(v, [](int a, int b) { return max(a, b); }); }
__device__ __forceinline__ long long wave_max(long long v) { return wave_fold(v, [](long long a, long long b) { return b > a ? b : a; }); }
__device__ __forceinline__ double wave_max(double v) { return wave_fold(v, [](double a, double b) { return fmax(a, b); }); }

// inclusive sum over the lanes up to and including this one
template <class T> __device__ __forceinline__ T wave_scan_inclusive(T v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const T w = __shfl_up(v, o, 64);
        if (lane >= o) v += w;
    }
    return v;
}

// the value of a lane, float64 (triangulate.hip)
__device__ __forceinline__ double read_lane(double v, int lane) {
    return __builtin_bit_cast(double, read_lane(__builtin_bit_cast(unsigned long long, v), lane));
}

// Block-wide sum for blocks of up to 1024 threads; result valid in thread 0 (and all threads of wave 0).
__device__ __forceinline__ float block_sum(float v, float *smem /* >= 16 floats */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) smem[wid] = v;
    __syncthreads();
    float r = 0.f;
    if (wid == 0) {
        r = lane < nw ? smem[lane] : 0.f;
        r = wave_sum(r);
    }
    return r;
}

// Sums of up to TWELVE values per lane over the 64 lanes in 30 instructions (twelve wave_sum calls: 130).  gfx950's
// v_permlane32_swap / v_permlane16_swap exchange half-waves / odd and even 16-lane rows between two registers, so one swap and
// one add fold a PAIR of values to half the lanes each: 12 values -> 6 registers (component i in lanes 0-31, i + 6 in lanes
// 32-63) -> 3 registers (rows hold components i, i + 3, i + 6, i + 9), then four DPP adds inside the rows.
// On return every lane of row r (lanes 16 r .. 16 r + 15) holds the sum of component i + 3 r in q[i], i = 0 .. 2.
// (spelled in assembly: with the __builtin_amdgcn_permlane*_swap builtins hipcc 7.2 adds the FIRST result to itself - it loses the
// second, in-place updated operand; tools/dbg/sum12_test.hip checks this function against a serial sum)
__device__ __forceinline__ float swap32_add(float a, float b) {  // lanes 0-31: a[l] + a[l + 32]; lanes 32-63: b[l - 32] + b[l]
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}
__device__ __forceinline__ float swap16_add(float a, float b) {  // rows 0, 2: a's row + a's next row; rows 1, 3: b's previous row + b's row
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libsmilfit is written for gfx950 (MI355X) only: v_permlane32_swap / v_permlane16_swap and the tile kernel's LDS and register budgets have no other target"
#endif
__device__ __forceinline__ void wave_sum12(const float (&v)[12], float (&q)[3]) {
    float h[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) h[i] = swap32_add(v[i], v[i + 6]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float x = swap16_add(h[i], h[i + 3]);
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true));  // row_half_mirror
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true));  // row_mirror
        q[i] = x;
    }
}

// ---- order-independent scatter sums: int64 fixed point with a unit that follows the data (mesh3d.hip, pointnet2.hip) ----
// A gradient that many threads add into one element is summed as integers: no float atomics, and the result does not depend on the
// order of the additions.  The unit 2^-fix is a power of two per segment (a mesh and direction, a mesh, a cloud).  A first pass
// leaves the bits of the segment's largest magnitude with an atomicMax (magnitudes are >= 0: their bits order like the values, and
// a maximum does not depend on the order either).  With every |addend| < 2^eb and fewer than 2^pb addends meeting in one element,
// fix = 61 - pb - eb keeps the sum, roundings included, below 2^62 whatever the data's extent (a fixed 2^-32 lost the gradient
// of clouds whose extent is far below 1), and scaling the data by a power of two scales the result exactly.

// eb with m < 2^eb for a recorded maximum m, from its bits
__device__ __forceinline__ int fix_max_exp(unsigned int max_bits) {
    int ex;
    frexpf(fminf(__uint_as_float(max_bits), 3.0e38f), &ex);  // (non-finite input: any finite unit)
    return ex;
}
// fix for |addend| < 2^eb and at most `addends` (>= 1, < 2^pb) addends per element
__device__ __forceinline__ int fix_unit_exp(int eb, long long addends) { return 61 - (64 - __clzll(addends)) - eb; }
__device__ __forceinline__ void fix_add(long long *acc, double v, int fix) {
    atomicAdd((unsigned long long *)acc, (unsigned long long)__double2ll_rn(ldexp(v, fix)));
}
__device__ __forceinline__ float fix_read(long long acc, int fix) { return (float)ldexp((double)acc, -fix); }
// the first pass: the wave's largest m (>= 0) into the segment's slot, zeroed before the launch
__device__ __forceinline__ void fix_record_max(unsigned int *slot, float m) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(slot, __float_as_uint(m));
}

// ---- FoV-perspective camera of an image: parameters, projection forward and backward (project.hip, lbs.hip) ----
#include "camera.h"
