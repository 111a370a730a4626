// What more than one kernel of the rasteriser uses (raster.hip; see the map of the headers there): the tile and record constants,
// the argument structures, the clip tables, the stream addressing, the wave helpers and the per-(pixel, face) arithmetic that the tile
// kernel and k_raster_tie_replay must evaluate to the same bits.  Included by raster.hip only, behind common.h and raster_hooks.h.
#pragma once

// the rounded blur box: which tiles, rows and columns of a face's pixel box can hold a record (k_raster_setup, stage_faces)
#define REACH_FN __host__ __device__ __forceinline__
#include "raster_reach.h"

#define DCHUNK 32           // faces staged per chunk
#define FREC 28             // floats per staged face record
#define FSTR 28             // its stride in LDS: 112 bytes = 28 banks, so the 16-byte rows of 16 consecutive faces start in 16 different
                            // bank quads (a 128-byte stride would put the same row of every face in the same banks)
#define K_EPS 1e-8f
#define ALPHA_GRAD_EPS 1e-12f  // pixels whose transmittance is below this contribute no gradient
#ifndef SEL_BITS
#define SEL_BITS 5
#endif
//      SEL_BITS            // radix-select digit width (two 16-bit counts per LDS word, 16 words per pixel)
#ifndef SEL1_BITS
#define SEL1_BITS 6
#endif
//      SEL1_BITS           // width of the FIRST digit, the one pass 1 counts and the closing rule works with: 64 buckets in the same
                            // 16 words per pixel as four 8-bit counts that stop at SAT8 (a count only ever matters up to K <= 128)
#define SAT8 160u           // a byte takes no further increment from here on; at most 63 more arrive with the instruction that crosses it
#ifndef DGROUP
#define DGROUP 4            // 64-record rows per buffer in the dense walks (two buffers)
#endif
#ifndef KGROUP
#define KGROUP 4            // 64-key rows per buffer in the selection sweeps (two buffers)
#endif
#ifndef SELR
#define SELR 6              // compact records a lane holds once the selection runs in registers (the stream is then at most SELR * 64 long)
#endif
#ifndef LIST_LDS_ROWS
#define LIST_LDS_ROWS 8     // 64-entry rows of a binned tile list that the list phase keeps in LDS (longer lists: read three times from memory)
#endif
#ifndef REC_CAP
#define REC_CAP 65536       // pair records one (sub-)tile may produce
#endif
#define REC_PAD 64          // slack so that a clamped read stays inside the allocation
#ifndef RESIDENT_PER_CU
#define RESIDENT_PER_CU 16
#endif
//      RESIDENT_PER_CU     // single-wave workgroups per CU: what 128 VGPRs and 9.9 KB of LDS per workgroup allow (measured 10 ... 14: every
                            // further workgroup still shortens the launch)

#ifndef WAVES_PER_SIMD
#define WAVES_PER_SIMD 4     // what the tile kernel's register budget is set for: RESIDENT_PER_CU / 4
#endif
enum { MODE_FWD = 0, MODE_BWD = 1, MODE_FUSED = 2 };

// Work items (touched tiles) are queued in four cost classes by the number of (face, pixel) pairs the tile will evaluate
// (the sum of its faces' pixel boxes), and handed out heaviest class first: a persistent kernel whose longest items take
// a fifth of the whole launch must not start them last.
// Per partition two arrays of ceil(N / N_PARTS) * tiles entries hold two classes each (one filled from the front, one
// from the back).
#define N_CLASSES 4
#ifndef PACKED_MIN_IMAGES
#define PACKED_MIN_IMAGES 64  // from this many images per launch the fused entry point packs its gradient atomics (see image_fx_scale)
#endif
#ifndef CLASS_T0
#define CLASS_T0 65536        // class 0 can be dealt out in pieces (SPLIT0_LOG)
#endif
#define CLASS_T1 16384
#define CLASS_T2 4096
#ifndef SPLIT0_LOG
#define SPLIT0_LOG 0          // log2 of the pieces every class-0 tile is dealt out in (0: whole; with near-to-far lists and closing the
#endif                        // tiles with the longest lists finish early, and pieces only repeat their list walk: measured 2 -> 0: mouse -9 %)
#define COUNT_TILES_MAX 4096  // per-tile cost / entry counts and list cursors live in LDS (12 bytes per tile); larger images (S > 512) queue
                              // everything in the last class and build their lists in the tile kernel
// XCD-aware dealing.  Each of the 8 XCDs of an MI355X has its own 4 MB L2, and the tiles of one image read the same
// per-image tables (projected vertices, face tile boxes, depth ranges: ~180 KB on STICK).  Images are therefore dealt to
// N_PARTS work-list partitions (image % N_PARTS); a workgroup drains the partition of the XCD it runs on first
// (HW_REG_XCC_ID - placement is whatever the dispatcher chose, only speed depends on it) and then helps the others, so an
// image's tables are fetched into one L2 instead of eight while the launch is busy, and the tail still balances.
#define N_PARTS 8
struct RasterCounters {
    unsigned int n_class[N_PARTS][N_CLASSES];
    struct { unsigned int next, pad[15]; } deal[N_PARTS];  // one cache line per partition's cursor
    unsigned int straddling;  // faces that cross z_clip in this launch: cut at the plane (smil_raster_stats) ...
    unsigned int unclipped;   // ... except these: beyond the per-image clip tables, rendered whole or dropped
    unsigned int tie_pixels;  // (tie_rule 1) pixels left to k_raster_tie_replay
    unsigned int tie_next;    // ... and its ticket counter
};

// The tile kernel's dealing policy, shared by the kernel and the host: with fewer tiles than workgroup slots every tile is dealt out
// as 2, 4 or 8 runs of pixels (round 4, from a sweep over 1 ... 64 images x workgroups per CU x pieces, profiles/r4_small_launches.txt:
// the launch is fastest with ~2.3 pieces per WORKING workgroup and about 1.2 pieces per resident slot in all), and only
// max(slots / 8, pieces x 7 / 16) workgroups take part.
__host__ __device__ __forceinline__ unsigned int deal_split_log(unsigned int n_items, unsigned int slots) {
    return n_items * 8u <= slots * 5u / 8u ? 3u : (n_items * 4u <= slots * 5u / 4u ? 2u : (n_items * 2u <= slots * 5u / 4u ? 1u : 0u));
}
__host__ __device__ __forceinline__ unsigned int deal_working(unsigned int n_items, unsigned int split_log, unsigned int slots) {
    const unsigned int w = (n_items << split_log) * 7u / 16u;
    return w > slots / 8u ? w : slots / 8u;
}

struct Rec3 { uint32_t a, b, c; };  // one 12-byte record: loaded / stored as one dwordx3
// Per list position of the current tile, left by pass 1 (which has them in registers) for pass 3: the face's projected vertices
// and its vertex ids.  Pass 3 used to fetch them per group of 64 faces through the chain list -> face -> vertex: three dependent
// memory round trips per group and 28 % of pass 3 (profiles/r4_pass3_timers.txt).  Vertices as three float2 arrays, see stage_faces.
struct TriIds { int a, b, c; };

// clip_faces (pytorch3d renderer/mesh/clip.py, as MeshRasterizer applies it with z_clip_value = znear / 2; the reference leaves that
// default on, p3d_renderer.py:36-47): a face with one or two vertices nearer than z_clip is cut at the plane and its front part
// (one triangle, or a quadrilateral as two) rendered instead.  Such faces are rare (the mesh must reach the camera), so they are
// handled beside the mesh, per image: up to CLIP_FX front-part triangles get face ids from FP = F rounded up to 64 on, their
// new vertices (on the plane) vertex ids from V on, both in small side tables; every fetch of a face's vertex indices or of a
// vertex's coordinates / gradient row goes through one compare that picks the table.  A new vertex is
// c_a xy[a] + c_b xy[b] of the cut edge's end points (interpolated in view space); its gradient goes back to them with the
// coefficients held constant (k_clip_backward).  Faces beyond the tables' capacity are rendered as before and counted.
#define CLIP_CUTS 1024           // cut faces per image (ONE capacity: each owns two front-part triangle slots and two new-vertex slots;
                                 // round 4: 256 -> 1024 - with the camera inside the 17 420-face mouse a third of the fuzzed scenes had exceeded 256)
#define CLIP_FX (2 * CLIP_CUTS)  // front-part triangles per image
#define CLIP_VX (2 * CLIP_CUTS)  // new vertices per image
struct ClipTables {
    float *xv;          // (N, CLIP_VX, 3) new vertices (x_ndc, y_ndc, z_clip)
    int *xf;            // (N, CLIP_FX, 3) vertex ids of the front-part triangles (>= V: new vertices)
    int2 *xsrc;         // (N, CLIP_VX) end points (a, b) of the edge a new vertex lies on
    float2 *xcoef;      // (N, CLIP_VX) (c_a, c_b)
    float *xg;          // (N, CLIP_VX, 2) gradient rows of the new vertices (same representation as d_ndc)
    uint32_t *xcount;   // (N) new vertices of the image
    int *xparent;       // (N, CLIP_CUTS) the face cut c belongs to, or NULL (only the colour path asks: smil_colour_setup)
};
__host__ __device__ __forceinline__ int faces_padded(int F) { return (F + WAVE - 1) / WAVE * WAVE; }
// vertex ids of face f of image n / coordinates of vertex i of image n, through the clip tables
__device__ __forceinline__ int face_vertex(const int *__restrict__ faces, const int *__restrict__ xf_n, int F, int f, int k) {
    return f < F ? faces[3 * f + k] : xf_n[3 * (f - faces_padded(F)) + k];
}
__device__ __forceinline__ const float *vertex_ptr(const float *__restrict__ vn, const float *__restrict__ xv_n, int V, int i) {
    return i < V ? vn + 3 * i : xv_n + 3 * (i - V);
}

struct RasterArgs {
    const float *verts_ndc;  // (N,V,3)
    const int *faces;        // (F,3)
    const uint32_t *tbox;    // (N,F) tile box of every face
    const uint32_t *gbox;    // (N, ceil(F/64)) union of the tile boxes of 64 consecutive faces
    const uint4 *items;      // work lists of {tile code, first list entry, entries (0xFFFFFFFF: build the list here), depth extent of the
                             // image's deepest face}, per partition q at 2 q cap: [0, cap) classes 0 (front) / 1 (back), [cap, 2 cap) classes 2 / 3
    uint32_t item_cap;       // entries of one array of ONE partition: ceil(N / N_PARTS) * tiles
    const float2 *fzr;       // (N,F) nearest / farthest vertex depth of every face
    RasterCounters *ctr;
    int N, V, F, S, tiles_x, K;
    int FT;                  // rows of the per-image face tables: F rounded up to 64 + CLIP_FX (front parts of cut faces)
    ClipTables clip;
    float blur, sqrt_blur, inv_sigma, inv_sigma_log2e;
    // outputs / inputs per mode
    float *sil;              // (N,S,S) FWD (or optional in FUSED)
    const float *grad_sil;   // BWD
    const float *target;     // FUSED (fp32 targets) ...
    const uint8_t *target_u8; // ... or binary {0,1} targets stored as bytes
    const float *pix_scale;  // FUSED (N,)
    const float *img_bound;  // (N,) setup kernel: 0.4 x valence x largest face box (pixels), the geometric part of the bound on a vertex's gradient
    int packed;              // FUSED: d_ndc is accumulated as (x, y) fixed point packed in 64 bits (one memory-side atomic per vertex, not two)
    float *loss_img;         // FUSED (N,)
    unsigned long long *loss_acc;  // FUSED (N,) the tiles' loss terms as 2^-32 fixed point: integer adds, the same bits in any order of
                             // arrival (round 5; a float atomic per tile before); k_clip_backward adds the sum to loss_img afterwards
    float *d_ndc;            // (N,V,2)
    // scratch per resident workgroup
    const uint2 *lists;      // (N, list_cap) tile lists binned by the setup kernel: {face id, bits of its nearest vertex depth}
    uint32_t list_cap;
    uint2 *slist;            // the current tile's faces when it builds its list itself (ascending id; same entry layout) ...
    uint32_t *slist2;        // ... and the ids the tile walks: near to far by the first radix digit of that depth when the tile may
                             // truncate (the sort reads the depths it needs from slist instead of gathering them per face)
    uint32_t *scfirst;       // F / DCHUNK + 2: first record of every chunk from the 128th on (the others live in registers)
    float2 *sxy;             // (3, list_stride) projected vertices v0 / v1 / v2 of the tile's faces by list position ...
    TriIds *sid;             // (list_stride) ... and their vertex ids
    // record streams, REC_CAP + REC_PAD entries each (structure of arrays: every sweep reads only what it needs)
    // pair records, 12 bytes each in ONE stream per workgroup (an append or a sweep step then touches one contiguous run of
    // memory instead of three): {depth bits, pixel | list position << 6 | inside << 22 | closest edge << 23, signed squared
    // distance to the closest edge (pass 3 recomputes the closest point itself)}
    Rec3 *srec;
    // records that survive the first selection digit: {key = depth bits - tile minimum, meta, log2 of the blend factor}
    Rec3 *crec;
    int list_stride, n_cf;   // entries of slist / scfirst per workgroup
    unsigned int slots;      // resident workgroup slots of the device (the dealing policy's yardstick; gridDim.x <= slots)
    SmilClipDepth cd;        // where k_clip_backward leaves the depth gradients of cut edges' end points (range == NULL: nowhere)
    int image0;              // index of the call's first image in the caller's batch (cd.range)
    int tie_rule;            // SmilRasterSettings.tie_rule (0: K smallest by (depth, face id); 1: the reference's queue, k_raster_tie_replay)
    unsigned long long *tie_mask;  // tie_rule 1: per work item (same index as `items`) the pixels of the tile whose K-th depth is a
                             // tie group that K cuts through: left out by the tile kernel, rendered by k_raster_tie_replay
    HOOK_ARGS_FIELDS         // (instrumented builds: counter buffer, cut-off phase, forced split)
};

// centre of tile column / row t (output order: column xo holds pixel index S - 1 - xo): what a tile's face records are relative to
__device__ __forceinline__ float tile_centre(int t, int S) { return pix_to_ndc(S - 1 - (t * TILE + TILE / 2), S); }

__device__ __forceinline__ float edge_fn(float px, float py, float ax, float ay, float bx, float by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// Packed gradient accumulation (fused entry point, large launches).  The flush of pass 3 goes to memory-side atomics (the
// per-XCD L2s forward every atomic), whose cost is proportional to their number: (x, y) of a vertex travel as two 32-bit
// fixed-point numbers in ONE 64-bit integer atomic instead of two float atomics.  The scale is a power of two per image,
// chosen so that no vertex component can overflow: |sum| <= img_bound * |pix_scale| / sqrt(sigma) (see k_raster_setup) maps into
// [2^29, 2^30].  Integer sums are order independent: the gradient becomes reproducible bit for bit.  k_unpack_dndc turns the
// buffer into the (N,V,2) floats the interface promises, in place.
__device__ __forceinline__ float image_fx_scale(float img_bound, float pix_scale, float inv_sigma) {
    const float bound = img_bound * fabsf(pix_scale) * sqrtf(inv_sigma);
    return (bound > 0.f && bound < 3.0e38f) ? exp2f(fminf(29.0f - floorf(log2f(bound)), 100.0f)) : 0.f;
}

// Element i of a per-workgroup stream: uniform base pointer + 32-bit byte offset, which hipcc turns into the SGPR-base /
// VGPR-offset form of the global load / store (a 64-bit address per lane costs two extra VALU instructions per access).
// (12-byte elements: the index must be below 2^24, so that the full-rate 24-bit multiply is exact; left to itself hipcc emits the
// quarter-rate v_mul_lo_u32, also for the shift-and-add spelling.  ONLY for per-workgroup / per-image arrays whose length the
// host bounds - REC_CAP + REC_PAD records, list_stride entries, both checked in raster_common(), raster.hip's host side.  An array
// whose index grows with the number of images must not come through here: a round-4 experiment stored its 12-byte work items
// this way, the index reaches 16 * ceil(N / 8) * tiles = 18.9e6 > 2^24 at 2 304 images @512^2, partition 7's items landed 2^24 elements early and the
// tile kernel read stale words as work items - the GPU abort of gpurun_out/r4/tests_itb.txt, DESIGN.md section 8.  The shipped
// work items are 16 bytes and plainly indexed.)
template <typename T>
__device__ __forceinline__ uint32_t byte_offset(uint32_t i) {
    if (sizeof(T) == 12) {
        uint32_t r;
        asm("v_mul_u32_u24 %0, %1, 12" : "=v"(r) : "v"(i));
        return r;
    }
    return i * (uint32_t)sizeof(T);
}
template <typename T>
__device__ __forceinline__ T &at(T *base, uint32_t i) {
    i = HOOK_WRAP_IDX(i);
    return *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_offset<T>(i));
}
template <typename T>
__device__ __forceinline__ const T &at(const T *base, uint32_t i) {
    i = HOOK_WRAP_IDX(i);
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_offset<T>(i));
}

// The lane index as a value the compiler cannot trace back to threadIdx.x: what is derived from it (an LDS address, a table offset) is
// recomputed where it is used, an instruction or two, and not kept for the whole kernel in a register that then spills.
__device__ __forceinline__ int opaque_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// inclusive wave64 prefix sum in DPP (row_shr within 16-lane rows, then row_bcast across rows)
__device__ __forceinline__ int wave_scan_add(int x) {
#define SCAN_STEP(ctrl, rows) { x += __builtin_amdgcn_update_dpp(0, x, ctrl, rows, 0xF, false); }
    SCAN_STEP(0x111, 0xF) SCAN_STEP(0x112, 0xF) SCAN_STEP(0x114, 0xF) SCAN_STEP(0x118, 0xF)
    SCAN_STEP(0x142, 0xA) SCAN_STEP(0x143, 0xC)
#undef SCAN_STEP
    return x;
}

// The record sweeps hold a buffer of N rows of 64 records; the buffer that meets the end of its range holds fewer.  A row body asks
// rows.has(u) before it touches row u, in its gather phase and again in its arithmetic: for a full buffer (RowsAll) that folds away
// and the body is the straight-line code it always was; for the last buffer (RowsUpto) it is a scalar branch per row and phase - the
// ranges are scalars, so the count is wave-uniform - and the rows behind the end cost nothing.
struct RowsAll { __device__ constexpr bool has(int) const { return true; } };
struct RowsUpto { int n; __device__ bool has(int u) const { return u < n; } };
static_assert(WAVE == 64, "rows_upto shifts by log2(WAVE)");
__device__ __forceinline__ int rows_upto(int g0, int end) { return (end - g0 + WAVE - 1) >> 6; }  // rows that the records [g0, end) touch
// Double-buffered sweep over the records [beg, end), beg < end, N rows per buffer; the caller has requested load(ra, beg).  While a
// buffer is processed the next one is in flight, as long as there is a next one: a buffer behind `end` is neither loaded nor processed.
// The loop is the one every sweep had - two full buffers per turn, straight line - and runs while a whole turn is full; the one or
// two buffers that remain, the last of them up to `end`, follow it.  Rows are processed in stream order.
template <int N, typename Buf, typename Load, typename Body>
__device__ __forceinline__ void sweep_rows(int beg, int end, Buf (&ra)[N], Buf (&rb)[N], Load &&load, Body &&body) {
    int g0 = beg;
    for (; g0 + 2 * N * WAVE < end; g0 += 2 * N * WAVE) {
        load(rb, g0 + N * WAVE);
        body(RowsAll(), ra, g0);
        load(ra, g0 + 2 * N * WAVE);
        body(RowsAll(), rb, g0 + N * WAVE);
    }
    if (g0 + N * WAVE < end) {
        load(rb, g0 + N * WAVE);
        body(RowsAll(), ra, g0);
        body(RowsUpto{rows_upto(g0 + N * WAVE, end)}, rb, g0 + N * WAVE);
    } else {
        body(RowsUpto{rows_upto(g0, end)}, ra, g0);
    }
}

#ifndef SETUP_THREADS
#define SETUP_THREADS 1024
#endif
#ifndef SETUP_REG_ROUNDS
#define SETUP_REG_ROUNDS 6    // rounds of SETUP_THREADS faces whose tile box and nearest depth k_raster_setup keeps in registers between its two
#endif                        // passes (two registers a round; STICK takes six rounds); a mesh with more rounds goes through the tables in memory
#ifndef LIST_CAP_PER_FACE
#define LIST_CAP_PER_FACE 8   // (tile, face) list entries an image may have per face at S <= 256 (a face's blurred box covers ~4 tiles there,
                              // ~8 at 512^2: the blur radius is a fixed fraction of the image); doubled above 256
#endif
struct SetupArgs {
    ClipTables clip;
    const float *verts_ndc; const int *faces;
    uint32_t *tbox, *gbox; uint4 *items; uint32_t item_cap; float2 *fzr;
    RasterCounters *ctr;
    int V, F, S, tiles_x; float sqrt_blur, z_clip;
    float *d_ndc_zero; const float *loss_src; float *loss_dst; unsigned long long *loss_acc; float *img_bound; int max_valence;
    float *dndc_scale; const float *pix_scale; float inv_sigma; int packed;
    uint2 *lists;       // (N, list_cap) binned tile lists: {face id, bits of its nearest vertex depth} (8 bytes: the farthest depth only ever fed the
                        // tile's depth range, and farthest <= nearest + the image's largest face extent bounds that as well)
    uint32_t list_cap;  // entries per image (0: no binning)
    uint32_t *cd_counter;  // SmilClipDepth.counter of a gradient call with image0 == 0: reset here (block 0), or NULL
    int store_tables;   // tbox / fzr / gbox have a reader behind this kernel (tie_rule 1, the colour path, image sizes that are never binned):
                        // store them for every image.  0: only an image whose lists do not fit stores them (for build_list), and a mesh
                        // of more than SETUP_REG_ROUNDS rounds, whose pass 2 reads them back
    int copies;         // (round 5) per-tile counters / list cursors are kept in this many copies (1, 2 or 4: what fits 48 KB of LDS), a
                        // face using copy (face id % copies): consecutive faces hit the same tiles, and LDS atomics of one wave
                        // instruction on ONE address execute one after the other - the two atomic passes were two thirds of this kernel
};

// ---------------------------------------------------------------------------------------------
// per-(pixel, face) evaluation
// ---------------------------------------------------------------------------------------------
// Face record staged in LDS (32 floats = 8 x 16 B).  Everything that does not depend on the pixel is folded in once
// per (tile, face): coordinates are relative to the tile centre (cx, cy) so the affine forms below do not cancel
// catastrophically.
//   w_i(p) = A_i dx + B_i dy + C_i  = b_i(p) * z_j z_k   (perspective-correct barycentric numerators; the
//            common denominator is positive, so inside <=> all w_i > 0)
// The fields are ordered so that what the evaluation computes in pairs sits in adjacent registers after the 16-byte LDS reads:
// (w0, w1), the projections on the two edges leaving v0, ... become one packed fp32 instruction each (v_pk_fma_f32 / v_pk_mul_f32 /
// v_pk_add_f32) without register moves; the third of each kind stays scalar.
struct alignas(16) FaceRec {
    float A0, A1, B0, B1;
    float C0, C1, A2, B2;
    float C2, z0, z1, z2;
    float x0c, x1c, y0c, y1c;       // v0, v1 relative to the tile centre
    float e01x, e02x, e01y, e02y;   // edge vectors and 1/|e|^2 (0 for a degenerate edge)
    float rl01, rl02, e12x, e12y;
    float rl12;
    int i0, i1, i2;
};
static_assert(sizeof(FaceRec) == FREC * sizeof(float), "FaceRec layout");
// (Round 4: the record no longer carries the blurred bounding box.  A lane only ever sees pixels of its face's pixel box, a superset of
// the bounding box by 0.01 px, and a pixel outside the box is farther than sqrt(blur) from the face, so the distance test rejects it
// as the box test did; the two can differ only for a pixel centre within rounding of the box edge.)

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 splat2(float x) { return (f32x2){x, x}; }
__device__ __forceinline__ f32x2 clamp01(f32x2 v) {  // (folds into the clamp bit of the producing instruction)
    return __builtin_elementwise_min(__builtin_elementwise_max(v, splat2(0.f)), splat2(1.f));
}
__device__ __forceinline__ float vmax_raw(float a, float b) {
    // (v_max_f32 spelled out: hipcc puts a canonicalising v_max x, x in front of every fmaxf whose input it cannot prove canonical,
    // and these inputs - results of fma instructions - always are)
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Two horizontally adjacent pixels of one face per lane (round 4).  Everything a lane does per (face, pixel) pair that is not
// arithmetic - finding its face and pixel, gathering the face record from LDS, the loop around it - is paid once per TWO pairs, and
// the arithmetic itself packs over the two pixels (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32, the face's constants as op_sel
// splats): the two pixels share dy, and with it the y parts of every projection.
// The face record as seven 16-byte rows read straight into registers.  (Reading it through a FaceRec in private memory let the
// optimiser turn `w0 > 0 ? z0 : z1` into an INDEXED load from that private copy - which then lives in scratch memory, with a
// scratch store and six scratch loads per sweep step.)
struct FaceRows { float4 r0, r1, r2, r3, r4, r5, r6; };
struct PairEval2 {
    f32x2 w0, w1, w2;     // perspective-correct barycentric numerators, .x = left pixel (even column), .y = right pixel
    f32x2 sd;             // signed squared distance
    bool cand0, cand1, inside0, inside1;
    uint32_t ebits0, ebits1;  // closest edge << 23 (record layout)
};
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
// clamp(v * s, 0, 1) for both pixels in one instruction, s = the low / high half of the pair `s2` (hipcc leaves the clamp of a packed
// product as two separate v_max)
__device__ __forceinline__ f32x2 pk_mul_clamp_lo(f32x2 v, f32x2 s2) {
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0] clamp" : "=v"(r) : "v"(v), "v"(s2));
    return r;
}
__device__ __forceinline__ f32x2 pk_mul_clamp_hi(f32x2 v, f32x2 s2) {
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] clamp" : "=v"(r) : "v"(v), "v"(s2));
    return r;
}
__device__ __forceinline__ void eval_pair2(const FaceRows &q, float dx0, float dx1, float dyp, float blur, PairEval2 &e) {
    const f32x2 DX = {dx0, dx1};
    const f32x2 base01 = pk_fma((f32x2){q.r0.z, q.r0.w}, splat2(dyp), (f32x2){q.r1.x, q.r1.y});
    const float base2 = fmaf(q.r1.w, dyp, q.r2.x);
    e.w0 = pk_fma(splat2(q.r0.x), DX, splat2(base01.x));
    e.w1 = pk_fma(splat2(q.r0.y), DX, splat2(base01.y));
    e.w2 = pk_fma(splat2(q.r1.z), DX, splat2(base2));
    e.inside0 = fminf(fminf(e.w0.x, e.w1.x), e.w2.x) > 0.f;   // (all three positive; the numerators are finite)
    e.inside1 = fminf(fminf(e.w0.y, e.w1.y), e.w2.y) > 0.f;
    // pixels relative to v0 and to v1; the y parts are the same for both pixels
    const f32x2 QX0 = DX - splat2(q.r3.x), QX1 = DX - splat2(q.r3.y);
    const f32x2 qy = splat2(dyp) - (f32x2){q.r3.z, q.r3.w};           // .x relative to v0, .y relative to v1
    const f32x2 eyq0 = (f32x2){q.r4.z, q.r4.w} * splat2(qy.x);        // y parts of the projections on the edges leaving v0
    const float eyq12 = q.r5.w * qy.y;
    const f32x2 rl0102 = {q.r5.x, q.r5.y}, rl12_ = {q.r6.x, q.r6.y};
    const f32x2 T01 = pk_mul_clamp_lo(pk_fma(splat2(q.r4.x), QX0, splat2(eyq0.x)), rl0102);
    const f32x2 T02 = pk_mul_clamp_hi(pk_fma(splat2(q.r4.y), QX0, splat2(eyq0.y)), rl0102);
    const f32x2 T12 = pk_mul_clamp_lo(pk_fma(splat2(q.r5.z), QX1, splat2(eyq12)), rl12_);
    const f32x2 RX01 = pk_fma(T01, splat2(q.r4.x), -QX0), RY01 = pk_fma(T01, splat2(q.r4.z), -splat2(qy.x));
    const f32x2 RX02 = pk_fma(T02, splat2(q.r4.y), -QX0), RY02 = pk_fma(T02, splat2(q.r4.w), -splat2(qy.x));
    const f32x2 RX12 = pk_fma(T12, splat2(q.r5.z), -QX1), RY12 = pk_fma(T12, splat2(q.r5.w), -splat2(qy.y));
    const f32x2 D01 = pk_fma(RX01, RX01, RY01 * RY01), D02 = pk_fma(RX02, RX02, RY02 * RY02), D12 = pk_fma(RX12, RX12, RY12 * RY12);
    const float dist0 = fminf(fminf(D01.x, D02.x), D12.x), dist1 = fminf(fminf(D01.y, D02.y), D12.y);
    e.cand0 = e.inside0 || dist0 < blur;
    e.cand1 = e.inside1 || dist1 < blur;
    e.sd = (f32x2){e.inside0 ? -dist0 : dist0, e.inside1 ? -dist1 : dist1};
    // closest edge in the reference's order e01, e02, e12 with <= ties: the first whose distance IS the minimum
    e.ebits0 = D01.x == dist0 ? 0u : (D02.x == dist0 ? 1u << 23 : 2u << 23);
    e.ebits1 = D01.y == dist1 ? 0u : (D02.y == dist1 ? 1u << 23 : 2u << 23);
}
// depth at the clipped, renormalised perspective-correct barycentrics, both pixels:
// c_i = max(p_i,0) / max(sum, 1e-5), p_i = w_i / den; 1/den cancels: c_i = max(w_i,0) / max(sum max(w,0), 1e-5 den).
// When a single weight survives the clip the depth is EXACTLY that vertex's depth, so faces sharing the vertex tie
// exactly (as x / x == 1 does in the reference) and the (depth, face id) order stays well defined.
__device__ __forceinline__ f32x2 pair_depth2(const FaceRows &q, const PairEval2 &e) {
    // (the vertex depths as opaque scalars: selecting among the ELEMENTS of a row makes the optimiser index the row dynamically,
    // through scratch memory)
    float z0 = q.r2.y, z1 = q.r2.z, z2 = q.r2.w;
    asm("" : "+v"(z0), "+v"(z1), "+v"(z2));
    const f32x2 den3 = e.w0 + e.w1 + e.w2;
    const f32x2 den = {fmaxf(den3.x, K_EPS), fmaxf(den3.y, K_EPS)};
    const f32x2 m0 = {vmax_raw(e.w0.x, 0.f), vmax_raw(e.w0.y, 0.f)}, m1 = {vmax_raw(e.w1.x, 0.f), vmax_raw(e.w1.y, 0.f)},
                m2 = {vmax_raw(e.w2.x, 0.f), vmax_raw(e.w2.y, 0.f)};
    const f32x2 msum = m0 + m1 + m2, floor_ = splat2(1e-5f) * den;
    const f32x2 cs = {fmaxf(msum.x, floor_.x), fmaxf(msum.y, floor_.y)};
    const f32x2 rc = {__builtin_amdgcn_rcpf(cs.x), __builtin_amdgcn_rcpf(cs.y)};
    // (every fused multiply-add spelled out: left to the compiler, the last one is contracted in one inlining context and not in
    // another - k_raster_tie_replay must reproduce these depths bit for bit, or an exact tie here is no tie there)
    const f32x2 pz = pk_fma(splat2(z2), m2 * rc, pk_fma(splat2(z0), m0 * rc, splat2(z1) * (m1 * rc)));
    // one survivor <=> the sum of the clipped weights equals their maximum (and was not lifted by the 1e-5 floor)
    const float mx0 = fmaxf(fmaxf(m0.x, m1.x), m2.x), mx1 = fmaxf(fmaxf(m0.y, m1.y), m2.y);
    const bool single0 = (msum.x == mx0) && (mx0 >= cs.x), single1 = (msum.y == mx1) && (mx1 >= cs.y);
    const float zv0 = m0.x > 0.f ? z0 : (m1.x > 0.f ? z1 : z2), zv1 = m0.y > 0.f ? z0 : (m1.y > 0.f ? z1 : z2);
    return (f32x2){single0 ? zv0 : pz.x, single1 ? zv1 : pz.y};
}

// float -> nearest integer in ONE instruction (v_cvt_rpi_i32_f32 = floor(x + 0.5); __float2int_rn is v_rndne + v_cvt; the two differ
// only on exact halves, which round up here)
__device__ __forceinline__ int cvt_round(float x) {
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// (x, y) -> x * 2^32 + y as 64-bit two's complement (a negative y borrows one from the high word): the packed fixed-point form of a
// gradient contribution in the LDS accumulators of pass 3 and in the rows of a packed launch (image_fx_scale)
__device__ __forceinline__ unsigned long long pack_fx2(float x, float y) {
    const int qx = cvt_round(x), qy = cvt_round(y);
    return ((unsigned long long)(uint32_t)(qx + (qy >> 31)) << 32) | (unsigned long long)(uint32_t)qy;
}

// What a record hands to the end points a, b of its closest edge in pass 3: the closest point of the edge is the clamped projection of
// the pixel c, as eval_pair computed it (t = 0 for a degenerate edge); r = closest point - pixel; the end points share 2 r gd as
// (1 - t) : t.  Every rounding is spelled out and contraction is off: the row body of pass 3 exists in two instances (sweep_rows) and
// left to itself the compiler fuses their multiplies and adds differently - a unit in the last place of a fixed-point contribution.
// The fused operations are the ones the single instance compiled to.
struct EdgeGrad { float ax, ay, bx, by; };
__device__ __forceinline__ EdgeGrad edge_gradient(float2 pa, float2 pb, float2 pc, float gd) {
#pragma clang fp contract(off)
    const float exx = pb.x - pa.x, eyy = pb.y - pa.y;
    const float l2 = exx * exx + eyy * eyy;
    const float dot = fmaf(exx, pc.x - pa.x, eyy * (pc.y - pa.y));
    const float t = __builtin_amdgcn_fmed3f(dot * (l2 <= K_EPS ? 0.f : __builtin_amdgcn_rcpf(l2)), 0.f, 1.f);
    const float rx2 = 2.0f * fmaf(t, exx, pa.x - pc.x), ry2 = 2.0f * fmaf(t, eyy, pa.y - pc.y);
    const float bx = t * (rx2 * gd), by = t * (ry2 * gd);
    return EdgeGrad{fmaf(rx2, gd, -bx), fmaf(ry2, gd, -by), bx, by};
}

__device__ __forceinline__ float face_prob(float sd, float inv_sigma_log2e) {
    // sigmoid(-dist / sigma) = 1 / (1 + 2^{dist log2(e) / sigma}); v_exp_f32 + v_rcp_f32 (1 ulp each), the two constant factors
    // of the exponent folded into one on the host
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(sd * inv_sigma_log2e));
}

__device__ __forceinline__ bool box_has(uint32_t b, int tx, int ty) {
    const int tx0 = b & 0xFF, ty0 = (b >> 8) & 0xFF, tx1 = (b >> 16) & 0xFF, ty1 = b >> 24;
    return (tx >= tx0) && (tx <= tx1) && (ty >= ty0) && (ty <= ty1);
}

struct Tri9 { float x0, y0, z0, x1, y1, z1, x2, y2, z2; };
// the nine vertex floats of a lane's face (both lanes of a face load the same: one transaction), through the clip tables
__device__ __forceinline__ Tri9 load_tri(const RasterArgs &a, const float *__restrict__ vn, const float *__restrict__ xv_n, int i0, int i1, int i2) {
    const float *p0 = vertex_ptr(vn, xv_n, a.V, i0), *p1 = vertex_ptr(vn, xv_n, a.V, i1), *p2 = vertex_ptr(vn, xv_n, a.V, i2);
    return Tri9{p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2]};
}
// The seven rows of a face record from its vertices, in two halves (stage_faces: one lane each).  Every rounding is spelled out -
// no contraction left to the compiler (which fuses a*b - c*d one way in one inlining context and another way in the next): the
// tile kernel and k_raster_tie_replay must get the SAME bits from the same face, or an exact depth tie in one is no tie in the other.
__device__ __forceinline__ float edge_fx(float px, float py, float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
    return fmaf(px - ax, by - ay, -((py - ay) * (bx - ax)));
}
__device__ __forceinline__ void face_rows_lo(const Tri9 &tv, float cx, float cy, float4 &r0, float4 &r1, float4 &r2) {
#pragma clang fp contract(off)
    const float x0 = tv.x0, y0 = tv.y0, z0 = tv.z0, x1 = tv.x1, y1 = tv.y1, z1 = tv.z1, x2 = tv.x2, y2 = tv.y2, z2 = tv.z2;
    // (only the signs of the w_i and their ratios are used: the scale's last bits do not matter)
    const float rcp_area = __builtin_amdgcn_rcpf(edge_fx(x2, y2, x0, y0, x1, y1) + K_EPS);
    // edge function e_k(p) = (px - ax)(by - ay) - (py - ay)(bx - ax), linear in p; value at the tile centre + slopes
    const float s0 = rcp_area * (z1 * z2), s1 = rcp_area * (z0 * z2), s2 = rcp_area * (z0 * z1);
    r0 = make_float4((y2 - y1) * s0, (y0 - y2) * s1, -(x2 - x1) * s0, -(x0 - x2) * s1);                                      // A0 A1 B0 B1
    r1 = make_float4(edge_fx(cx, cy, x1, y1, x2, y2) * s0, edge_fx(cx, cy, x2, y2, x0, y0) * s1, (y1 - y0) * s2, -(x1 - x0) * s2);  // C0 C1 A2 B2
    r2 = make_float4(edge_fx(cx, cy, x0, y0, x1, y1) * s2, z0, z1, z2);
}
__device__ __forceinline__ void face_rows_hi(const Tri9 &tv, float cx, float cy, float4 &r3, float4 &r4, float4 &r5, float &rl12_out) {
#pragma clang fp contract(off)
    const float x0 = tv.x0, y0 = tv.y0, x1 = tv.x1, y1 = tv.y1, x2 = tv.x2, y2 = tv.y2;
    const float e01x = x1 - x0, e01y = y1 - y0, e02x = x2 - x0, e02y = y2 - y0, e12x = x2 - x1, e12y = y2 - y1;
    const float l01 = fmaf(e01x, e01x, e01y * e01y), l02 = fmaf(e02x, e02x, e02y * e02y), l12 = fmaf(e12x, e12x, e12y * e12y);
    const float rl01 = l01 <= K_EPS ? 0.f : __builtin_amdgcn_rcpf(l01);
    const float rl02 = l02 <= K_EPS ? 0.f : __builtin_amdgcn_rcpf(l02);
    rl12_out = l12 <= K_EPS ? 0.f : __builtin_amdgcn_rcpf(l12);
    r3 = make_float4(x0 - cx, x1 - cx, y0 - cy, y1 - cy);
    r4 = make_float4(e01x, e02x, e01y, e02y);
    r5 = make_float4(rl01, rl02, e12x, e12y);
}

__device__ __forceinline__ FaceRows face_rows_from_tri(const Tri9 &tv, float cx, float cy) {
    FaceRows q;
    float rl12;
    face_rows_lo(tv, cx, cy, q.r0, q.r1, q.r2);
    face_rows_hi(tv, cx, cy, q.r3, q.r4, q.r5, rl12);
    q.r6 = make_float4(rl12, 0.f, 0.f, 0.f);
    return q;
}
// largest value of the wave (values > 0, or 0 for "none") in DPP: a running maximum along the lanes as wave_scan_add runs its sum
// (lanes that receive nothing read 0), read from the last lane - no LDS round trips in the replay's serial chain
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    int x = (int)v;
#define MAX_STEP(ctrl, rows) { x = (int)max((uint32_t)x, (uint32_t)__builtin_amdgcn_update_dpp(0, x, ctrl, rows, 0xF, false)); }
    MAX_STEP(0x111, 0xF) MAX_STEP(0x112, 0xF) MAX_STEP(0x114, 0xF) MAX_STEP(0x118, 0xF)
    MAX_STEP(0x142, 0xA) MAX_STEP(0x143, 0xC)
#undef MAX_STEP
    return (uint32_t)__builtin_amdgcn_readlane(x, WAVE - 1);
}
