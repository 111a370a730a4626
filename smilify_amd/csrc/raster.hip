// Soft-silhouette rasteriser for gfx950: forward, backward and fused forward+L1+backward.
//
// Replaces (reference): smal_fitter/p3d_renderer.py:41-52,142-146 - MeshRasterizer(bin_size=0,
// faces_per_pixel=100, blur_radius=log(1/1e-4-1)*1e-4, perspective-correct, clipped barycentrics) +
// SoftSilhouetteShader (sigmoid_alpha_blend) - and, in the fused entry point, the silhouette L1 term of
// SMALFitter.forward (fitter.py:332-333) with its gradient.  The per-(pixel,face) arithmetic restates
// pytorch3d 0.7.x (un-vendored): CheckPixelInsideFace / RasterizeMeshesBackward / geometry_utils.
//
// Design (see DESIGN.md "raster"):
//  * The reference visits all F faces for all S^2 pixels and stores (S,S,K) fragments in HBM (157 MB / image at 256^2).
//  * k_raster_setup (one workgroup per image): per-face validity + blurred bbox in 8x8-pixel tile units (4 x u8 packed),
//    the union of those boxes per 64 consecutive faces, per-face vertex-depth range, a tile-occupancy bitmap in LDS, and
//    the compacted list of touched tiles appended to a global work list.  Untouched tiles are never visited (their
//    silhouette is 0).
//  * k_raster_dense (persistent single-wave workgroups, work item = one 8x8 tile).  Every (face, pixel) pair is
//    evaluated ONCE, by a lane that exists only for pairs inside the face's pixel box; every later step is a dense sweep
//    (lane = record) over the records that pass produced.  An earlier design (lane = pixel, each face broadcast to the 64
//    pixels of the tile, three re-evaluating passes, K smallest depths in a sorted register array) spent ~75 % of its
//    lanes on pairs that do not exist and 100 v_med3 per face on the selection; it is gone.
//      list    faces whose tile box contains the tile (via the 64-face group boxes), with their nearest vertex depth; tiles
//              that may truncate (list > K) order it NEAR TO FAR by the first radix digit of that depth (counting sort).
//              A binned list of up to LIST_LDS_ROWS * 64 entries is read from memory once and sorted out of LDS.
//      pass 1  lane = pair.  Per DCHUNK-face chunk: two lanes per face stage its record and its pixel box inside the tile
//              (shrunk to the pixels that are still open), a prefix sum lays the boxes end to end, and the wave sweeps that
//              pair list 64 at a time (a start-bit map gives each pair its face with two v_mbcnt and two ds_bpermute; face
//              record and pixel coordinates are gathered from LDS).  Accepted pairs are ballot-compacted into the
//              workgroup's record stream in global memory (reused for every tile): 12 bytes {depth, pixel | list position
//              | inside | edge, signed squared distance}, one array of structures.  The first radix digit of every depth
//              (64 buckets, saturating 8-bit counts) is histogrammed per pixel on the way.  CLOSING: a record's depth is
//              at least its face's nearest vertex depth, so once the walk reaches digit d the per-pixel counts of digits
//              < d are final; a pixel holding >= K records there takes no further record, and when no pixel is open the
//              rest of the list is skipped.
//      blend   one sweep over the records.  A record of a pixel with <= K candidates, or whose first digit lies below the
//              digit that holds the pixel's K-th depth, is kept for certain: log2 of its factor is added to the pixel's
//              sum (fp64 LDS atomics).  A record inside that digit goes on to a compact stream {key, meta, log} and has
//              its second digit counted; one above it is dropped.
//      select  (only where a pixel has more than K candidates) the remaining digits by radix select over the compact
//              stream, SEL_BITS per sweep, per-pixel histograms in LDS; the stream shrinks in place with every sweep.
//              Exact, including the number of faces tied at the threshold; when a tie group straddles K, further sweeps
//              select on the face id (fetched through the list only for records at the threshold).  A last sweep adds the
//              logs of the records that made it; alpha = exp2(sum) (the fp32 product and the fp64-accumulated log-sum are
//              both ~1e-6 relative from the exact product).
//      pass 3  gradient of every kept record into per-face LDS accumulators ((x, y) packed as two 32-bit fixed-point numbers
//              in one 64-bit word), per 64 faces; the closest point on the record's edge is recomputed from a table of the
//              group's vertices.  Flush: one global atomic per touched vertex - two floats, or, from 64 images per launch
//              on, one packed 64-bit integer decoded afterwards (k_unpack_dndc); these atomics execute memory-side.
//  * A tile whose records would not fit the stream (REC_CAP) is processed in sub-tiles: power-of-two runs of its 64 pixels,
//    halved until pass 1 fits.  A single pixel always fits because F <= REC_CAP is required on the host.
//  * Deviation from the reference kept on purpose: the K faces a truncated pixel keeps are the K smallest by (depth, face
//    id).  The reference's unsorted-queue eviction picks among equal depths by visiting history (measured effect on the
//    L1 loss: ~1e-5 relative at K = 100; tests/test_gpu_kernels.py checks this rule exactly against the oracle's
//    select_mode(1) and the faithful queue within the documented tolerance).
//
// Map (one translation unit; the headers are included below in this order and by nothing else):
//   raster_common.h  constants, RasterArgs / SetupArgs, clip tables, `at`, wave helpers, the pair arithmetic, pack_fx2; it includes
//   raster_reach.h   the rounded blur box (corner-tile flags, row / column trim): plain C++, also compiled on the host by a test
//   raster_setup.h   k_raster_setup, k_clip_backward, k_unpack_dndc
//   raster_tile.h    DenseLds, the list phase, stage_faces, the select sweeps, k_raster_dense
//   raster_replay.h  k_raster_tie_replay
//   here             the host side: workspace layout, launchers, profiler, the extern "C" entries, the colour path's setup
#include "common.h"

// Instrumentation hooks (phase timers, work counters, cut-off / wrap experiments): empty in libsmilfit.so.  `make variant` builds the
// instrumented libraries of tools/dbg with -DSMIL_INSTRUMENTED, which pulls their definitions from tools/dbg/raster_hooks_dbg.h; this
// translation unit itself holds no experiment code, and smil_version() says which kind of build a library is.
#include "raster_hooks.h"
#include "raster_common.h"
#include "raster_setup.h"
#include "raster_tile.h"
#include "raster_replay.h"

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// Compute units of the current device (256 on MI355X): the persistent grids are sized to fill them.
static int device_cus() { return smil_device_limits().cus; }

// resident workgroup slots of the device: what the tile kernel's dealing policy (pieces per tile) is tuned against
static long long tile_slots() {
    long long resident = (long long)device_cus() * RESIDENT_PER_CU;
    HOOK_RESIDENT(resident)
    return resident;
}
static int tile_grid(int N, int tiles_x) {
    // The grid - and with it the scratch arena, 1.6 MB per workgroup - is the largest number of workgroups the policy can put to
    // work on at most N x tiles touched tiles (the policy is piecewise monotone in the number of touched tiles: its maximum lies at
    // the upper end of one of its four ranges), so a small launch neither starts nor pays scratch for workgroups that would leave
    // at once: one 256^2 image gets 1 792 workgroups, one 128^2 image 896, not 4 096.
    const long long resident = tile_slots();
    const unsigned long long n_max = (unsigned long long)N * tiles_x * tiles_x;
    const unsigned int slots = (unsigned int)resident;
    unsigned int best = slots / 8u;
    const unsigned long long ends[4] = {slots * 5ull / 64ull, slots * 5ull / 16ull, slots * 5ull / 8ull, n_max};
    for (int k = 0; k < 4; ++k) {
        const unsigned long long n = ends[k] < n_max ? ends[k] : n_max;
        if (n == 0ull || n > 0x7FFFFFFull) { if (n) best = slots; continue; }
        const unsigned int w = deal_working((unsigned int)n, deal_split_log((unsigned int)n, slots), slots);
        best = w > best ? w : best;
    }
    return (int)(best < slots ? best : slots);
}

// binned tile lists: LIST_CAP_PER_FACE entries per face and image (8 bytes each) + one depth range per tile; images with more than
// COUNT_TILES_MAX tiles are never binned
static inline uint32_t list_cap_of(const SmilModel *m, int S) {
    return ceil_div(S, TILE) * ceil_div(S, TILE) <= COUNT_TILES_MAX ? (uint32_t)LIST_CAP_PER_FACE * (S > 256 ? 2u : 1u) * (uint32_t)m->F : 0u;
}

static inline int face_rows(const SmilModel *m) { return faces_padded(m->F) + CLIP_FX; }
// THE layout of a rasteriser workspace (smil_raster_workspace_bytes sizes it, raster_common carves it; tools/raster_probe.py reads the
// counters and tile boxes).  The counters come first, so that smil_raster_stats finds them without knowing N.  Fills the regions' pointers
// and capacities in q (setup kernel) and a (tile kernel).
static size_t raster_layout(const SmilModel *m, int N, int S, char *base, SetupArgs &q, RasterArgs &a) {
    const int tiles_x = ceil_div(S, TILE), FT = face_rows(m);
    Workspace w{base};
    a.ctr = q.ctr = w.take<RasterCounters>(1);
    a.tbox = q.tbox = w.take<uint32_t>((size_t)N * FT);
    a.item_cap = q.item_cap = (uint32_t)ceil_div(N, N_PARTS) * (uint32_t)(tiles_x * tiles_x);
    a.items = q.items = w.take<uint4>((size_t)2 * N_PARTS * q.item_cap);  // work lists (2, N, tiles)
    a.tie_mask = w.take<unsigned long long>((size_t)2 * N_PARTS * q.item_cap);  // (tie_rule 1)
    a.fzr = q.fzr = w.take<float2>((size_t)N * FT);
    a.gbox = q.gbox = w.take<uint32_t>((size_t)N * (FT / WAVE));
    a.img_bound = q.img_bound = w.take<float>(N);
    a.loss_acc = q.loss_acc = w.take<unsigned long long>(N);
    a.list_cap = q.list_cap = list_cap_of(m, S);
    a.lists = q.lists = w.take<uint2>((size_t)N * q.list_cap);
    // per-image clip tables: new vertices, their gradient rows, end points and coefficients, front-part faces, count
    ClipTables &c = q.clip;
    c.xv = w.take<float>((size_t)N * CLIP_VX * 3);
    c.xg = w.take<float>((size_t)N * CLIP_VX * 2);
    c.xsrc = w.take<int2>((size_t)N * CLIP_VX);
    c.xcoef = w.take<float2>((size_t)N * CLIP_VX);
    c.xf = w.take<int>((size_t)N * CLIP_FX * 3);
    c.xcount = w.take<uint32_t>(N);
    c.xparent = nullptr;
    a.clip = c;
    w.take<char>(256);  // (slack ahead of the scratch that the sizes have always carried)
    // per resident workgroup: F x {face id, nearest depth} in id order (tiles of images that are not binned), F face ids in walking
    // order, F / DCHUNK + 2 chunk starts, F x {projected vertices, vertex ids} by list position, the two record streams
    const size_t grid = (size_t)tile_grid(N, tiles_x);
    a.list_stride = (int)(align256((size_t)FT * sizeof(uint32_t)) / sizeof(uint32_t));
    a.n_cf = (int)(align256((size_t)(FT / DCHUNK + 2) * sizeof(uint32_t)) / sizeof(uint32_t));
    a.slist = w.take<uint2>(grid * a.list_stride);
    a.slist2 = w.take<uint32_t>(grid * a.list_stride);
    a.scfirst = w.take<uint32_t>(grid * a.n_cf);
    a.sxy = w.take<float2>(grid * a.list_stride * 3);
    a.sid = w.take<TriIds>(grid * a.list_stride);
    a.srec = w.take<Rec3>(grid * (REC_CAP + REC_PAD));
    a.crec = w.take<Rec3>(grid * (REC_CAP + REC_PAD));
    return w.used;
}

extern "C" size_t smil_raster_workspace_bytes(const SmilModel *m, int32_t N, int32_t S) {
    SetupArgs q;
    RasterArgs a;
    return (m && N > 0 && S > 0) ? raster_layout(m, N, S, nullptr, q, a) : 0;
}

// Counters of the most recent rasteriser call that used `workspace` (device -> host copy: synchronises the stream).
extern "C" int smil_raster_stats(const SmilModel *m, const void *workspace, void *stream_, uint32_t *out4) {
    SMIL_REQUIRE(m && workspace && out4, "smil_raster_stats: bad argument");
    RasterCounters h;
    SMIL_HIP(hipMemcpyAsync(&h, workspace, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    SMIL_HIP(hipStreamSynchronize((hipStream_t)stream_));
    unsigned int tiles = 0;
    for (int q = 0; q < N_PARTS; ++q)
        for (int c = 0; c < N_CLASSES; ++c) tiles += h.n_class[q][c];
    out4[0] = h.straddling; out4[1] = tiles; out4[2] = h.unclipped; out4[3] = h.tie_pixels;
    return SMIL_OK;
}

// the size and index-range checks of every call that runs the setup kernel
static int check_sizes(const SmilModel *m, int N, int S, const char *who) {
    SMIL_REQUIRE(N > 0 && S > 0 && S <= TILE * 256, "%s: bad sizes N=%d S=%d", who, N, S);
    const int tiles_x = ceil_div(S, TILE);
    SMIL_REQUIRE((double)N * tiles_x * tiles_x < 2147483647.0, "%s: N * tiles exceeds the work-item index range (2^31); launch in slices", who);
    SMIL_REQUIRE(face_rows(m) + 64 < (1 << 24) && (double)list_cap_of(m, S) * sizeof(uint2) < 4294967296.0,
                 "%s: per-workgroup / per-image tables exceed the 24-bit index / 32-bit byte-offset range of at()", who);
    return SMIL_OK;
}

// zero the counters and run k_raster_setup, one workgroup per image
static int launch_setup(SetupArgs &q, int N, hipStream_t stream) {
    SMIL_HIP(hipMemsetAsync(q.ctr, 0, sizeof(RasterCounters), stream));
    const int n_tiles = q.tiles_x * q.tiles_x;
    // per tile and copy: 8 bytes of counts + 4 bytes of list cursor (as many copies as fit 48 KB: two workgroups per CU), or one bit
    q.copies = n_tiles * 2 * 12 <= 48 * 1024 ? 2 : 1;  // (measured: two copies -10 % STICK / -17 % mouse at 256^2, four copies -5 % / -6 %)
#ifdef SETUP_COPIES
    q.copies = SETUP_COPIES;
#endif
    const size_t setup_lds = n_tiles <= COUNT_TILES_MAX ? (size_t)n_tiles * q.copies * 12 : (size_t)((n_tiles + 31) / 32) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_raster_setup, dim3(N), dim3(SETUP_THREADS), setup_lds, stream, q);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// Carves the workspace and runs the setup kernel.  q: the caller has set the fields it owns (the gradient calls' d_ndc_zero, loss
// sums, packing and decode scale), everything else is set here; a: the per-mode outputs are the caller's to set afterwards.
static int raster_common(const SmilModel *m, const float *verts_ndc, int N, int S, const SmilRasterSettings *rs, void *workspace,
                         hipStream_t stream, bool grads, SetupArgs &q, RasterArgs &a) {
    SMIL_REQUIRE(m && verts_ndc && rs && workspace, "raster: null argument");
    if (int rc = check_sizes(m, N, S, "raster")) return rc;
    SMIL_REQUIRE(rs->faces_per_pixel > 0 && rs->faces_per_pixel <= SMIL_MAX_FACES_PER_PIXEL,
                 "raster: faces_per_pixel=%d outside 1..%d", rs->faces_per_pixel, SMIL_MAX_FACES_PER_PIXEL);
    SMIL_REQUIRE(rs->sigma > 0.f && rs->blur_radius >= 0.f, "raster: bad blend settings");
    SMIL_REQUIRE(rs->tie_rule == SMIL_TIE_DEPTH_FACE_ID || rs->tie_rule == SMIL_TIE_REFERENCE_QUEUE, "raster: tie_rule=%d is neither 0 nor 1", rs->tie_rule);
    SMIL_REQUIRE(face_rows(m) <= REC_CAP, "raster: %d faces exceed the %d a single pixel's records may hold", m->F, REC_CAP - CLIP_FX - WAVE);
    static_assert(REC_CAP + REC_PAD < (1 << 24), "at<12-byte>() multiplies 24-bit indices");
    if (grads && rs->clip_depth)
        SMIL_REQUIRE(rs->clip_depth->vertex && rs->clip_depth->dz && rs->clip_depth->range && rs->clip_depth->counter && rs->clip_depth->capacity >= 0 &&
                     rs->image0 >= 0, "raster: incomplete SmilClipDepth");
    raster_layout(m, N, S, (char *)workspace, q, a);
    // the per-image tables tbox / fzr / gbox are read behind the setup kernel by k_raster_tie_replay and by tiles of images that are
    // never binned; otherwise only an image whose lists do not fit needs them, and the kernel finds that out itself
    q.store_tables = (rs->tie_rule != SMIL_TIE_DEPTH_FACE_ID || q.list_cap == 0u) ? 1 : 0;
    const int tiles_x = ceil_div(S, TILE);
    if (rs->tie_rule) SMIL_HIP(hipMemsetAsync(a.tie_mask, 0, (size_t)2 * N_PARTS * a.item_cap * sizeof(unsigned long long), stream));
    q.verts_ndc = a.verts_ndc = verts_ndc; q.faces = a.faces = m->faces;
    q.V = a.V = m->V; q.F = a.F = m->F; q.S = a.S = S; q.tiles_x = a.tiles_x = tiles_x;
    q.sqrt_blur = a.sqrt_blur = sqrtf(rs->blur_radius); q.z_clip = rs->z_clip; q.max_valence = m->max_valence;
    q.inv_sigma = a.inv_sigma = 1.0f / rs->sigma;
    q.cd_counter = (grads && rs->clip_depth && rs->image0 == 0) ? rs->clip_depth->counter : nullptr;
    if (int rc = launch_setup(q, N, stream)) return rc;
    a.FT = face_rows(m); a.slots = (unsigned int)tile_slots();
    a.tie_rule = rs->tie_rule; a.image0 = rs->image0;
    a.cd = (grads && rs->clip_depth) ? *rs->clip_depth : SmilClipDepth{nullptr, nullptr, nullptr, nullptr, 0};
    a.N = N; a.K = rs->faces_per_pixel; a.packed = 0;
    a.blur = rs->blur_radius; a.inv_sigma_log2e = (float)(1.4426950408889634 / (double)rs->sigma);
    HOOK_HOST_LAUNCH_SETUP(a, stream)
    a.sil = nullptr; a.grad_sil = nullptr; a.target = nullptr; a.target_u8 = nullptr; a.pix_scale = nullptr; a.loss_img = nullptr;
    a.d_ndc = nullptr;
    return SMIL_OK;
}

// ---- the colour path's share of the setup (shade.hip): k_raster_setup with blur 0 (K = 1 needs no blur box), its per-image tables,
// binned lists, work items and clip tables - none of the tile kernel's per-workgroup scratch ----
static size_t colour_setup_layout(const SmilModel *m, int N, int S, char *base, ColourSetup *o, SetupArgs *q) {
    const int tiles_x = ceil_div(S, TILE), FT = face_rows(m);
    const uint32_t item_cap = (uint32_t)ceil_div(N, N_PARTS) * (uint32_t)(tiles_x * tiles_x);
    const uint32_t list_cap = list_cap_of(m, S);
    Workspace w{base};
    uint32_t *tbox = w.take<uint32_t>((size_t)N * FT);
    RasterCounters *c = w.take<RasterCounters>(1);
    uint4 *items = w.take<uint4>((size_t)2 * N_PARTS * item_cap);
    float2 *fzr = w.take<float2>((size_t)N * FT);
    uint32_t *gbox = w.take<uint32_t>((size_t)N * (FT / WAVE));
    uint2 *lists = w.take<uint2>((size_t)N * list_cap);
    ClipTables clip;
    clip.xv = w.take<float>((size_t)N * CLIP_VX * 3);
    clip.xsrc = w.take<int2>((size_t)N * CLIP_VX);
    clip.xcoef = w.take<float2>((size_t)N * CLIP_VX);
    clip.xf = w.take<int>((size_t)N * CLIP_FX * 3);
    clip.xparent = w.take<int>((size_t)N * CLIP_CUTS);
    clip.xg = nullptr; clip.xcount = nullptr;  // (no gradient rows)
    if (!base) return w.used;
    o->tbox = tbox; o->gbox = gbox; o->fzr = fzr; o->items = items;
    o->n_class = &c->n_class[0][0]; o->ticket = &c->deal[0].next; o->item_cap = item_cap;
    o->lists = lists; o->list_cap = list_cap;
    o->xv = clip.xv; o->xf = clip.xf; o->xsrc = clip.xsrc; o->xparent = clip.xparent;
    o->FT = FT; o->FP = faces_padded(m->F); o->clip_vx = CLIP_VX; o->clip_fx = CLIP_FX; o->n_parts = N_PARTS; o->n_classes = N_CLASSES;
    *q = SetupArgs{};
    q->clip = clip; q->faces = m->faces; q->tbox = tbox; q->gbox = gbox; q->items = items;
    q->item_cap = item_cap; q->fzr = fzr; q->ctr = c; q->V = m->V; q->F = m->F; q->S = S; q->tiles_x = tiles_x;
    q->sqrt_blur = 0.f; q->inv_sigma = 1.f; q->lists = lists; q->list_cap = list_cap;
    q->store_tables = 1;  // (k_colour_tiles reads the tile boxes and depth ranges)
    return w.used;
}

size_t smil_colour_setup_bytes(const SmilModel *m, int N, int S) {
    return (m && N > 0 && S > 0) ? colour_setup_layout(m, N, S, nullptr, nullptr, nullptr) : 0;
}

int smil_colour_setup(const SmilModel *m, const float *verts_ndc, int N, int S, float z_clip, void *workspace, hipStream_t stream,
                      ColourSetup *out) {
    if (int rc = check_sizes(m, N, S, "smil_render_colour")) return rc;
    SetupArgs q;
    colour_setup_layout(m, N, S, (char *)workspace, out, &q);
    q.verts_ndc = verts_ndc; q.z_clip = z_clip;
    return launch_setup(q, N, stream);
}

// ---- optional in-process timing of the tile kernel (bench.py): HIP events recorded on the launch stream ----
#define PROF_SLOTS 512
static bool g_prof_on = false;
static hipEvent_t g_prof_ev[PROF_SLOTS][2];
static int g_prof_n = 0;
static bool g_prof_init = false;

extern "C" int smil_profile_enable(int32_t on) {
    if (on && !g_prof_init) {
        for (int i = 0; i < PROF_SLOTS; ++i) {
            SMIL_HIP(hipEventCreate(&g_prof_ev[i][0]));
            SMIL_HIP(hipEventCreate(&g_prof_ev[i][1]));
        }
        g_prof_init = true;
    }
    g_prof_on = on != 0;
    g_prof_n = 0;
    return SMIL_OK;
}

// Sum / count of the tile-kernel durations recorded since smil_profile_enable(1).  Synchronises the events.
extern "C" int smil_profile_read(float *total_ms, int32_t *launches) {
    SMIL_REQUIRE(total_ms && launches, "smil_profile_read: null argument");
    float tot = 0.f;
    const int n = g_prof_n < PROF_SLOTS ? g_prof_n : PROF_SLOTS;
    for (int i = 0; i < n; ++i) {
        SMIL_HIP(hipEventSynchronize(g_prof_ev[i][1]));
        float ms = 0.f;
        SMIL_HIP(hipEventElapsedTime(&ms, g_prof_ev[i][0], g_prof_ev[i][1]));
        tot += ms;
    }
    *total_ms = tot;
    *launches = n;
    g_prof_n = 0;
    return SMIL_OK;
}

#define PROF_BEGIN(stream) \
    const int _slot = (g_prof_on && g_prof_n < PROF_SLOTS) ? g_prof_n++ : -1; \
    if (_slot >= 0) (void)hipEventRecord(g_prof_ev[_slot][0], stream)
#define PROF_END(stream) \
    if (_slot >= 0) (void)hipEventRecord(g_prof_ev[_slot][1], stream)

// (tie_rule 1) the pixels the tile kernel left out: the reference's queue replayed, one wave per pixel
template <int MODE>
static void launch_tie_replay(const RasterArgs &a, hipStream_t stream) {
    // dynamic LDS: the face-id bitmap (FT bits), the filling queue (128 slots x 3 words), the tile's ordered face ids (17 bits each)
    const size_t lds = (size_t)a.FT / 8 + 6 * WAVE * sizeof(uint32_t) + (size_t)TIE_ORD_CAP * sizeof(uint16_t) + TIE_ORD_CAP / 8;
    // (as many waves as the registers let a CU hold - the ~6 KB of LDS per wave allow more; they take tickets until none is left)
    if (a.tie_rule) hipLaunchKernelGGL((k_raster_tie_replay<MODE>), dim3((unsigned int)device_cus() * 4u * TIE_WAVES_PER_SIMD), dim3(64), lds, stream, a);
}
// the tile kernel (timed when profiling is on), then the tie replay
template <int MODE>
static int launch_raster(const RasterArgs &a, hipStream_t stream) {
    PROF_BEGIN(stream);
    hipLaunchKernelGGL((k_raster_dense<MODE>), dim3(tile_grid(a.N, a.tiles_x)), dim3(64), 0, stream, a);
    PROF_END(stream);
    launch_tie_replay<MODE>(a, stream);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_silhouette_forward(const SmilModel *m, const float *verts_ndc, int32_t N, int32_t S,
                                       const SmilRasterSettings *rs, float *sil, void *workspace, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SetupArgs q{};
    RasterArgs a;
    int rc = raster_common(m, verts_ndc, N, S, rs, workspace, stream, false, q, a);
    if (rc) return rc;
    SMIL_REQUIRE(sil, "smil_silhouette_forward: null output");
    SMIL_HIP(hipMemsetAsync(sil, 0, (size_t)N * S * S * sizeof(float), stream));
    a.sil = sil;
    return launch_raster<MODE_FWD>(a, stream);
}

extern "C" int smil_silhouette_backward(const SmilModel *m, const float *verts_ndc, int32_t N, int32_t S,
                                        const SmilRasterSettings *rs, const float *grad_sil, float *d_ndc,
                                        void *workspace, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SetupArgs q{};
    RasterArgs a;
    int rc = raster_common(m, verts_ndc, N, S, rs, workspace, stream, true, q, a);
    if (rc) return rc;
    SMIL_REQUIRE(grad_sil && d_ndc, "smil_silhouette_backward: null argument");
    SMIL_HIP(hipMemsetAsync(d_ndc, 0, (size_t)N * m->V * 2 * sizeof(float), stream));
    a.grad_sil = grad_sil; a.d_ndc = d_ndc;
    if ((rc = launch_raster<MODE_BWD>(a, stream))) return rc;
    hipLaunchKernelGGL(k_clip_backward, dim3(N), dim3(64), 0, stream, a.clip, d_ndc, m->V, (float *)nullptr, (const unsigned long long *)nullptr, verts_ndc, rs->z_clip, a.cd, a.image0);  // (new vertices of cut faces -> their edges' end points)
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

extern "C" int smil_silhouette_l1_fused(const SmilModel *m, const float *verts_ndc, int32_t N, int32_t S,
                                        const SmilRasterSettings *rs, const void *target, int32_t target_is_u8,
                                        const float *target_sum, const float *pix_scale, float *loss_img, float *d_ndc,
                                        float *sil_out, float *d_ndc_scale, void *workspace, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SMIL_REQUIRE(target && target_sum && pix_scale && loss_img && d_ndc, "smil_silhouette_l1_fused: null argument");
    SetupArgs q{};
    RasterArgs a;
    // large launches accumulate the vertex gradients as packed fixed point (half the memory-side atomics); small ones keep float
    // atomics.  The packed rows are decoded in place afterwards, unless the caller takes them as they are (d_ndc_scale).
    q.packed = (N >= PACKED_MIN_IMAGES && (reinterpret_cast<uintptr_t>(d_ndc) & 7u) == 0u) ? 1 : 0;  // (64-bit atomics need 8-byte alignment)
    q.d_ndc_zero = d_ndc; q.loss_src = target_sum; q.loss_dst = loss_img; q.dndc_scale = d_ndc_scale; q.pix_scale = pix_scale;
    int rc = raster_common(m, verts_ndc, N, S, rs, workspace, stream, true, q, a);
    if (rc) return rc;
    if (sil_out) SMIL_HIP(hipMemsetAsync(sil_out, 0, (size_t)N * S * S * sizeof(float), stream));
    if (target_is_u8) a.target_u8 = (const uint8_t *)target; else a.target = (const float *)target;
    a.pix_scale = pix_scale; a.loss_img = loss_img; a.d_ndc = d_ndc; a.sil = sil_out;
    a.packed = q.packed;
    if ((rc = launch_raster<MODE_FUSED>(a, stream))) return rc;
    hipLaunchKernelGGL(k_clip_backward, dim3(N), dim3(64), 0, stream, a.clip, d_ndc, m->V, loss_img, (const unsigned long long *)a.loss_acc, verts_ndc, rs->z_clip, a.cd, a.image0);  // (new vertices of cut faces -> their edges' end points; the images' loss sums)
    SMIL_LAUNCH_CHECK();
    if (a.packed && !d_ndc_scale) {
        hipLaunchKernelGGL(k_unpack_dndc, dim3(N, ceil_div(m->V, 256)), dim3(256), 0, stream, d_ndc, a.img_bound, pix_scale, a.inv_sigma, m->V, a.clip.xcount);
        SMIL_LAUNCH_CHECK();
    }
    return SMIL_OK;
}
