// The rasteriser's setup kernel and the two small kernels behind the tile kernel (raster.hip; see the map of the headers there).
#pragma once

// ---------------------------------------------------------------------------------------------
// setup: per-face tile boxes + touched-tile work list
// ---------------------------------------------------------------------------------------------
// One workgroup per image.  Pass 1: per face validity, blurred pixel box -> tile box, depth range; per covered tile ONE LDS
// atomic adds the face's cost and list entry (64-bit: entries << 32 | cost).  Then the touched tiles go to the work lists by cost
// class and - new in round 3 - the faces are BINNED: a prefix sum over the tiles' entry counts lays the image's tile lists
// end to end, and pass 2 walks the faces again and appends each to the lists of the tiles its box covers.  The tile kernel
// then starts from its list instead of scanning the tile boxes of every 64-face group that reaches its tile (build_list:
// 13 % of the tile kernel in round 2).  Images whose lists exceed list_cap keep the old way.
__global__ void __launch_bounds__(SETUP_THREADS, 8) k_raster_setup(SetupArgs q) {  // (two blocks per CU: <= 64 VGPRs)
    __shared__ uint32_t s_maxpx;  // largest blurred pixel box of a face
    __shared__ uint32_t s_straddle;
    __shared__ uint32_t s_zext;   // bits of the largest depth extent (farthest - nearest vertex) of a rendered face
    if (threadIdx.x == 0) { s_maxpx = 0u; s_straddle = 0u; s_zext = 0u; }
    uint32_t my_px = 0u;
    float my_zext = 0.f;
    // per tile: entries << 32 | cost (counted), or a touched-tile bitmap when the image has too many tiles; behind it the tiles'
    // list cursors
    extern __shared__ __align__(16) unsigned long long tcnt64[];
    TSETUP_INIT
    const int n = blockIdx.x;
    const int V = q.V, F = q.F, S = q.S, tiles_x = q.tiles_x;
    // the fused entry point's per-image initialisation rides along (saves a 100 MB memset and a copy launch per iteration):
    // the vertex gradient of this image starts at zero, its loss at sum |0 - target|
    if (q.d_ndc_zero) {
        float2 *z = reinterpret_cast<float2 *>(q.d_ndc_zero) + (size_t)n * V;
        for (int i = threadIdx.x; i < V; i += blockDim.x) z[i] = make_float2(0.f, 0.f);
    }
    if (q.loss_dst && threadIdx.x == 0) { q.loss_dst[n] = q.loss_src[n]; q.loss_acc[n] = 0ull; }
    if (q.cd_counter && n == 0 && threadIdx.x == 0) { q.cd_counter[0] = 0u; q.cd_counter[1] = 0u; }
    const int n_tiles = tiles_x * tiles_x;
    const bool counted = n_tiles <= COUNT_TILES_MAX;
    uint32_t *const tbits = reinterpret_cast<uint32_t *>(tcnt64);        // (!counted) touched-tile bitmap
    const int KC = counted ? q.copies : 1;                                   // copies of the per-tile words: [copy][tile]
    uint32_t *const tcur = reinterpret_cast<uint32_t *>(tcnt64 + KC * n_tiles);  // (counted) list cursor of every tile and copy
    if (counted) { for (int i = threadIdx.x; i < KC * n_tiles; i += blockDim.x) tcnt64[i] = 0ull; }
    else { for (int i = threadIdx.x; i < (n_tiles + 31) >> 5; i += blockDim.x) tbits[i] = 0u; }
    __syncthreads();
    const float *vn = q.verts_ndc + (size_t)n * V * 3;
    const float fS = (float)S;
    const int FP = faces_padded(F), FT = FP + CLIP_FX;  // ids of the front parts of cut faces start at FP; tables are FT long
    const int n_groups = FT / WAVE;
    __shared__ uint32_t s_ncut, s_unclipped;
    __shared__ int s_cut[CLIP_CUTS];
    if (threadIdx.x == 0) { s_ncut = 0u; s_unclipped = 0u; }
    // A face's tile box and nearest depth stay in the registers of the thread that computed them - pass 2 walks the faces with the same
    // f = round * blockDim.x + threadIdx.x - when the mesh has at most SETUP_REG_ROUNDS rounds (block-uniform).  The tables tbox / fzr /
    // gbox are then stored only for a reader behind this kernel: every image when the host says so (store_tables), else an image
    // whose lists turn out not to fit (write_tables below, for build_list).  The front parts of cut faces (ids from FP on) are
    // emitted by whichever thread cut their face: their rows always go through memory.
    const bool in_regs = FP <= SETUP_REG_ROUNDS * (int)blockDim.x;
    const bool store = q.store_tables != 0 || !in_regs;
    uint32_t rbox[SETUP_REG_ROUNDS], rzn[SETUP_REG_ROUNDS];
    // Corner tiles of a face's tile box that cannot hold a record of it (raster_reach.h) get neither a count nor an entry.  The four
    // flags of a face are worked out ONCE, in pass 1, and ride beside its box - four bits a round in one register - to pass 2, which
    // fills exactly the list space pass 1 counted.  Faces whose rows go through memory (the front parts of cut faces, every face of
    // a mesh of more than SETUP_REG_ROUNDS rounds) are not culled: the tables have no room for the flags.  Nor is anything culled
    // where the reach exceeds a tile (edge tiles could then fail too, and four flags would not say so) or the tiles are not counted.
    static_assert(4 * SETUP_REG_ROUNDS <= 32, "four corner flags a round in one register");
    uint32_t rcull = 0u;
    const bool cull_ok = counted && in_regs && q.sqrt_blur * fS * 0.5f + REACH_SLACK_PX <= (float)TILE;
#pragma unroll
    for (int r = 0; r < SETUP_REG_ROUNDS; ++r) { rbox[r] = 0x0000FFFFu; rzn[r] = 0u; }
    if (store)
        for (int i = threadIdx.x; i < FT - F; i += blockDim.x) q.tbox[(size_t)n * FT + F + i] = 0x0000FFFFu;  // (ids F .. FT-1: empty unless a cut face fills them)
    __syncthreads();
    TSETUP(1)
    float *const xv_n = q.clip.xv + (size_t)n * CLIP_VX * 3;
    int *const xf_n = q.clip.xf + (size_t)n * CLIP_FX * 3;
    // one face (an original one or the front part of a cut one): validity, blurred pixel box -> tile box, cost / entry per tile;
    // `carried` (a literal at every call): the face's corner flags can ride to pass 2, so its corner tiles may be culled
    auto emit = [&](int fid, float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2, float z2, float &znear, const bool carried, uint32_t &cull) -> uint32_t {
        uint32_t box = 0x0000FFFFu;  // empty: tx0 = ty0 = 255 > tx1 = ty1 = 0
        cull = 0u;
        const float zmin = fminf(fminf(z0, z1), z2), zmax = fmaxf(fmaxf(z0, z1), z2);
        znear = zmin;
        if (store || fid >= FP) q.fzr[(size_t)n * FT + fid] = make_float2(zmin, zmax);
        const float area = edge_fn(x0, y0, x1, y1, x2, y2);
        const bool finite = (x0 == x0) && (x1 == x1) && (x2 == x2) && (y0 == y0) && (y1 == y1) && (y2 == y2);
        // zmin < 1e-8: the rasteriser's own rule; zmax < z_clip: the face lies entirely nearer than MeshRasterizer's
        // z_clip_value (znear / 2) and clip_faces() removes it
        if (finite && !(zmin < K_EPS) && !(zmax < q.z_clip) && !(area <= K_EPS && area >= -K_EPS)) {
            const float fx0 = fminf(fminf(x0, x1), x2), fx1 = fmaxf(fmaxf(x0, x1), x2), fy0 = fminf(fminf(y0, y1), y2), fy1 = fmaxf(fmaxf(y0, y1), y2);
            const float xlo = fx0 - q.sqrt_blur, xhi = fx1 + q.sqrt_blur;
            const float ylo = fy0 - q.sqrt_blur, yhi = fy1 + q.sqrt_blur;
            // pixel index i (flipped axis) has centre -1 + (2i+1)/S: centres inside [lo,hi] are ceil(v_lo)..floor(v_hi)
            // with v = ((x+1) S - 1)/2; 0.01 px of slack covers the float rounding of both sides (clamped in float first: the
            // front part of a cut face can reach far outside the image)
            const float vxl = fminf(fmaxf(((xlo + 1.0f) * fS - 1.0f) * 0.5f - 0.01f, -1.0f), fS), vxh = fminf(fmaxf(((xhi + 1.0f) * fS - 1.0f) * 0.5f + 0.01f, -1.0f), fS);
            const float vyl = fminf(fmaxf(((ylo + 1.0f) * fS - 1.0f) * 0.5f - 0.01f, -1.0f), fS), vyh = fminf(fmaxf(((yhi + 1.0f) * fS - 1.0f) * 0.5f + 0.01f, -1.0f), fS);
            int xi_lo = (int)ceilf(vxl), xi_hi = (int)floorf(vxh), yi_lo = (int)ceilf(vyl), yi_hi = (int)floorf(vyh);
            xi_lo = max(xi_lo, 0); yi_lo = max(yi_lo, 0);
            xi_hi = min(xi_hi, S - 1); yi_hi = min(yi_hi, S - 1);
            if (xi_lo <= xi_hi && yi_lo <= yi_hi) {
                my_zext = fmaxf(my_zext, zmax - zmin);
                // output column xo = S-1-xi
                const int tx0 = (S - 1 - xi_hi) / TILE, tx1 = (S - 1 - xi_lo) / TILE;
                const int ty0 = (S - 1 - yi_hi) / TILE, ty1 = (S - 1 - yi_lo) / TILE;
                box = (uint32_t)tx0 | ((uint32_t)ty0 << 8) | ((uint32_t)tx1 << 16) | ((uint32_t)ty1 << 24);
                if (store || fid >= FP) q.tbox[(size_t)n * FT + fid] = box;  // (ahead of the tile loop: the address does not live through it)
                const int xo0 = S - 1 - xi_hi, xo1 = S - 1 - xi_lo, yo0 = S - 1 - yi_hi, yo1 = S - 1 - yi_lo;
                if (carried && cull_ok)  // (the limit worked out here: a value kept across the rounds would cost a register the kernel does not have)
                    cull = reach_corner_flags(reach_px_of(fx0, fS), reach_px_of(fx1, fS), reach_px_of(fy0, fS), reach_px_of(fy1, fS),
                                              xo0, xo1, yo0, yo1, tx0, tx1, ty0, ty1, S, TILE, reach_limit2(q.sqrt_blur, fS));
                for (int ty = ty0; ty <= ty1; ++ty)
                    for (int tx = tx0; tx <= tx1; ++tx) {
                        if (reach_corner_culled(cull, tx, ty, tx0, tx1, ty0, ty1)) continue;
                        const int t = ty * tiles_x + tx;
                        if (counted) {  // cost of this face in this tile: its (face, pixel) pairs plus a bit for staging it; one list entry
                            const int wx = min(xo1, tx * TILE + TILE - 1) - max(xo0, tx * TILE) + 1;
                            const int wy = min(yo1, ty * TILE + TILE - 1) - max(yo0, ty * TILE) + 1;
                            HOOK_SETUP_COUNT(atomicAdd(&tcnt64[(fid & (KC - 1)) * n_tiles + t], (1ull << 32) | (unsigned long long)(uint32_t)(wx * wy + 8));)
                        } else {
                            atomicOr(&tbits[t >> 5], 1u << (t & 31));
                        }
                    }
                my_px = max(my_px, (uint32_t)((xo1 - xo0 + 1) * (yo1 - yo0 + 1)));  // (behind the tile loop: not live through it)
            }
        }
        if ((store || fid >= FP) && box == 0x0000FFFFu) q.tbox[(size_t)n * FT + fid] = box;
        return box;
    };
    // union of a wave's 64 boxes -> the box of group `grp`: the tile kernel skips whole groups of faces with one test (images that are not binned)
    // (in DPP: a smallest value is 255 - the largest of 255 - x; no lane-index register for ds_bpermute lives through the rounds)
    auto wave_box = [&](uint32_t box) -> uint32_t {
        const uint32_t gx0 = 255u - wave_max_u32(255u - (box & 0xFFu)), gy0 = 255u - wave_max_u32(255u - ((box >> 8) & 0xFFu));
        const uint32_t gx1 = wave_max_u32((box >> 16) & 0xFFu), gy1 = wave_max_u32(box >> 24);
        return gx0 | (gy0 << 8) | (gx1 << 16) | (gy1 << 24);
    };
    auto group_box = [&](uint32_t box, int grp) {
        const uint32_t g = wave_box(box);
        if ((threadIdx.x & (WAVE - 1)) == 0 && grp < FP / WAVE) q.gbox[(size_t)n * n_groups + grp] = g;
    };
    // (the vertex ids of the NEXT round's face are requested before this round's vertices are gathered: a round is one memory
    // round trip - ids -> vertices was two - and an image is a chain of F / blockDim.x rounds)
    int nx0 = 0, nx1 = 0, nx2 = 0;
    uint32_t wave_px = 0u, wave_zext = 0u;
    if ((int)threadIdx.x < F) { nx0 = q.faces[3 * threadIdx.x]; nx1 = q.faces[3 * threadIdx.x + 1]; nx2 = q.faces[3 * threadIdx.x + 2]; }
    for (int f0 = 0; f0 < FP; f0 += blockDim.x) {  // every wave handles 64 consecutive faces per round
        const int f = f0 + threadIdx.x;
        uint32_t box = 0x0000FFFFu, cull = 0u;
        float znear = 0.f;
        const int ii[3] = {nx0, nx1, nx2};
        {
            const int fn = min(f + (int)blockDim.x, F - 1);
            nx0 = q.faces[3 * fn]; nx1 = q.faces[3 * fn + 1]; nx2 = q.faces[3 * fn + 2];
        }
        if (f < F) {
            float X[3], Y[3], Z[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { X[k] = vn[3 * ii[k]]; Y[k] = vn[3 * ii[k] + 1]; Z[k] = vn[3 * ii[k] + 2]; }
            const int nb = (Z[0] < q.z_clip ? 1 : 0) + (Z[1] < q.z_clip ? 1 : 0) + (Z[2] < q.z_clip ? 1 : 0);  // vertices behind the plane
            const bool finite = (X[0] == X[0]) && (X[1] == X[1]) && (X[2] == X[2]) && (Y[0] == Y[0]) && (Y[1] == Y[1]) && (Y[2] == Y[2]) &&
                                (Z[0] == Z[0]) && (Z[1] == Z[1]) && (Z[2] == Z[2]);
            bool cut = false;
            if (finite && (nb == 1 || nb == 2)) {  // crosses the plane: set aside for the cut loop below (rare: kept out of this loop's registers)
                atomicAdd(&s_straddle, 1u);  // (rare: straight to LDS, no register across the rounds)
                const uint32_t c = q.clip.xv ? atomicAdd(&s_ncut, 1u) : (uint32_t)CLIP_CUTS;
                if (c < (uint32_t)CLIP_CUTS) {
                    s_cut[c] = f;
                    cut = true;
                    if (store) {
                        q.tbox[(size_t)n * FT + f] = 0x0000FFFFu;  // the face itself is replaced by its front part
                        q.fzr[(size_t)n * FT + f] = make_float2(fminf(fminf(Z[0], Z[1]), Z[2]), fmaxf(fmaxf(Z[0], Z[1]), Z[2]));
                    }
                } else {
                    atomicAdd(&s_unclipped, 1u);  // beyond the tables: rendered whole, or dropped when a vertex is nearer than 1e-8 (counted)
                }
            }
            if (!cut) box = emit(f, X[0], Y[0], Z[0], X[1], Y[1], Z[1], X[2], Y[2], Z[2], znear, true, cull);
        }
        if (in_regs) {  // (the round number is uniform: a select per register, no indexed access)
#pragma unroll
            for (int r = 0; r < SETUP_REG_ROUNDS; ++r) {
                const bool here = f0 == r * (int)blockDim.x;
                rbox[r] = here ? box : rbox[r];
                rzn[r] = here ? __float_as_uint(znear) : rzn[r];
                rcull |= here ? cull << (4 * r) : 0u;
            }
        }
        if (store) group_box(box, (f0 + (int)threadIdx.x) / WAVE);
        // (the wave's largest so far ride in scalar registers; non-negative floats order like their bit patterns)
        wave_px = max(wave_px, wave_max_u32(my_px));
        wave_zext = max(wave_zext, wave_max_u32(__float_as_uint(my_zext)));
        my_px = 0u;
        my_zext = 0.f;
    }
    my_px = wave_px;
    my_zext = __uint_as_float(wave_zext);
    __syncthreads();
    TSETUP(2)
    // the faces that cross the plane: cut c owns the new vertices 2c, 2c + 1 and the front-part faces FP + 2c, FP + 2c + 1
    const uint32_t n_cut = min(s_ncut, (uint32_t)CLIP_CUTS);
    for (uint32_t c = threadIdx.x; c < n_cut; c += blockDim.x) {
        const int f = s_cut[c];
        if (q.clip.xparent) q.clip.xparent[(size_t)n * CLIP_CUTS + c] = f;
        const int ii[3] = {q.faces[3 * f], q.faces[3 * f + 1], q.faces[3 * f + 2]};
        float X[3], Y[3], Z[3];
        for (int k = 0; k < 3; ++k) { X[k] = vn[3 * ii[k]]; Y[k] = vn[3 * ii[k] + 1]; Z[k] = vn[3 * ii[k] + 2]; }
        const int nb = (Z[0] < q.z_clip ? 1 : 0) + (Z[1] < q.z_clip ? 1 : 0) + (Z[2] < q.z_clip ? 1 : 0);
        // the isolated vertex first (the one behind, or the one in front), cyclic order kept
        const int k1 = nb == 1 ? (Z[0] < q.z_clip ? 0 : (Z[1] < q.z_clip ? 1 : 2)) : (!(Z[0] < q.z_clip) ? 0 : (!(Z[1] < q.z_clip) ? 1 : 2));
        const int o1 = k1, o2 = (k1 + 1) % 3, o3 = (k1 + 2) % 3;
        const uint32_t jv = 2u * c;
        float nx[2], ny[2], zn_;
        uint32_t cull_;  // (front parts go through the tables: never culled)
        {  // the front parts' vertex ids (ahead of the arithmetic: the face's own ids do not live through it)
            const int v4 = V + (int)jv, v5 = v4 + 1;
            int *xf = xf_n + 3 * (2 * c);
            if (nb == 1) { xf[0] = v4; xf[1] = ii[o2]; xf[2] = ii[o3]; xf[3] = v4; xf[4] = ii[o3]; xf[5] = v5; }  // quadrilateral (p4, p2, p3, p5) as (p4, p2, p3) + (p4, p3, p5)
            else { xf[0] = ii[o1]; xf[1] = v4; xf[2] = v5; }                                                    // triangle (p1, p4, p5)
        }
        for (int e = 0; e < 2; ++e) {  // where the edges p1-p2 and p1-p3 cross the plane (view-space interpolation)
            const int a = o1, b = e == 0 ? o2 : o3;
            const float wb = (Z[a] - q.z_clip) / (Z[a] - Z[b]);
            const float ca = Z[a] * (1.0f - wb) / q.z_clip, cb = Z[b] * wb / q.z_clip;
            nx[e] = ca * X[a] + cb * X[b]; ny[e] = ca * Y[a] + cb * Y[b];
            float *o = xv_n + 3 * (jv + e);
            o[0] = nx[e]; o[1] = ny[e]; o[2] = q.z_clip;
            q.clip.xsrc[(size_t)n * CLIP_VX + jv + e] = make_int2(ii[a], ii[b]);
            q.clip.xcoef[(size_t)n * CLIP_VX + jv + e] = make_float2(ca, cb);
        }
        if (nb == 1) {  // quadrilateral (p4, p2, p3, p5) as (p4, p2, p3) + (p4, p3, p5)
            emit(FP + 2 * (int)c, nx[0], ny[0], q.z_clip, X[o2], Y[o2], Z[o2], X[o3], Y[o3], Z[o3], zn_, false, cull_);
            emit(FP + 2 * (int)c + 1, nx[0], ny[0], q.z_clip, X[o3], Y[o3], Z[o3], nx[1], ny[1], q.z_clip, zn_, false, cull_);
        } else {        // triangle (p1, p4, p5)
            emit(FP + 2 * (int)c, X[o1], Y[o1], Z[o1], nx[0], ny[0], q.z_clip, nx[1], ny[1], q.z_clip, zn_, false, cull_);
            q.tbox[(size_t)n * FT + FP + 2 * (int)c + 1] = 0x0000FFFFu;  // (the cut's second slot: empty - nothing else fills the rows from FP on when the tables are not stored)
        }
    }
    __syncthreads();  // the front parts' tile boxes are in place (written by whichever thread cut their face)
    TSETUP(3)
    static_assert(CLIP_FX % WAVE == 0 && SETUP_THREADS % WAVE == 0, "whole waves of front-part faces");
    auto front_group_boxes = [&]() {  // their group boxes (wave = group of 64; rows behind the last cut are empty)
        for (int i = threadIdx.x; i < CLIP_FX; i += blockDim.x) {
            const uint32_t box = i < 2 * (int)n_cut ? q.tbox[(size_t)n * FT + FP + i] : 0x0000FFFFu;
            const uint32_t g = wave_box(box);
            if ((i & (WAVE - 1)) == 0) q.gbox[(size_t)n * n_groups + FP / WAVE + i / WAVE] = g;
        }
    };
    if (store) front_group_boxes();
    if (q.clip.xcount) {
        const uint32_t nxv = 2u * n_cut;
        if (threadIdx.x == 0) q.clip.xcount[n] = nxv;
        for (int i = threadIdx.x; i < (int)nxv * 2; i += blockDim.x) q.clip.xg[(size_t)n * CLIP_VX * 2 + i] = 0.f;
    }
    if (threadIdx.x == 0 && s_unclipped) atomicAdd(&q.ctr->unclipped, s_unclipped);
    // Bound on what one vertex component of this image can receive from pass 3, up to the factor |upstream gradient| /
    // sqrt(sigma): a kept record of probability p = sigmoid(-+r^2 / sigma) adds at most 2 r p alpha |g| / sigma to an end point,
    // alpha <= 1 - p, and r p (1 - p) <= 0.197 sqrt(sigma) for every r (maximum of sqrt(u) s(u) (1 - s(u)), u = r^2 / sigma);
    // a face has at most its blurred pixel box of records; a vertex has at most max_valence faces.
    {  // over the wave first, then one LDS atomic per wave (1 024 lanes on one LDS word took 16 k cycles of a one-image launch's 103 k)
        uint32_t zb = __float_as_uint(my_zext);  // (non-negative floats order like their bit patterns)
        for (int o = 32; o > 0; o >>= 1) {
            my_px = max(my_px, (uint32_t)__shfl_xor((int)my_px, o, WAVE));
            zb = max(zb, (uint32_t)__shfl_xor((int)zb, o, WAVE));
        }
        if ((threadIdx.x & (WAVE - 1)) == 0) {
            if (my_px) atomicMax(&s_maxpx, my_px);
            if (zb) atomicMax(&s_zext, zb);
        }
    }
    __syncthreads();
    TSETUP(4)
    if (threadIdx.x == 0 && q.img_bound) {
        const float bound = 1.02f * 0.4f * (float)q.max_valence * (float)s_maxpx;
        q.img_bound[n] = bound;
        if (q.dndc_scale) {  // what the consumer of a packed gradient row multiplies by (0: the row holds plain floats)
            // (an image with cut faces accumulates in plain floats: the gradients its new vertices hand back are scaled by z / z_clip
            // factors that no a-priori bound covers)
            const bool pk = q.packed && s_ncut == 0u;
            const float sc = pk ? image_fx_scale(bound, q.pix_scale[n], q.inv_sigma) : 0.f;
            q.dndc_scale[n] = sc > 0.f ? 1.0f / sc : (pk ? -1.0f : 0.f);  // (-1: packed row that received nothing: decodes to zeros)
        }
    }
    if (threadIdx.x == 0 && s_straddle) atomicAdd(&q.ctr->straddling, s_straddle);
    // touched tiles -> the work list of their cost class
    __shared__ uint32_t s_cnt[N_CLASSES], s_base[N_CLASSES], s_ents[SETUP_THREADS / WAVE], s_binned;
    if (threadIdx.x < N_CLASSES) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    auto tile_class = [&](int t) -> int {  // -1: untouched
        if (!counted) return ((tbits[t >> 5] >> (t & 31)) & 1u) ? N_CLASSES - 1 : -1;
        uint32_t c = 0u;
        for (int k = 0; k < KC; ++k) c += (uint32_t)tcnt64[k * n_tiles + t];
        return c == 0u ? -1 : (c >= CLASS_T0 ? 0 : (c >= CLASS_T1 ? 1 : (c >= CLASS_T2 ? 2 : 3)));
    };
    uint32_t mine[N_CLASSES] = {0u, 0u, 0u, 0u};
    uint32_t my_ents = 0u;  // list entries of this thread's tiles (t = thread, thread + block, ...)
    for (int t = threadIdx.x; t < n_tiles; t += blockDim.x) {
        const int c = tile_class(t);
#pragma unroll
        for (int k = 0; k < N_CLASSES; ++k) mine[k] += (c == k) ? 1u : 0u;
        if (counted)
            for (int k = 0; k < KC; ++k) my_ents += (uint32_t)(tcnt64[k * n_tiles + t] >> 32);
    }
    uint32_t off[N_CLASSES];
#pragma unroll
    for (int k = 0; k < N_CLASSES; ++k) off[k] = mine[k] ? atomicAdd(&s_cnt[k], mine[k]) : 0u;
    // lists end to end: exclusive prefix of the entry counts over the block (thread order, each thread's tiles consecutive)
    const uint32_t incl = (uint32_t)wave_scan_add((int)my_ents);
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) s_ents[threadIdx.x / WAVE] = incl;
    __syncthreads();
    TSETUP(5)
    uint32_t ent_off = incl - my_ents;
    for (int w = 0; w < (int)(threadIdx.x / WAVE); ++w) ent_off += s_ents[w];
    if (threadIdx.x == blockDim.x - 1) s_binned = (counted && q.list_cap != 0u && ent_off + my_ents <= q.list_cap) ? 1u : 0u;
    const int part = n % N_PARTS;
    if (threadIdx.x < N_CLASSES) s_base[threadIdx.x] = s_cnt[threadIdx.x] ? atomicAdd(&q.ctr->n_class[part][threadIdx.x], s_cnt[threadIdx.x]) : 0u;
    __syncthreads();
    TSETUP(6)
    const bool binned = s_binned != 0u;
#pragma unroll
    for (int k = 0; k < N_CLASSES; ++k) off[k] += s_base[k];
    uint32_t run = ent_off;
    const uint32_t zext_bits = s_zext;  // (final since the barrier behind the atomicMax above)
    for (int t = threadIdx.x; t < n_tiles; t += blockDim.x) {
        const int c = tile_class(t);
        uint32_t e = 0u;
        const uint32_t first = run;
        if (counted)
            for (int k = 0; k < KC; ++k) {  // a tile's entries lie copy by copy inside its list
                if (binned) tcur[k * n_tiles + t] = run + e;
                e += (uint32_t)(tcnt64[k * n_tiles + t] >> 32);
            }
        run += e;
        if (c < 0) continue;
        uint32_t slot = 0u;
#pragma unroll
        for (int k = 0; k < N_CLASSES; ++k)
            if (c == k) slot = off[k]++;
        // classes 0 and 2 grow from the front of their array, 1 and 3 from the back (read back by k_colour_tiles with this formula, by
        // the silhouette kernels' `item_at` from the item's number within its partition)
        const uint32_t idx = (uint32_t)(2 * part + (c >> 1)) * q.item_cap + ((c & 1) ? q.item_cap - 1u - slot : slot);
        // the work item carries its tile's list with it: {image * tiles + tile, first entry, entries (0xFFFFFFFF: the tile kernel builds the
        // list), largest depth extent of a face of this image} - one 16-byte load in the tile kernel where the item code and a tile
        // descriptor were two dependent ones
        q.items[idx] = make_uint4((uint32_t)n * (uint32_t)n_tiles + (uint32_t)t, binned ? first : 0u, binned ? e : 0xFFFFFFFFu, zext_bits);
    }
    if (!binned) {  // (block-uniform)
        // The tile kernel builds this image's lists itself, from the tables: nobody stored them yet - the boxes come from the registers,
        // a face's depth range from its vertices again (min / max of the same three floats; this is the rare image, and a third
        // register a round for the farthest depth would cost every image), the rows behind the last cut face's front parts are empty.
        if (!store) {
            for (int i = threadIdx.x + 2 * (int)n_cut; i < CLIP_FX; i += blockDim.x) q.tbox[(size_t)n * FT + FP + i] = 0x0000FFFFu;
#pragma unroll
            for (int r = 0; r < SETUP_REG_ROUNDS; ++r) {
                const int f = r * (int)blockDim.x + (int)threadIdx.x;
                if (r * (int)blockDim.x < FP) {
                    if (f < FP) q.tbox[(size_t)n * FT + f] = rbox[r];
                    if (f < F) {
                        const float z0 = vn[3 * q.faces[3 * f] + 2], z1 = vn[3 * q.faces[3 * f + 1] + 2], z2 = vn[3 * q.faces[3 * f + 2] + 2];
                        q.fzr[(size_t)n * FT + f] = make_float2(fminf(fminf(z0, z1), z2), fmaxf(fmaxf(z0, z1), z2));
                    }
                    group_box(rbox[r], f / WAVE);
                }
            }
            front_group_boxes();
        }
        return;
    }
    __syncthreads();
    TSETUP(7)
    // pass 2: every face to the lists of the tiles of its box (box and nearest depth from this thread's registers; the front parts of
    // cut faces, and every face of a mesh of more than SETUP_REG_ROUNDS rounds, from the tables: back from L1 / L2)
    uint2 *const lists = q.lists + (size_t)n * q.list_cap;
    // (consecutive faces cover the same tiles: their entries take consecutive slots, so a wave's stores land in few cache lines;
    // spreading the lanes over distant faces to thin out the same-address atomics was measured slower, 601 -> 658 us)
    const int f_end = FP + 2 * (int)n_cut;  // (the rows behind the last cut face's front parts are empty)
    auto bin_face = [&](int f, uint32_t box, uint32_t znear_bits, uint32_t cull) {
        const uint2 ent = make_uint2((uint32_t)f, znear_bits);
        const int tx0 = box & 0xFF, ty0 = (box >> 8) & 0xFF, tx1 = (box >> 16) & 0xFF, ty1 = box >> 24;
        if (tx0 > tx1) return;
        uint32_t *const cur = tcur + (f & (KC - 1)) * n_tiles;
        // (a fast path for boxes of at most 2 x 2 tiles - the four returning atomics issued before the four stores - measured no
        // different, profiles/r5_experiments.md)
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx)
                if (!reach_corner_culled(cull, tx, ty, tx0, tx1, ty0, ty1)) at(lists, atomicAdd(&cur[ty * tiles_x + tx], 1u)) = ent;  // (pass 1's flags: its count)
    };
    if (in_regs) {
#pragma unroll
        for (int r = 0; r < SETUP_REG_ROUNDS; ++r)
            if (r * (int)blockDim.x < FP) bin_face(r * (int)blockDim.x + (int)threadIdx.x, rbox[r], rzn[r], (rcull >> (4 * r)) & 15u);  // (rows from FP on: empty boxes)
    }
    for (int f = (in_regs ? FP : 0) + (int)threadIdx.x; f < f_end; f += blockDim.x)
        bin_face(f, q.tbox[(size_t)n * FT + f], __float_as_uint(q.fzr[(size_t)n * FT + f].x), 0u);  // (one round trip: both requested together)
    TSETUP(8)
    TSETUP_REPORT
}

__global__ void __launch_bounds__(256) k_unpack_dndc(float *__restrict__ d_ndc, const float *__restrict__ img_bound,
                                                     const float *__restrict__ pix_scale, float inv_sigma, int V,
                                                     const uint32_t *__restrict__ xcount) {
    const int n = blockIdx.x, v = blockIdx.y * blockDim.x + threadIdx.x;
    if (v >= V || (xcount && xcount[n] != 0u)) return;  // (images with cut faces hold plain floats already)
    const float sc = image_fx_scale(img_bound[n], pix_scale[n], inv_sigma);
    const float inv = sc > 0.f ? 1.0f / sc : 0.f;
    unsigned long long *p = reinterpret_cast<unsigned long long *>(d_ndc) + (size_t)n * V + v;
    const unsigned long long tot = *p;
    const int qy = (int)(uint32_t)tot;
    const int qx = (int)(uint32_t)((tot - (unsigned long long)(long long)qy) >> 32);
    *reinterpret_cast<float2 *>(p) = make_float2((float)qx * inv, (float)qy * inv);
}

// Gradient of the new vertices of cut faces back to the end points of the edges they lie on: xy_new = c_a xy_a + c_b xy_b with the
// coefficients held constant (see ClipTables).  One workgroup per image; images without cut faces leave at once.  Images with
// cut faces accumulate in plain floats, so these are float atomics on d_ndc (two new vertices may share an end point).
__global__ void __launch_bounds__(64) k_clip_backward(ClipTables c, float *__restrict__ d_ndc, int V, float *__restrict__ loss_img,
                                                      const unsigned long long *__restrict__ loss_acc, const float *__restrict__ verts_ndc,
                                                      float z_clip, SmilClipDepth cd, int image0) {
    const int n = blockIdx.x;
    // (fused entry point: the image's loss = what the setup kernel seeded it with + the tiles' terms, summed as integers)
    if (loss_img && threadIdx.x == 0) loss_img[n] += (float)((double)(long long)loss_acc[n] * (1.0 / 4294967296.0));
    const uint32_t nx = c.xcount[n];
    // Depth channel (round 5): the crossing point xy_new = (xy_a z_a (1 - w) + xy_b z_b w) / z_clip, w = (z_a - z_clip) / (z_a - z_b), also
    // depends on the end points' DEPTHS - pytorch3d's autograd differentiates clip_faces through them.  d_ndc has no depth
    // component, so these (rare) terms travel as a sparse list: two entries {vertex, d / d z} per new vertex, the image's run
    // recorded in cd.range; the LBS backward / smil_clip_depth_backward carry them through the camera.
    __shared__ uint32_t s_first;
    if (cd.range) {
        if (threadIdx.x == 0) {
            uint32_t first = 0u, cnt = 0u;
            if (nx) {
                first = atomicAdd(&cd.counter[0], 2u * nx);
                if (first + 2u * nx <= (uint32_t)cd.capacity) cnt = 2u * nx;
                else atomicAdd(&cd.counter[1], 2u * nx);  // (does not fit: dropped, counted; the run stays reserved but unused)
            }
            cd.range[2 * (size_t)(image0 + n)] = first;
            cd.range[2 * (size_t)(image0 + n) + 1] = cnt;
            s_first = cnt ? first : 0xFFFFFFFFu;
        }
        __syncthreads();
    }
    const uint32_t zfirst = cd.range ? s_first : 0xFFFFFFFFu;
    const float *vn = verts_ndc + (size_t)n * V * 3;
    for (uint32_t j = threadIdx.x; j < nx; j += blockDim.x) {
        const float gx = c.xg[((size_t)n * CLIP_VX + j) * 2], gy = c.xg[((size_t)n * CLIP_VX + j) * 2 + 1];
        const int2 ab = c.xsrc[(size_t)n * CLIP_VX + j];
        if (zfirst != 0xFFFFFFFFu) {
            const float xa = vn[3 * ab.x], ya = vn[3 * ab.x + 1], za = vn[3 * ab.x + 2];
            const float xb = vn[3 * ab.y], yb = vn[3 * ab.y + 1], zb = vn[3 * ab.y + 2];
            // xy_new = xy_a (1 - s) + xy_b s with s = z_b w / z_clip (the two weights sum to one: the crossing's depth is z_clip), so both
            // derivatives point along the edge: d xy_new / d z_a = (xy_b - xy_a) z_b (z_clip - z_b) / (z_clip (z_a - z_b)^2) and
            // d xy_new / d z_b = (xy_b - xy_a) z_a (z_a - z_clip) / (z_clip (z_a - z_b)^2).  Expanding them from the w form instead
            // cancels two terms of size |xy| |z| / z_clip against each other in fp32 (profiles/r5_fuzz.md).
            const float inv = 1.0f / (za - zb);
            const float ge = fmaf(gx, xb - xa, gy * (yb - ya)) * (inv * inv) * (1.0f / z_clip);
            cd.vertex[zfirst + 2u * j] = ab.x;
            cd.dz[zfirst + 2u * j] = ge * (zb * (z_clip - zb));
            cd.vertex[zfirst + 2u * j + 1u] = ab.y;
            cd.dz[zfirst + 2u * j + 1u] = ge * (za * (za - z_clip));
        }
        if (gx == 0.f && gy == 0.f) continue;
        const float2 co = c.xcoef[(size_t)n * CLIP_VX + j];
        float *da = d_ndc + ((size_t)n * V + ab.x) * 2, *db = d_ndc + ((size_t)n * V + ab.y) * 2;
        atomicAdd(da, co.x * gx); atomicAdd(da + 1, co.x * gy);
        atomicAdd(db, co.y * gx); atomicAdd(db + 1, co.y * gy);
    }
}
