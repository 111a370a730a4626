// The tile kernel k_raster_dense and what only it uses (raster.hip; see the map of the headers there).
#pragma once

// ---------------------------------------------------------------------------------------------
// tile kernel
// ---------------------------------------------------------------------------------------------
#ifndef GCHUNK
#define GCHUNK 64            // faces whose gradient accumulators are live in pass 3 (a multiple of WAVE)
#endif
#ifndef GCOPIES
#define GCOPIES 2
#endif
//      GCOPIES              // private copies of those accumulators (measured: 1 -> 2 copies -3 %, 4 copies lose it again to zeroing and flushing)
struct alignas(16) DenseLds {
    union {
        float rec[DCHUNK * FSTR];    // pass 1: staged face records
        struct {
            // pass 3: gradient accumulators of GCHUNK faces x 3 vertices, (x, y) packed as two 32-bit fixed-point numbers
            // in one 64-bit word so that one ds_add_u64 adds both; GCOPIES private copies indexed by lane & (GCOPIES - 1)
            // keep the consecutive lanes of one face's run of records off each other's address (measured: the four
            // 13-way conflicting ds_add_f64 per record this replaces were more than half of pass 3)
            unsigned long long gacc[GCOPIES][GCHUNK * 3];
            double plog[WAVE];       // pass 2: sum of log2(1 - p_k) (fp64: ds_add_f64 runs at full rate on gfx950,
                                     //         ds_add_f32 at ~3 cycles per active lane)
            float4 pgrad[WAVE];      // after pass 1: {gradient coefficient, threshold depth bits, tie cut (face id), -}
        };
    };
    // select: [bucket / 2][pixel], two 16-bit counts per word; the first digit is counted by pass 1
    uint32_t hist[(1 << SEL_BITS) / 2 * WAVE];
    float2 pixt[WAVE];               // pass 1: pixel centre (px, py) in NDC
    uint2 psel[WAVE];                // select: {prefix of the wanted key, rank wanted among the keys sharing it (0: none)}
    int start[WAVE];                 // pass 1: 2048-bit map of the pairs that start a face's run (list phase: bucket counters)
    uint16_t bstart[1 << SEL1_BITS]; // first list position of every depth bucket of the near-to-far list (clamped to 65535)
};
static_assert(sizeof(DenseLds) * RESIDENT_PER_CU <= 160 * 1024, "the resident workgroups of a CU must fit its 160 KB of LDS");

// Record-stream accesses: written once, read once or twice, never shared between workgroups (non-temporal forms measured 12 % slower
// in round 2: the streams do live on L2 / Infinity Cache hits between pass 1 and the sweeps).
template <typename T> __device__ __forceinline__ T ld_stream(const T *base, uint32_t i) { return at(base, i); }
template <typename T> __device__ __forceinline__ void st_stream(T *base, uint32_t i, T v) { at(base, i) = v; }

// Single-wave workgroups: lanes exchange data through LDS without s_barrier, but the compiler must not forward a lane's
// own store to its later load, and the LDS queue must have drained.  Unlike __syncthreads() this does NOT wait for
// outstanding global stores (vmcnt), which in pass 1 would stall every sweep step on the previous step's record stores.
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// the staged face record of pass 1 as its seven rows (FaceRows)
__device__ __forceinline__ FaceRows load_face_rows(const float *rec) {
    const float4 *r = reinterpret_cast<const float4 *>(rec);
    return FaceRows{r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
}

#ifndef LGROUP
#define LGROUP 8  // 64-face groups whose tile boxes / depth ranges are requested together by the list build
#endif
// Ordered list of the faces whose tile box contains (tx,ty), written to `list` (global).  Also the range of the nearest /
// farthest vertex depth over those faces: every pair depth lies inside it (a convex combination of the face's vertex
// depths), which fixes the radix-select digits before pass 1 starts.  Depths are positive: the bit patterns order like
// the values.
__device__ __forceinline__ int build_list(const RasterArgs &a, int n, int tx, int ty, uint2 *list, int lane, uint32_t &kmin,
                                          uint32_t &kmax) {
    const uint32_t *__restrict__ tbox_n = a.tbox + (size_t)n * a.FT;
    const float2 *__restrict__ fzr_n = a.fzr + (size_t)n * a.FT;
    const int n_groups = a.FT / WAVE;
    const uint32_t *__restrict__ gbox_n = a.gbox + (size_t)n * n_groups;
    int cnt = 0;
    float zlo = 3.0e38f, zhi = 0.f;
    for (int g0 = 0; g0 < n_groups; g0 += WAVE) {
        // lane = group of 64 consecutive faces: does its box union reach this tile?
        const int g = g0 + lane;
        unsigned long long gm = __ballot(g < n_groups && box_has(gbox_n[min(g, n_groups - 1)], tx, ty));
        while (gm) {  // wave-uniform: the groups that do, in ascending order, LGROUP at a time (independent loads in flight)
            int fidx[LGROUP];
            uint32_t tb[LGROUP];
            float2 zz[LGROUP];
#pragma unroll
            for (int u = 0; u < LGROUP; ++u) {
                const int gi = gm ? g0 + (int)__builtin_ctzll(gm) : -1;
                gm &= gm - 1ull;  // 0 stays 0
                fidx[u] = gi >= 0 ? gi * WAVE + lane : a.FT;
                const int fc = min(fidx[u], a.FT - 1);
                tb[u] = tbox_n[fc];
                zz[u] = fzr_n[fc];
            }
#pragma unroll
            for (int u = 0; u < LGROUP; ++u) {
                const bool hit = fidx[u] < a.FT && box_has(tb[u], tx, ty);
                const unsigned long long mask = __ballot(hit);
                if (hit) {
                    at(list, (uint32_t)(cnt + __popcll(mask & ((1ull << lane) - 1ull)))) = make_uint2((uint32_t)fidx[u], __float_as_uint(zz[u].x));
                    zlo = fminf(zlo, zz[u].x);
                    zhi = fmaxf(zhi, zz[u].y);
                }
                cnt += __popcll(mask);
            }
        }
    }
    uint32_t lo = __float_as_uint(zlo), hi = __float_as_uint(zhi);
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, WAVE));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, WAVE));
    }
    kmin = lo;
    kmax = hi;
    return cnt;
}

// Near-to-far order for the tile's list: a counting sort of the faces by the first radix digit (the same digit the
// records' depths are histogrammed by) of their NEAREST vertex depth.  A record's depth is at least its face's nearest
// vertex depth, so once every face of digit <= d has been processed the per-pixel record counts of digits <= d are final:
// pass 1 uses that to stop collecting records for pixels that already hold K nearer ones (the reference keeps the K = 100
// nearest per pixel, p3d_renderer.py:42-47), and to leave the tile when no pixel is open any more.
// Order inside a bucket is arbitrary; depth ties between records are broken by face id, which the records' list position
// recovers through `out`.  bstart[d] = first position of bucket d.
__device__ __forceinline__ void sort_list_near_to_far(const uint2 *list, uint32_t *out, int n, uint32_t kmin, int shift1, int b1,
                                                      DenseLds &lds, int lane) {
    const int n_buckets = 1 << b1;
    lds.start[lane] = 0;
    __syncthreads();
    auto digit_of = [&](const uint2 &e) { return (int)(((e.y - kmin) >> shift1) & (uint32_t)(n_buckets - 1)); };
    // (four rows per step: the loads of a step are in flight together - at small launches a tile's time is its chain of
    // memory round trips)
    for (int i0 = 0; i0 < n; i0 += 4 * WAVE) {
        uint2 e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = at(list, (uint32_t)min(i0 + u * WAVE + lane, n - 1));
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * WAVE + lane < n) atomicAdd(&lds.start[digit_of(e[u])], 1);
    }
    __syncthreads();
    const int c = lane < n_buckets ? lds.start[lane] : 0;
    const int incl = wave_scan_add(c);
    __syncthreads();
    if (lane < n_buckets) lds.bstart[opaque_lane(lane)] = (uint16_t)min(incl - c, 65535);
    lds.start[lane] = incl - c;  // running cursor of every bucket
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 4 * WAVE) {
        uint2 e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = at(list, (uint32_t)min(i0 + u * WAVE + lane, n - 1));
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * WAVE + lane < n) out[atomicAdd(&lds.start[digit_of(e[u])], 1)] = e[u].x;
    }
    __syncthreads();
}

// Staging of a chunk of DCHUNK = 32 faces by all 64 lanes: lanes l and l + 32 share face l.  The LOW lane builds the affine
// forms (rows 1-3 of the record) and the pixel ROWS the face's blurred box covers inside the open part of the tile; the
// HIGH lane the bounding box (row 0), the edge data (rows 4-7) and the pixel COLUMNS; rows and columns are cut to what the blur
// disc of the face's bounding box reaches (the lanes swap their gaps: one ds_bpermute), the columns then cross over (one more,
// both ends in one word) and the low lane leaves with the face's pair count `cf` and the word pairs decode their pixel from.
// Both lanes load the same nine vertex floats (one transaction); the face's vertex indices (i0, i1, i2) come from the
// caller, which fetched them while the previous chunk was being evaluated.  Pixel index i (flipped axis) has centre -1 + (2i+1)/S:
// centres inside [lo, hi] are ceil(v_lo) .. floor(v_hi) with v = ((x+1) S - 1)/2; 0.01 px of slack covers the float rounding
// (a superset; eval_pair applies the exact test).
static_assert(2 * DCHUNK == WAVE, "two lanes per staged face");
__device__ __forceinline__ void stage_faces(const RasterArgs &a, const Tri9 &tv, int i0, int i1, int i2, int m,
                                            float *rec, int lane, float cx, float cy, float fS, int tx, int ty, int ox0, int ox1,
                                            int oy0, int oy1, unsigned long long open_px, int &cf, int &packed2, float2 *__restrict__ sxy,
                                            TriIds *__restrict__ sid, int c0, int list_stride) {
    const int slot = lane & (DCHUNK - 1);
    const bool hi = lane >= DCHUNK;
    int b0 = 0, b1 = -1;  // low lane: box rows by0 .. by1; high lane: box columns bx0 .. bx1
    float c_lo = 0.f, c_hi = 0.f;  // the face's unblurred extent on the lane's axis (NDC)
    if (slot < m) {
        const float x0 = tv.x0, y0 = tv.y0, x1 = tv.x1, y1 = tv.y1, x2 = tv.x2, y2 = tv.y2;
        float4 *r = reinterpret_cast<float4 *>(rec + slot * FSTR);
        // The tile's vertex table for pass 3: three arrays of float2 (v0, v1, v2 by list position) and the vertex ids, so that every
        // store instruction writes whole runs of bytes (one 24-byte structure per face, stored as 16 + 8 bytes, cost 0.45 ms per
        // cfg2b launch in partial-line writes; this form 0.1): v0 from the low lanes and v1 from the high lanes in one instruction
        at(sxy, (uint32_t)((hi ? list_stride : 0) + c0 + slot)) = hi ? make_float2(x1, y1) : make_float2(x0, y0);
        if (!hi) {
            at(sid, (uint32_t)(c0 + slot)) = TriIds{i0, i1, i2};
            face_rows_lo(tv, cx, cy, r[0], r[1], r[2]);
            const float ymin = fminf(fminf(y0, y1), y2) - a.sqrt_blur, ymax = fmaxf(fmaxf(y0, y1), y2) + a.sqrt_blur;
            const int yi_lo = (int)ceilf(((ymin + 1.0f) * fS - 1.0f) * 0.5f - 0.01f), yi_hi = (int)floorf(((ymax + 1.0f) * fS - 1.0f) * 0.5f + 0.01f);
            b0 = max(a.S - 1 - yi_hi - ty * TILE, oy0);
            b1 = min(a.S - 1 - yi_lo - ty * TILE, oy1);
            c_lo = fminf(fminf(y0, y1), y2); c_hi = fmaxf(fmaxf(y0, y1), y2);
        } else {
            const float xmin = fminf(fminf(x0, x1), x2) - a.sqrt_blur, xmax = fmaxf(fmaxf(x0, x1), x2) + a.sqrt_blur;
            float rl12;
            face_rows_hi(tv, cx, cy, r[3], r[4], r[5], rl12);
            r[6] = make_float4(rl12, __int_as_float(i0), __int_as_float(i1), __int_as_float(i2));
            at(sxy, (uint32_t)(2 * list_stride + c0 + slot)) = make_float2(x2, y2);  // (the table, see above)
            const int xi_lo = (int)ceilf(((xmin + 1.0f) * fS - 1.0f) * 0.5f - 0.01f), xi_hi = (int)floorf(((xmax + 1.0f) * fS - 1.0f) * 0.5f + 0.01f);
            b0 = max(a.S - 1 - xi_hi - tx * TILE, ox0);
            b1 = min(a.S - 1 - xi_lo - tx * TILE, ox1);
            c_lo = fminf(fminf(x0, x1), x2); c_hi = fmaxf(fmaxf(x0, x1), x2);
        }
    }
    // The rectangle above is the blurred SQUARE cut to the tile and its open pixels; a record needs dx^2 + dy^2 < blur (raster_reach.h).
    // Each lane works out how far its run of rows / columns stays from the face's extent on its axis, the two lanes of a face swap
    // these gaps, and each cuts its run to what the other's gap leaves of the reach: the rounded box.  (Both lanes run the same
    // code on their own axis; one round - a run cut here could shorten the other's again, which was not worth a second exchange.)
    {
        const int edge = a.S - 1 - (hi ? tx : ty) * TILE;  // pixel index (flipped axis) of the tile's first row / column
        const bool any = b0 <= b1;
        const float vlo = reach_px_of(c_lo, fS), vhi = reach_px_of(c_hi, fS);
        const float gap = any ? reach_gap(vlo, vhi, edge - b1, edge - b0) : 0.f;
        const float gap_other = __shfl(gap, lane ^ DCHUNK, WAVE);  // (all lanes: no divergent ds_bpermute)
        if (any) {
            int i_lo = edge - b1, i_hi = edge - b0;
            float sb = a.sqrt_blur;
            asm volatile("" : "+v"(sb));  // (the limit is worked out per chunk, three instructions, and not kept in a register across the chunks)
            reach_trim(vlo, vhi, gap_other, reach_limit2(sb, fS), i_lo, i_hi);
            b0 = edge - i_hi;
            b1 = edge - i_lo;
        }
    }
    const int bxx = __shfl(b0 <= b1 ? (b0 | (b1 << 4)) : 1, slot + DCHUNK, WAVE);  // the columns cross over: bx0 | bx1 << 4 (empty: 1 | 0)
    int bx0 = bxx & 15, bx1 = bxx >> 4;
    cf = 0;
    packed2 = 0;
    if (!hi && slot < m && bx0 <= bx1 && b0 <= b1) {
        // shrink the box to the open pixels inside it (bit 8 * row + column of `open_px`): between two closing steps the
        // open pixels of a tile are often scattered, and their common bounding box (ox0 .. oy1) is then the whole tile
        const uint32_t colb = ((2u << bx1) - (1u << bx0)) * 0x01010101u;                  // columns bx0 .. bx1 of every row
        const unsigned long long rows = (b1 >= 7 ? ~0ull : ((1ull << (8 * (b1 + 1))) - 1ull)) & ~((1ull << (8 * b0)) - 1ull);
        const unsigned long long mbox = open_px & rows & (((unsigned long long)colb << 32) | colb);
        if (mbox == 0ull) {
            b1 = b0 - 1;
        } else {
            b0 = (int)(__builtin_ctzll(mbox) >> 3);
            b1 = (int)((63 - __builtin_clzll(mbox)) >> 3);
            uint32_t c8 = (uint32_t)mbox | (uint32_t)(mbox >> 32);
            c8 |= c8 >> 16;
            c8 = (c8 | (c8 >> 8)) & 0xFFu;
            bx0 = (int)__builtin_ctz(c8);
            bx1 = 31 - (int)__builtin_clz(c8);
        }
    }
    if (!hi && slot < m && bx0 <= bx1 && b0 <= b1) {
        // the box in PIXEL PAIRS (columns 2c, 2c + 1 of one row; pair index = pixel index / 2): a lane of the sweep evaluates one
        const int cp0 = bx0 >> 1, bw = (bx1 >> 1) - cp0 + 1;   // 1 ... 4 pairs per row
        cf = bw * (b1 - b0 + 1);
        // what a lane needs to find its pixel pair: lane r of the box sits in box row r / bw, computed as (r * inv) >> 16 with
        // inv = floor(65536 / bw) + 1 (exact for r < 32, bw <= 4: the reciprocal is exact for 1, 2, 4 and 1e-4 away from an
        // integer otherwise), and its pair is first + r + (r / bw) * (4 - bw)
        const int inv = (int)(65536.0f * __builtin_amdgcn_rcpf((float)bw)) + 1;
        packed2 = inv | ((TILE / 2 - bw) << 17) | ((b0 * (TILE / 2) + cp0) << 20);
    }
}

// lane = pixel: in the histogram `hist` ([bucket / 2][pixel]) find the digit that holds the `need`-th smallest key.
// Returns the number of keys counted for this pixel; updates (pre, need) and reports the count of the chosen digit.
__device__ __forceinline__ int pick_digit(const uint32_t *hist, int lane, int b, uint32_t &pre, int &need, int &n_eq) {
    uint32_t hw[(1 << SEL_BITS) / 2];
#pragma unroll
    for (int w_ = 0; w_ < (1 << SEL_BITS) / 2; ++w_) hw[w_] = hist[w_ * WAVE + lane];  // (all reads in flight together)
    // Running sums c_k are non-decreasing: the chosen bucket is the number of c_k below `need`, the keys in lower buckets the largest
    // such c_k, and the chosen bucket ends at the first c_k that reaches `need`.  Arithmetic selects only (as a chain of `if`s this
    // was thirty-two exec-masked branches per call).
    int c = 0, sel = 0, below = 0, first_ge = 0x7FFFFFFF;
#pragma unroll
    for (int k = 0; k < (1 << SEL_BITS); ++k) {
        c += (k & 1) ? (int)(hw[k >> 1] >> 16) : (int)(hw[k >> 1] & 0xFFFFu);
        const bool lt = c < need;
        sel += lt ? 1 : 0;
        below = lt ? c : below;
        first_ge = min(first_ge, lt ? 0x7FFFFFFF : c);
    }
    if (need > 0 && c >= need) {
        pre = (pre << b) | (uint32_t)sel;
        need -= below;
        n_eq = first_ge - below;
    } else {
        need = 0;  // fewer keys than the rank asked for: this pixel keeps everything
        n_eq = 0;
    }
    return c;
}

// The same for the first digit, whose histogram holds four 8-bit counts per word ([bucket / 4][pixel]) that stop growing at
// SAT8 > K: the cumulative counts below the chosen digit are exact (they are below `need` <= K), a count that reached SAT8
// only ever compares as "more than K".
__device__ __forceinline__ int pick_digit8(const uint32_t *hist, int lane, int b, uint32_t &pre, int &need, int &n_eq) {
    int cum = 0, sel = 0, cnt_sel = 0, all = 0;
    bool found = false;
#pragma unroll
    for (int w_ = 0; w_ < (1 << SEL1_BITS) / 4; ++w_) {
        const uint32_t hw = hist[w_ * WAVE + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int h = (int)((hw >> (8 * q)) & 0xFFu);
            all += h;
            if (!found && cum + h >= need) { sel = 4 * w_ + q; cnt_sel = h; found = true; }
            cum += found ? 0 : h;
        }
    }
    if (need > 0 && found) {
        pre = (pre << b) | (uint32_t)sel;
        need -= cum;
        n_eq = cnt_sel;
    } else {
        need = 0;
        n_eq = 0;
    }
    return all;
}

// One radix-select sweep over `n_rec` (key, meta) pairs: among the keys of pixel p whose bits above `nbits` equal
// psel[p].x, histogram the next `b` bits (psel[p].y == 0: pixel not taking part; key 0xFFFFFFFF: record not taking part).
template <typename KeyFn>
__device__ __forceinline__ void select_sweep(DenseLds &lds, const Rec3 *__restrict__ crec, int n_rec, int nbits, int b,
                                             int lane, uint32_t pre, int need, KeyFn key_of) {
    const int shift = nbits - b;
    lds.psel[lane] = make_uint2(pre, (uint32_t)need);
    for (int i_ = lane; i_ < (1 << SEL_BITS) / 2 * WAVE; i_ += WAVE) lds.hist[i_] = 0u;
    __syncthreads();
    auto load_keys = [&](uint32_t (&kk)[KGROUP], uint32_t (&mt)[KGROUP], int g0) {
#pragma unroll
        for (int u = 0; u < KGROUP; ++u) {
            const uint32_t idx = (uint32_t)min(g0 + u * WAVE + lane, n_rec - 1);  // unsigned 32-bit: SGPR base + VGPR offset addressing
            mt[u] = at(crec, idx).b;
            kk[u] = key_of(idx, mt[u]);
        }
    };
    auto count_keys = [&](const uint32_t (&kk)[KGROUP], const uint32_t (&mt)[KGROUP], int g0) {
        uint2 ps[KGROUP];  // all LDS gathers first: one latency, not one per row
#pragma unroll
        for (int u = 0; u < KGROUP; ++u) ps[u] = lds.psel[mt[u] & 63u];
#pragma unroll
        for (int u = 0; u < KGROUP; ++u) {
            const uint32_t pxl = mt[u] & 63u;
            const bool hit = (g0 + u * WAVE + lane < n_rec) & (ps[u].y > 0u) & ((kk[u] >> nbits) == ps[u].x) & (kk[u] != 0xFFFFFFFFu);
            const uint32_t bucket = (kk[u] >> shift) & ((1u << b) - 1u);
            if (hit) atomicAdd(&lds.hist[(bucket >> 1) * WAVE + pxl], (bucket & 1u) ? 0x10000u : 1u);
        }
    };
    if (n_rec > 0) {  // double-buffered: the next KGROUP rows are in flight while this one is counted
        uint32_t ka[KGROUP], ma[KGROUP], kb[KGROUP], mb[KGROUP];
        load_keys(ka, ma, 0);
        for (int g0 = 0; g0 < n_rec; g0 += 2 * KGROUP * WAVE) {
            load_keys(kb, mb, g0 + KGROUP * WAVE);
            count_keys(ka, ma, g0);
            load_keys(ka, ma, g0 + 2 * KGROUP * WAVE);
            count_keys(kb, mb, g0 + KGROUP * WAVE);
        }
    }
    __syncthreads();
}

// One refinement step of the radix select over the compact stream, which SHRINKS as it goes.  Among the records of pixel p
// (still selecting: psel[p].y > 0) the bits of the key above `nbits` are compared with the prefix psel[p].x chosen so far:
//   below it  -> the record lies in a lower bucket of the digit picked last: it is among the K nearest for certain, its log
//                factor goes to the pixel's sum and the record leaves the stream;
//   equal     -> it stays (compacted IN PLACE: the write position never passes the read position, and every lane has
//                loaded its record before any lane of the same step stores) and its next `b` bits are histogrammed;
//   above     -> dropped.
// Returns the number of records left.  Every later sweep thus reads only the records that are still undecided (a tenth per
// digit) instead of the whole compact stream, and the final pass only sees the last bucket.
__device__ __forceinline__ int refine_sweep(DenseLds &lds, Rec3 *crec, int n_rec, int nbits, int b,
                                            int lane, uint32_t pre, int need) {
    const int shift = nbits - b;
    lds.psel[lane] = make_uint2(pre, (uint32_t)need);
    for (int i_ = lane; i_ < (1 << SEL_BITS) / 2 * WAVE; i_ += WAVE) lds.hist[i_] = 0u;
    __syncthreads();
    int n_out = 0;
    struct CRec { uint32_t kk, mt; float lf; };
    auto load_recs = [&](CRec (&r)[KGROUP], int g0) {
#pragma unroll
        for (int u = 0; u < KGROUP; ++u) {
            const uint32_t idx = (uint32_t)min(g0 + u * WAVE + lane, n_rec - 1);
            const Rec3 q = at(crec, idx);
            r[u].kk = q.a; r[u].mt = q.b; r[u].lf = __uint_as_float(q.c);
        }
    };
    auto sift_rows = [&](auto rows, const CRec (&r)[KGROUP], int g0) {  // (rows.has: sweep_rows)
        uint2 ps[KGROUP];  // all LDS gathers first: one latency, not one per row
#pragma unroll
        for (int u = 0; u < KGROUP; ++u)
            if (rows.has(u)) ps[u] = lds.psel[r[u].mt & 63u];
#pragma unroll
        for (int u = 0; u < KGROUP; ++u) {
            if (!rows.has(u)) continue;
            const uint32_t pxl = r[u].mt & 63u;
            const bool live = (g0 + u * WAVE + lane < n_rec) & (ps[u].y > 0u);
            const uint32_t top = r[u].kk >> nbits;
            const bool sure = live & (top < ps[u].x), stay = live & (top == ps[u].x);
            if (sure & (r[u].lf != 0.f)) atomicAdd(&lds.plog[pxl], (double)r[u].lf);
            const unsigned long long sm = __ballot(stay);
            const uint32_t slot = (uint32_t)n_out + __builtin_amdgcn_mbcnt_hi((uint32_t)(sm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sm, 0u));
            if (stay) {
                at(crec, slot) = Rec3{r[u].kk, r[u].mt, __float_as_uint(r[u].lf)};
                const uint32_t bucket = (r[u].kk >> shift) & ((1u << b) - 1u);
                atomicAdd(&lds.hist[(bucket >> 1) * WAVE + pxl], (bucket & 1u) ? 0x10000u : 1u);
            }
            n_out += __popcll(sm);
        }
    };
    if (n_rec > 0) {  // double-buffered: the next KGROUP rows are in flight while this one is sifted
        CRec ra[KGROUP], rb[KGROUP];
        load_recs(ra, 0);
        sweep_rows<KGROUP>(0, n_rec, ra, rb, load_recs, sift_rows);
    }
    __syncthreads();
    return n_out;
}

template <int MODE>
__global__ void __launch_bounds__(64, WAVES_PER_SIMD) k_raster_dense(RasterArgs a) {
    __shared__ DenseLds lds;
    const int lane = threadIdx.x;
    uint2 *const slist = a.slist + (size_t)blockIdx.x * a.list_stride;
    uint32_t *const slist2 = a.slist2 + (size_t)blockIdx.x * a.list_stride;
    uint32_t *const scfirst = a.scfirst + (size_t)blockIdx.x * a.n_cf;
    float2 *const sxy = a.sxy + (size_t)blockIdx.x * 3 * a.list_stride;
    TriIds *const sid = a.sid + (size_t)blockIdx.x * a.list_stride;
    const size_t rec0 = (size_t)blockIdx.x * (REC_CAP + REC_PAD);
    Rec3 *const srec = a.srec + rec0, *const crec = a.crec + rec0;
    const uint32_t lane_lo = lane < 32 ? 1u << lane : 0u, lane_hi = lane >= 32 ? 1u << (lane - 32) : 0u;
    const int K = a.K;
    const int n_tiles = a.tiles_x * a.tiles_x;
    unsigned int n_items_all = 0;
    for (int q = 0; q < N_PARTS; ++q)
        for (int c = 0; c < N_CLASSES; ++c) n_items_all += a.ctr->n_class[q][c];
    // With fewer tiles than workgroups (a handful of images) every tile is dealt out as 2, 4 or 8 runs of pixels, so that
    // the launch finishes in a fraction of one tile's serial time.  Round 4, from a sweep over 1 ... 64 images x workgroups per CU x
    // pieces (profiles/r4_small_launches.txt): the launch is fastest with ~2.3 pieces per WORKING workgroup and about 1.2 pieces per
    // resident slot in all (8-pixel pieces - a whole list walk for one row of pixels - only while even they number under 0.6 per
    // slot); the workgroups beyond that leave at once - a one-image launch runs on 512 of them, not on 4 096 that queue for the same
    // ticket counter.
    const unsigned int slots = a.slots;  // (the device's resident slots; the grid may be smaller: tile_grid)
    const unsigned int split_log = HOOK_SPLIT_LOG(deal_split_log(n_items_all, slots));
    if (blockIdx.x >= deal_working(n_items_all, split_log, slots)) return;  // (workgroup-uniform, before any barrier)
    // The heaviest class can be dealt out in 2^SPLIT0_LOG pieces of pixels (see SPLIT0_LOG; off since the lists are walked
    // near to far) - and is, like the others, when the launch has workgroups to spare.
    const unsigned int split0_log = SPLIT0_LOG > split_log ? SPLIT0_LOG : split_log;
    const float fS = (float)a.S;
    unsigned int xcc;  // the XCD this workgroup runs on: which partition it drains first
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= (unsigned int)(N_PARTS - 1);

    TIMERS_INIT
    for (unsigned int turn = 0; turn < N_PARTS; ++turn) {
    const unsigned int part = (xcc + turn) & (unsigned int)(N_PARTS - 1);
    const unsigned int nc0 = a.ctr->n_class[part][0], nc1 = a.ctr->n_class[part][1], nc2 = a.ctr->n_class[part][2], nc3 = a.ctr->n_class[part][3];
    const unsigned int n_items = nc0 + nc1 + nc2 + nc3;
    const unsigned int units0 = nc0 << split0_log;
    const unsigned int n_units = units0 + ((n_items - nc0) << split_log);
    const uint4 *const items = a.items + (size_t)part * 2u * a.item_cap;
    while (n_units > 0u) {
        unsigned int unit = 0;
        TSUB(0)
        if (lane == 0) unit = atomicAdd(&a.ctr->deal[part].next, 1u);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= n_units) break;
        TUNIT_START
        const bool heavy = unit < units0;
        const unsigned int sl = heavy ? split0_log : split_log, u_ = heavy ? unit : unit - units0;
        const unsigned int item = (u_ >> sl) + (heavy ? 0u : nc0);
        const int p_begin = (int)(u_ & ((1u << sl) - 1u)) * (WAVE >> sl), p_end = p_begin + (WAVE >> sl);
        // heaviest class first (the same lines in k_raster_tie_replay)
        const uint32_t item_at = item < nc0 ? item
                               : item < nc0 + nc1 ? a.item_cap - 1u - (item - nc0)
                               : item < nc0 + nc1 + nc2 ? a.item_cap + (item - nc0 - nc1)
                               : 2u * a.item_cap - 1u - (item - nc0 - nc1 - nc2);
        const uint4 it = items[item_at];
        const uint32_t code = it.x;
        const int n = (int)(code / (uint32_t)n_tiles), tile = (int)(code % (uint32_t)n_tiles);
        const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
        const int xo = tx * TILE + (lane & 7), yo = ty * TILE + (lane >> 3);
        const bool in_img = xo < a.S && yo < a.S;
        const float cx = tile_centre(tx, a.S), cy = tile_centre(ty, a.S);
        const float *vn = a.verts_ndc + (size_t)n * a.V * 3;
        const float *const xv_n = a.clip.xv + (size_t)n * CLIP_VX * 3;   // the image's clip tables (touched only by cut faces)
        const int *const xf_n = a.clip.xf + (size_t)n * CLIP_FX * 3;
        const size_t pix = ((size_t)n * a.S + yo) * a.S + xo;

        uint32_t kmin, kmax;  // bounds of the depth keys of this tile
        // the faces whose blurred box reaches this tile: binned by the setup kernel (any order), or found here through the tile
        // boxes of the 64-face groups (ascending id) when the image's lists did not fit
        const uint2 td = make_uint2(it.y, it.z);
        const bool binned = td.y != 0xFFFFFFFFu;  // (wave-uniform)
        TSUB(1)
        const uint2 *const list_src = binned ? a.lists + (size_t)n * a.list_cap + td.x : slist;
        int list_total;
        // A binned list of at most LIST_LDS_ROWS rows of 64 entries is read from memory ONCE: a tile that cannot truncate sends the ids
        // straight on to `slist2`; one that can leaves the entries in LDS (the record and histogram areas are free until pass 1), where
        // the sort's counting pass and its scatter pass find them.  Before, the bounds, the count and the scatter each read the list from
        // memory, four rows per dependent round trip.  Longer lists, and lists built here, go through memory as before.
        const bool list_lds = LIST_LDS_ROWS > 0 && binned && td.y <= (uint32_t)(LIST_LDS_ROWS * WAVE);  // (wave-uniform)
        uint2 *const llist = reinterpret_cast<uint2 *>(&lds);
        static_assert(LIST_LDS_ROWS * WAVE * sizeof(uint2) <= offsetof(DenseLds, pixt), "the list lives in the record and histogram areas");
        // the head of the ordered list (the faces of pass 1's first three chunks) also stays in LDS: `psel` is free until the first chunk
        // is staged, and pass 1's first vertex ids are then requested while the stores to `slist2` are still on their way
        uint32_t *const head = reinterpret_cast<uint32_t *>(lds.psel);
        static_assert(3 * DCHUNK * sizeof(uint32_t) <= sizeof(lds.psel), "the list's head lives in psel");
        if (list_lds) {
            list_total = (int)td.y;
            kmin = 0u;
            kmax = 0u;  // a tile that cannot truncate uses neither bound (nbits0, b1, shift1 and the depth clamp are the sort's and the select's)
            if (list_total > K) {
                uint32_t lo = 0x7F7FFFFFu, hi = 0u;
                for (int i0 = 0; i0 < list_total; i0 += 4 * WAVE) {
                    uint2 e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = at(list_src, (uint32_t)min(i0 + u * WAVE + lane, list_total - 1));
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        lo = min(lo, e[u].y); hi = max(hi, e[u].y);
                        if (i0 + u * WAVE + lane < list_total) llist[i0 + u * WAVE + lane] = e[u];
                    }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, WAVE));
                    hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, WAVE));
                }
                kmin = lo;
                kmax = __float_as_uint((__uint_as_float(hi) + __uint_as_float(it.w) * 1.000001f) * 1.0000005f) + 1u;  // (as below)
            } else {  // at most K faces: the order of the list is kept
                for (int i0 = 0; i0 < list_total; i0 += 4 * WAVE) {
                    uint2 e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = at(list_src, (uint32_t)min(i0 + u * WAVE + lane, list_total - 1));
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int pos = i0 + u * WAVE + lane;
                        if (pos < list_total) {
                            slist2[pos] = e[u].x;
                            if (pos < 3 * DCHUNK) head[pos] = e[u].x;
                        }
                    }
                }
            }
        } else if (binned) {
            // every depth of the tile lies between the nearest vertex of its nearest face and the farthest vertex of any: the entries
            // carry the nearest depth only (8 bytes), and farthest <= nearest + (largest depth extent of a face of the image, from
            // the setup kernel with the work item) bounds the other end - an upper bound is all the key range needs
            list_total = (int)td.y;
            uint32_t lo = 0x7F7FFFFFu, hi = 0u;
            for (int i0 = 0; i0 < list_total; i0 += 4 * WAVE) {
                uint2 e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) e[u] = at(list_src, (uint32_t)min(i0 + u * WAVE + lane, list_total - 1));
#pragma unroll
                for (int u = 0; u < 4; ++u) { lo = min(lo, e[u].y); hi = max(hi, e[u].y); }
            }
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, WAVE));
                hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, WAVE));
            }
            kmin = lo;
            // (rounded up twice: the extent was a rounded difference, the sum rounds again)
            kmax = __float_as_uint((__uint_as_float(hi) + __uint_as_float(it.w) * 1.000001f) * 1.0000005f) + 1u;
        } else {
            list_total = build_list(a, n, tx, ty, slist, lane, kmin, kmax);
        }
        const bool may_truncate = list_total > K;
        TSUB(2)
        // radix select on key = depth bits - kmin, which lies in [0, kmax - kmin]: `nbits0` significant bits, of which the
        // first digit takes the top SEL_BITS (so it always spreads over at least half of its buckets)
        const uint32_t krange = kmax - kmin;
        const int nbits0 = krange ? 32 - __clz(krange) : 0;
        const int b1 = min(SEL1_BITS, nbits0), shift1 = nbits0 - b1;
        // tiles that may truncate walk their faces near to far (see sort_list_near_to_far); the others keep the id order
        const uint32_t *const lst = slist2;
        // The staging loads of pass 1 form a chain list entry -> vertex indices -> vertex coordinates.  The first two links are
        // fetched ahead: while chunk k is evaluated the indices of chunk k + 1 and the list entries of chunk k + 2 are in
        // flight (four registers), so a chunk starts with one memory round trip instead of three.
        const int slot_ = lane & (DCHUNK - 1);
        auto list_at = [&](int c) { return (int)lst[min(c + slot_, list_total - 1)]; };
        int f_nx;            // list entry of chunk k + 2
        int ia, ib, ic;      // vertex ids of chunk k + 1 ...
        int ja, jb, jc;      // ... and of chunk k
        auto fetch_ids = [&](int f0, int f1) {
            ja = face_vertex(a.faces, xf_n, a.F, f0, 0); jb = face_vertex(a.faces, xf_n, a.F, f0, 1); jc = face_vertex(a.faces, xf_n, a.F, f0, 2);
            ia = face_vertex(a.faces, xf_n, a.F, f1, 0); ib = face_vertex(a.faces, xf_n, a.F, f1, 1); ic = face_vertex(a.faces, xf_n, a.F, f1, 2);
        };
        // what a (sub-)tile's pass 1 starts from, through the ordered list in memory
        auto first_ids = [&]() { f_nx = list_at(2 * DCHUNK); fetch_ids(list_at(0), list_at(DCHUNK)); };
        if (list_lds) {
            if (may_truncate) {
                // the same (row, lane) order of the LDS atomics as sort_list_near_to_far: the same faces at the same positions
                const int n_buckets = 1 << b1;
                auto digit_of = [&](const uint2 &e) { return (int)(((e.y - kmin) >> shift1) & (uint32_t)(n_buckets - 1)); };
                lds.start[lane] = 0;
                lds_fence();
                for (int i0 = 0; i0 < list_total; i0 += 4 * WAVE) {
                    uint2 e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = llist[min(i0 + u * WAVE + lane, list_total - 1)];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i0 + u * WAVE + lane < list_total) atomicAdd(&lds.start[digit_of(e[u])], 1);
                }
                lds_fence();
                const int c = lane < n_buckets ? lds.start[lane] : 0;
                const int incl = wave_scan_add(c);
                lds_fence();
                if (lane < n_buckets) lds.bstart[opaque_lane(lane)] = (uint16_t)min(incl - c, 65535);
                lds.start[lane] = incl - c;  // running cursor of every bucket
                lds_fence();
                for (int i0 = 0; i0 < list_total; i0 += 4 * WAVE) {
                    uint2 e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = llist[min(i0 + u * WAVE + lane, list_total - 1)];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i0 + u * WAVE + lane < list_total) {
                            const int pos = atomicAdd(&lds.start[digit_of(e[u])], 1);
                            slist2[pos] = e[u].x;
                            if (pos < 3 * DCHUNK) head[pos] = e[u].x;
                        }
                }
            }
            // (the barrier that makes `slist2` visible is the one in front of pass 1, ahead of every read of it)
            lds_fence();
            auto head_at = [&](int c) { return (int)head[min(c + slot_, list_total - 1)]; };
            f_nx = head_at(2 * DCHUNK);
            fetch_ids(head_at(0), head_at(DCHUNK));
        } else {
            __syncthreads();  // the list stores are visible to the loads below
            if (may_truncate) {
                sort_list_near_to_far(list_src, slist2, list_total, kmin, shift1, b1, lds, lane);
            } else {  // at most K faces: the order of the list is kept
                for (int i = lane; i < list_total; i += WAVE) slist2[i] = at(list_src, (uint32_t)i).x;
                __syncthreads();
            }
            first_ids();
        }
        TMARK(0)
        TSUB(3)
        HOOK_STOP_AFTER(0, continue)

        unsigned long long tie_acc = 0ull;  // (tie_rule 1) pixels of this unit left to k_raster_tie_replay
        // Sub-tiles: runs of `span` pixels (lane order).  Start from an estimate (a quarter of the pairs pixel x face
        // exist) and halve whenever pass 1 finds that the records do not fit; span * list_total <= REC_CAP always fits.
        int span = p_end - p_begin;
        while (span > 1 && (long long)span * list_total > 4ll * REC_CAP) span >>= 1;
        int p_lo = p_begin;
        // next sub-tile (false: none left): its first vertex ids are requested here, so that they are defined on every way to pass 1
        auto next_sub_tile = [&]() -> bool {
            p_lo += span;
            if (p_lo >= p_end) return false;
            first_ids();
            return true;
        };
        for (;;) {
            const bool mine = lane >= p_lo && lane < p_lo + span;  // this lane's pixel belongs to the sub-tile
            const int sy0 = p_lo >> 3, sy1 = (p_lo + span - 1) >> 3;                       // its rows ...
            const int sx0 = span >= 8 ? 0 : (p_lo & 7), sx1 = span >= 8 ? 7 : ((p_lo & 7) + span - 1);  // ... and columns
            // pixels outside the image or the sub-tile get a position no bbox can contain
            const float px = (in_img && mine) ? pix_to_ndc(a.S - 1 - xo, a.S) : 3.0e38f, py = pix_to_ndc(a.S - 1 - yo, a.S);
            lds.pixt[lane] = make_float2(px, py);
            if (may_truncate)
                for (int i_ = lane; i_ < (1 << SEL_BITS) / 2 * WAVE; i_ += WAVE) lds.hist[i_] = 0u;
            __syncthreads();

            // ---------------- pass 1: every pair inside a face's pixel box, once --------------------------------
            int vbase = 0;  // records written so far (wave-uniform)
            bool fits = true;
            // Pixels that cannot keep any further record ("closed"): they already hold K records in depth digits that are
            // final, i.e. below the digit of the first face not yet processed.  Lane = pixel keeps its count of final records.
            int final_digits = 0, final_cnt = 0;
            unsigned long long open_px = __ballot(in_img && mine);
            int ox0 = sx0, ox1 = sx1, oy0 = sy0, oy1 = sy1;  // bounding box of the open pixels
            int chunks_done = 0;
            // first record of every chunk (pass 3 walks the records group by group): lane c of `cst0` / `cst1` holds the start of chunk c /
            // 64 + c - a register read in pass 3 instead of a memory round trip per group; chunks from 128 on (lists beyond 4096 faces)
            // go through memory
            uint32_t cst0 = 0u, cst1 = 0u;
            auto set_chunk_start = [&](int c, uint32_t v) {  // (c, v wave-uniform)
                if (c < WAVE) cst0 = lane == c ? v : cst0;
                else if (c < 2 * WAVE) cst1 = lane == c - WAVE ? v : cst1;
                else if (lane == 0) scfirst[c] = v;
            };
            auto chunk_start = [&](int c) -> uint32_t {
                if (c < WAVE) return (uint32_t)__builtin_amdgcn_readlane((int)cst0, c);
                if (c < 2 * WAVE) return (uint32_t)__builtin_amdgcn_readlane((int)cst1, c - WAVE);
                return (uint32_t)__builtin_amdgcn_readfirstlane((int)scfirst[c]);
            };
            // (round 4: one more link ahead - the VERTICES of chunk k + 1 are requested before chunk k is evaluated and wait in nine
            // registers, so a chunk starts with the drain of the previous sweep's stores only, not with a vertex fetch behind it)
            Tri9 tv_nx;          // vertices of chunk k (requested one chunk ahead); its ids were requested before the barrier above
            tv_nx = load_tri(a, vn, xv_n, ja, jb, jc);
            for (int c0 = 0; c0 < list_total; c0 += DCHUNK) {
                if (may_truncate) {
                    const int lane_b = opaque_lane(lane);  // (the address of the lane's `bstart` entry is not kept across chunks)
                    // digit of this chunk's first face = number of buckets that start at or before it, minus one
                    const int d0 = __popcll(__ballot(lane < (1 << b1) && (int)lds.bstart[lane_b] <= c0)) - 1;
                    if (d0 > final_digits) {  // wave-uniform: digits [final_digits, d0) have just become final
                        for (int d = final_digits; d < d0; ++d)
                            final_cnt += (int)((lds.hist[(d >> 2) * WAVE + lane] >> (8 * (d & 3))) & 0xFFu);
                        final_digits = d0;
                        open_px &= ~__ballot(final_cnt >= K);
                        if (open_px == 0ull) break;  // every pixel of the (sub-)tile is closed: the remaining faces are all farther
                        unsigned int cols = 0u;
                        oy0 = 8; oy1 = -1;
                        for (int y = 0; y < TILE; ++y) {
                            const unsigned int row = (unsigned int)(open_px >> (8 * y)) & 0xFFu;
                            cols |= row;
                            if (row) { oy0 = min(oy0, y); oy1 = y; }
                        }
                        ox0 = (int)__builtin_ctz(cols); ox1 = 31 - (int)__builtin_clz(cols);
                    }
                }
                const int m = min(DCHUNK, list_total - c0);
                int cf, packed2, packed = 0;
                // (the lane index as the staging sees it is opaque to the compiler: what it derives from it - LDS addresses, the table
                // offsets - is recomputed per chunk, a few instructions, and not kept for the whole kernel in registers that then spill)
                int lane_c = lane;
                asm volatile("" : "+v"(lane_c));
                const int i0 = ja, i1 = jb, i2 = jc;
                const Tri9 tv = tv_nx;                       // this chunk's vertices (in flight since the chunk before)
                ja = ia; jb = ib; jc = ic;
                tv_nx = load_tri(a, vn, xv_n, ja, jb, jc);  // chunk c0 + DCHUNK
                ia = face_vertex(a.faces, xf_n, a.F, f_nx, 0); ib = face_vertex(a.faces, xf_n, a.F, f_nx, 1); ic = face_vertex(a.faces, xf_n, a.F, f_nx, 2);  // chunk c0 + 2 DCHUNK
                f_nx = list_at(c0 + 3 * DCHUNK);
                stage_faces(a, tv, i0, i1, i2, m, lds.rec, lane_c, cx, cy, fS, tx, ty, ox0, ox1, oy0, oy1, open_px, cf, packed2, sxy, sid, c0, a.list_stride);
                set_chunk_start(c0 / DCHUNK, (uint32_t)vbase);
                chunks_done = c0 / DCHUNK + 1;
                lds_fence();
                HOOK_STOP_AFTER(1, continue)
                const int incl = wave_scan_add(cf);
                const int off = incl - cf;          // first pair of this face in the chunk's pair list
                const int n_pairs = __builtin_amdgcn_readlane(incl, 63);
                packed |= off;                      // off <= DCHUNK * 32
                if (vbase + 2 * n_pairs > REC_CAP) { fits = false; break; }  // wave-uniform (n_pairs lanes of two pixels each)
                STAT(20, 2 * n_pairs)
                // pair -> face.  Every non-empty face sets the bit of its first pair in a 2048-bit map (64 words in LDS) and
                // leaves its packed box at its rank among the non-empty faces.  Lane i then keeps words 2i, 2i+1 - the start
                // bits of sweep step i - and the packed box of rank i; in step i a pair's face is (starts before the step) +
                // (start bits at or below its lane) - 1, two v_mbcnt and one ds_bpermute away.
                const unsigned long long nonempty = __ballot(cf > 0);
                STAT(31, __popcll(nonempty))  // staged faces that have any open pixel in their box
                lds.start[lane_c] = 0;
                lds_fence();
                if (cf > 0) {
                    atomicOr(reinterpret_cast<uint32_t *>(lds.start) + (off >> 5), 1u << (off & 31));
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(nonempty >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nonempty, 0u));
                    lds.psel[rank] = make_uint2((uint32_t)packed | ((uint32_t)lane << 13), (uint32_t)packed2);
                }
                lds_fence();
                const uint32_t fl_lo = reinterpret_cast<const uint32_t *>(lds.start)[(2 * lane) & 63];
                const uint32_t fl_hi = reinterpret_cast<const uint32_t *>(lds.start)[(2 * lane + 1) & 63];
                const uint2 pk_rank = lds.psel[lane & (DCHUNK - 1)];
                lds_fence();
                TSTAGE_MARK
                uint32_t carry = 0;                 // faces started before this step
                for (int q0 = 0; q0 < n_pairs; q0 += WAVE) {
                    const uint32_t wlo = (uint32_t)__builtin_amdgcn_readlane((int)fl_lo, q0 >> 6), whi = (uint32_t)__builtin_amdgcn_readlane((int)fl_hi, q0 >> 6);
                    const uint32_t below = __builtin_amdgcn_mbcnt_hi(whi, __builtin_amdgcn_mbcnt_lo(wlo, 0u));
                    const uint32_t own = ((wlo & lane_lo) | (whi & lane_hi)) ? 1u : 0u;
                    const int r = min((int)(carry + below + own) - 1, DCHUNK - 1);
                    carry += (uint32_t)(__popc(wlo) + __popc(whi));
                    const bool valid = q0 + lane < n_pairs;
                    const uint32_t pk = (uint32_t)__shfl((int)pk_rank.x, max(r, 0), WAVE), pk2 = (uint32_t)__shfl((int)pk_rank.y, max(r, 0), WAVE);
                    const int fs = (int)((pk >> 13) & (DCHUNK - 1));
                    const uint32_t rr = (uint32_t)(q0 + lane) - (pk & 0x1FFFu);
                    // rr < 32 and the reciprocal has 17 bits: a 24-bit multiply (full rate) is exact.  Spelled in assembly because
                    // hipcc widens __umul24 here to the quarter-rate v_mul_lo_u32 (it cannot see the range of rr)
                    uint32_t rr_inv;
                    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(rr_inv) : "v"(rr), "v"(pk2 & 0x1FFFFu));
                    const uint32_t dy = rr_inv >> 16;
                    const int pp = (int)((__umul24(dy, (pk2 >> 17) & 3u) + rr + (pk2 >> 20)) & 31u);  // pixel pair: pixels 2 pp, 2 pp + 1
                    const int p = 2 * pp;
                    const float4 pc = *reinterpret_cast<const float4 *>(&lds.pixt[p]);   // (px, py) of both pixels: one 16-byte read
                    const FaceRows fr = load_face_rows(lds.rec + fs * FSTR);
                    PairEval2 e;
                    eval_pair2(fr, pc.x - cx, pc.z - cx, pc.y - cy, a.blur, e);
                    HOOK_EXTRA_VALU(pc)
                    const uint32_t open2 = (uint32_t)(open_px >> p) & 3u;
                    const bool cand0 = valid && e.cand0 && (open2 & 1u), cand1 = valid && e.cand1 && (open2 & 2u);
                    const unsigned long long cm0 = __ballot(cand0), cm1 = __ballot(cand1);
                    if ((cm0 | cm1) == 0ull) continue;
                    // depth: kept inside the tile's vertex-depth range, where the convex combination lives up to rounding
                    // ... and never nearer than the face's nearest vertex (rounding of the convex combination), so that a record's
                    // digit is at least its face's: the closing rule above relies on it
                    uint32_t zb0 = 0x7F61B1E6u, zb1 = 0x7F61B1E6u;  // (3.0e38f: tiles that cannot truncate carry no depths)
                    if (may_truncate) {
                        const f32x2 z2 = pair_depth2(fr, e);
                        const float zf = fminf(fminf(fr.r2.y, fr.r2.z), fr.r2.w);
                        zb0 = min(max(__float_as_uint(vmax_raw(z2.x, zf)), kmin), kmax);
                        zb1 = min(max(__float_as_uint(vmax_raw(z2.y, zf)), kmin), kmax);
                    }
                    // a step's left-pixel records first, then its right-pixel records: each of the two store instructions writes ONE
                    // contiguous run of 12-byte records (interleaved - a lane's two records next to each other - both instructions
                    // touched every cache line of the step's run, each with half of the bytes: the record stores are 1.35 ms of the
                    // cfg2b launch, profiles/r6_experiments.md).  No sweep depends on the order of the records inside a chunk.
                    const uint32_t slot0 = (uint32_t)vbase + __builtin_amdgcn_mbcnt_hi((uint32_t)(cm0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cm0, 0u));
                    const uint32_t slot1 = (uint32_t)vbase + (uint32_t)__popcll(cm0) + __builtin_amdgcn_mbcnt_hi((uint32_t)(cm1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cm1, 0u));
                    const uint32_t meta = (uint32_t)p | ((uint32_t)(c0 + fs) << 6);
                    if (cand0) {
                        st_stream(srec, slot0, Rec3{zb0, meta | (e.inside0 ? 1u << 22 : 0u) | e.ebits0, __float_as_uint(e.sd.x)});
                        if (may_truncate) {  // first radix digit, and with it the number of candidates of the pixel
                            const uint32_t bucket = ((zb0 - kmin) >> shift1) & ((1u << b1) - 1u);
                            uint32_t *const hw = &lds.hist[(bucket >> 2) * WAVE + p];
                            const uint32_t sh = 8u * (bucket & 3u);
                            if (((*hw >> sh) & 0xFFu) < SAT8) atomicAdd(hw, 1u << sh);
                        }
                    }
                    if (cand1) {
                        st_stream(srec, slot1, Rec3{zb1, (meta + 1u) | (e.inside1 ? 1u << 22 : 0u) | e.ebits1, __float_as_uint(e.sd.y)});
                        if (may_truncate) {
                            const uint32_t bucket = ((zb1 - kmin) >> shift1) & ((1u << b1) - 1u);
                            uint32_t *const hw = &lds.hist[(bucket >> 2) * WAVE + p + 1];
                            const uint32_t sh = 8u * (bucket & 3u);
                            if (((*hw >> sh) & 0xFFu) < SAT8) atomicAdd(hw, 1u << sh);
                        }
                    }
                    vbase += __popcll(cm0) + __popcll(cm1);
                }
                TSWEEP_MARK
                lds_fence();  // rec is rewritten by the next chunk
            }
            if (!fits) {  // wave-uniform: try again with half the pixels
                span >>= 1;
                __syncthreads();
                first_ids();
                continue;
            }
            set_chunk_start(chunks_done, (uint32_t)vbase);  // (chunks behind an early exit hold no records)
            STAT(21, vbase) STAT(26, 1) STAT(27, list_total) STAT(28, chunks_done) STAT(29, (list_total + DCHUNK - 1) / DCHUNK) STAT(30, __popcll(open_px))
            __syncthreads();  // also: record stores of other lanes are visible from here on
            TMARK(1)
            HOOK_STOP_AFTER(1, { if (!next_sub_tile()) break; continue; }) HOOK_STOP_AFTER(2, { if (!next_sub_tile()) break; continue; })

            // ---------------- select + pass 2 ---------------------------------------------------------------------
            // K-th smallest depth of every pixel that has more than K candidates, and log2 of every kept blend factor summed
            // per pixel.  threshold: depth bits of the K-th smallest (0x7F800000 = +inf bits: keep everything); tie_cut: among
            // the faces exactly at the threshold those up to this list position are kept.
            uint32_t zt_bits = 0x7F800000u;
            int tie_cut = 0x7FFFFFFF;
            uint32_t pre = 0u;
            int need = 0, n_eq = 0, nbits = nbits0 - b1;
            bool trunc = false;
            bool defer = false;  // (tie_rule 1) this pixel's tie group at the K-th depth is cut by K: k_raster_tie_replay renders it
            if (may_truncate && vbase > 0) {
                need = K;
                const int tot = pick_digit8(lds.hist, lane, b1, pre, need, n_eq);
                trunc = tot > K;
                if (!trunc) need = 0;
            }
            const bool any_trunc = __ballot(trunc) != 0ull;
            // One sweep over all records.  A record of a pixel that is not truncated, or whose first digit is below the
            // pixel's chosen one, is kept for certain: its log goes to the pixel's sum.  One inside the chosen digit goes on
            // to the compact stream (with its log) and has its second digit counted; one above it is dropped.
            lds.plog[lane] = 0.0;
            lds.psel[lane] = make_uint2(pre, (uint32_t)need);
            const int b2 = min(SEL_BITS, nbits), shift2 = nbits - b2;
            if (any_trunc)
                for (int i_ = lane; i_ < (1 << SEL_BITS) / 2 * WAVE; i_ += WAVE) lds.hist[i_] = 0u;
            __syncthreads();
            TSUB(0)
            int n_cmp = 0;
            float rmax2 = 0.f;  // largest |closest point - pixel|^2 over the records: bounds the gradient sums of pass 3
            if (vbase > 0) {
                struct Rec { uint32_t z, mt; float sd; };
                auto load_recs = [&](Rec (&r)[DGROUP], int g0) {
#pragma unroll
                    for (int u = 0; u < DGROUP; ++u) {
                        const uint32_t idx = (uint32_t)min(g0 + u * WAVE + lane, vbase - 1);
                        const Rec3 q = ld_stream(srec, idx);
                        r[u].z = q.a; r[u].mt = q.b; r[u].sd = __uint_as_float(q.c);
                    }
                };
                auto blend_rows = [&](auto rows, const Rec (&r)[DGROUP], int g0) {  // (rows.has: sweep_rows)
                    uint2 ps[DGROUP];
#pragma unroll
                    for (int u = 0; u < DGROUP; ++u)
                        if (rows.has(u)) ps[u] = lds.psel[r[u].mt & 63u];
#pragma unroll
                    for (int u = 0; u < DGROUP; ++u) {
                        if (!rows.has(u)) continue;
                        STAT(59, 1)
                        const bool valid = g0 + u * WAVE + lane < vbase;
                        const uint32_t key = r[u].z - kmin, d1 = key >> nbits;
                        const bool sure = valid & ((ps[u].y == 0u) | (d1 < ps[u].x));
                        const bool maybe = valid & (ps[u].y > 0u) & (d1 == ps[u].x);
                        rmax2 = fmaxf(rmax2, fabsf(r[u].sd));  // (the clamped tail of the last row repeats a record: harmless)
                        const float lf = __log2f(1.0f - face_prob(r[u].sd, a.inv_sigma_log2e));
                        if (sure & (lf != 0.f)) atomicAdd(&lds.plog[r[u].mt & 63u], (double)lf);
                        STAT(45, __popcll(__ballot(sure))) STAT(46, __popcll(__ballot(valid & !sure & !maybe)))
                        if (any_trunc) {  // wave-uniform
                            const unsigned long long km = __ballot(maybe);
                            const uint32_t slot = (uint32_t)n_cmp + __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
                            if (maybe) {
                                at(crec, slot) = Rec3{key, r[u].mt, __float_as_uint(lf)};
                                const uint32_t bucket = (key >> shift2) & ((1u << b2) - 1u);
                                atomicAdd(&lds.hist[(bucket >> 1) * WAVE + (r[u].mt & 63u)], (bucket & 1u) ? 0x10000u : 1u);
                            }
                            n_cmp += __popcll(km);
                        }
                    }
                };
                Rec ra[DGROUP], rb[DGROUP];
                load_recs(ra, 0);
                STAT(56, rows_upto(0, vbase)) STAT(57, (vbase + 2 * DGROUP * WAVE - 1) / (2 * DGROUP * WAVE) * (2 * DGROUP))  // rows needed; rows of whole turns
                sweep_rows<DGROUP>(0, vbase, ra, rb, load_recs, blend_rows);
            }
            __syncthreads();
            TSUB(4)
            if (any_trunc) {
                if (nbits > 0) {  // second digit: counted above
                    pick_digit(lds.hist, lane, b2, pre, need, n_eq);
                    nbits -= b2;
                    __syncthreads();
                }
                // refinement through memory while the compact stream is long (it shrinks about six-fold per sweep) ...
                while (nbits > 0 && __ballot(need > 0) != 0ull && n_cmp > SELR * WAVE) {
                    const int b = min(SEL_BITS, nbits);
                    n_cmp = refine_sweep(lds, crec, n_cmp, nbits, b, lane, pre, need);
                    pick_digit(lds.hist, lane, b, pre, need, n_eq);
                    nbits -= b;
                    __syncthreads();
                }
                if (n_cmp <= SELR * WAVE) {
                // ... then IN REGISTERS (round 4): a lane takes up to SELR of the remaining records and every further step - the digits
                // still to go, the cut of a tie group by face id, the sum of the logs that made it - runs on them with the per-pixel
                // histograms in LDS and no memory traffic at all.  Through memory each of those three to seven sweeps over a few
                // hundred records was two exposed round trips (the first load, the drain of the in-place stores): the selection was
                // 9.5 % of the launch for 23 % of the records.
                constexpr uint32_t INV = 0xFFFFFFFFu;  // record that has left the selection (keys are below 2^31)
                uint32_t rk[SELR], rm[SELR];
                float rl[SELR];
#pragma unroll
                for (int r_ = 0; r_ < SELR; ++r_) {
                    const int idx = r_ * WAVE + lane;
                    const Rec3 q = at(crec, (uint32_t)min(idx, max(n_cmp - 1, 0)));
                    rk[r_] = idx < n_cmp ? q.a : INV; rm[r_] = q.b; rl[r_] = __uint_as_float(q.c);
                }
                while (nbits > 0 && __ballot(need > 0) != 0ull) {
                    const int b = min(SEL_BITS, nbits), shift = nbits - b;
                    lds.psel[lane] = make_uint2(pre, (uint32_t)need);
                    for (int i_ = lane; i_ < (1 << SEL_BITS) / 2 * WAVE; i_ += WAVE) lds.hist[i_] = 0u;
                    lds_fence();
                    uint2 ps[SELR];
#pragma unroll
                    for (int r_ = 0; r_ < SELR; ++r_) ps[r_] = lds.psel[rm[r_] & 63u];
#pragma unroll
                    for (int r_ = 0; r_ < SELR; ++r_) {
                        const uint32_t pxl = rm[r_] & 63u;
                        const bool live = (rk[r_] != INV) & (ps[r_].y > 0u);
                        const uint32_t top = rk[r_] >> nbits;
                        const bool sure = live & (top < ps[r_].x), stay = live & (top == ps[r_].x);
                        if (sure & (rl[r_] != 0.f)) atomicAdd(&lds.plog[pxl], (double)rl[r_]);
                        if (stay) {
                            const uint32_t bucket = (rk[r_] >> shift) & ((1u << b) - 1u);
                            atomicAdd(&lds.hist[(bucket >> 1) * WAVE + pxl], (bucket & 1u) ? 0x10000u : 1u);
                        }
                        rk[r_] = (live & !stay) ? INV : rk[r_];  // decided either way: it leaves
                    }
                    lds_fence();
                    pick_digit(lds.hist, lane, b, pre, need, n_eq);
                    nbits -= b;
                    lds_fence();
                }
                if (trunc) zt_bits = pre + kmin;
                // `need` of the n_eq faces at the threshold are kept: the ones with the smallest face ids - or, under tie_rule 1, the
                // ones the reference's queue would keep (k_raster_tie_replay).  Which `need` of them they are matters only if the tied
                // records differ: a pixel outside two faces that meet in an edge (or a fan that meets in a vertex) - the usual tie -
                // has the same closest point, depth, distance and end points on all of them, so every choice gives the same
                // silhouette value and the same vertex gradient.  Such a pixel is cut by face id here (a fifth of the cut tie groups: 237 000 ->
                // 184 000 replayed pixels per cfg2b launch); only tie groups whose records differ in distance or side go on - mostly fans
                // around a vertex, whose faces clip the pixel's barycentrics to that vertex (one depth) but are at different distances.
                bool same = false;
                if (HOOK_TIE_EQUIV && a.tie_rule && __ballot(trunc && need < n_eq) != 0ull) {  // (wave-uniform)
                    lds.psel[lane] = make_uint2((trunc && need < n_eq) ? pre : INV, 0u);
                    lds.hist[lane] = 0xFFFFFFFFu; lds.hist[WAVE + lane] = 0u;         // min / max of the tied records' log bits
                    lds.hist[2 * WAVE + lane] = 1u; lds.hist[3 * WAVE + lane] = 0u;   // and / or of their inside flags
                    lds_fence();
#pragma unroll
                    for (int r_ = 0; r_ < SELR; ++r_) {
                        const uint32_t pxl = rm[r_] & 63u;
                        if (rk[r_] != INV && rk[r_] == lds.psel[pxl].x) {
                            const uint32_t lb = __float_as_uint(rl[r_]), ins = (rm[r_] >> 22) & 1u;
                            atomicMin(&lds.hist[pxl], lb); atomicMax(&lds.hist[WAVE + pxl], lb);
                            atomicAnd(&lds.hist[2 * WAVE + pxl], ins); atomicOr(&lds.hist[3 * WAVE + pxl], ins);
                        }
                    }
                    lds_fence();
                    same = lds.hist[lane] == lds.hist[WAVE + lane] && lds.hist[2 * WAVE + lane] == lds.hist[3 * WAVE + lane];
                    lds_fence();
                }
                const bool split = trunc && need < n_eq && (!a.tie_rule || same);
                defer = trunc && need < n_eq && a.tie_rule && !same;
                uint32_t rf[SELR];  // face ids of the records at the threshold of a split pixel (fetched only in tiles that have one)
#pragma unroll
                for (int r_ = 0; r_ < SELR; ++r_) rf[r_] = INV;
                if (__ballot(split) != 0ull) {
                    lds.psel[lane] = make_uint2(split ? pre : INV, 0u);
                    lds_fence();
#pragma unroll
                    for (int r_ = 0; r_ < SELR; ++r_)
                        if (rk[r_] != INV && rk[r_] == lds.psel[rm[r_] & 63u].x) rf[r_] = lst[(rm[r_] >> 6) & 0xFFFFu];
                    int pbits = 32 - __clz(max(a.FT - 1, 1));
                    uint32_t ppre = 0u;
                    int pneed = split ? need : 0, peq = 0;
                    lds_fence();
                    while (pbits > 0 && __ballot(pneed > 0) != 0ull) {
                        const int b = min(SEL_BITS, pbits), shift = pbits - b;
                        lds.psel[lane] = make_uint2(ppre, (uint32_t)pneed);
                        for (int i_ = lane; i_ < (1 << SEL_BITS) / 2 * WAVE; i_ += WAVE) lds.hist[i_] = 0u;
                        lds_fence();
#pragma unroll
                        for (int r_ = 0; r_ < SELR; ++r_) {
                            const uint32_t pxl = rm[r_] & 63u;
                            const uint2 ps = lds.psel[pxl];
                            const bool hit = (rf[r_] != INV) & (ps.y > 0u) & ((rf[r_] >> pbits) == ps.x);
                            const uint32_t bucket = (rf[r_] >> shift) & ((1u << b) - 1u);
                            if (hit) atomicAdd(&lds.hist[(bucket >> 1) * WAVE + pxl], (bucket & 1u) ? 0x10000u : 1u);
                        }
                        lds_fence();
                        pick_digit(lds.hist, lane, b, ppre, pneed, peq);
                        pbits -= b;
                        lds_fence();
                    }
                    if (split) tie_cut = (int)ppre;
                }
                // the records still held that made it: depth below the threshold, or at it up to the tie cut
                lds.psel[lane] = make_uint2(trunc ? pre : 0u, (uint32_t)tie_cut);
                lds_fence();
#pragma unroll
                for (int r_ = 0; r_ < SELR; ++r_) {
                    const uint32_t pxl = rm[r_] & 63u;
                    const uint2 ps = lds.psel[pxl];
                    const bool keep = (rk[r_] != INV) & ((rk[r_] < ps.x) | ((rk[r_] == ps.x) & (((int)ps.y == 0x7FFFFFFF) | ((int)rf[r_] <= (int)ps.y))));
                    if (keep & (rl[r_] != 0.f)) atomicAdd(&lds.plog[pxl], (double)rl[r_]);
                }
                lds_fence();
                } else {
                // (the compact stream never got short - thousands of records tied in their first digits: everything through memory)
                while (nbits > 0 && __ballot(need > 0) != 0ull) {
                    const int b = min(SEL_BITS, nbits);
                    n_cmp = refine_sweep(lds, crec, n_cmp, nbits, b, lane, pre, need);
                    pick_digit(lds.hist, lane, b, pre, need, n_eq);
                    nbits -= b;
                    __syncthreads();
                }
                if (trunc) zt_bits = pre + kmin;
                // `need` of the n_eq faces at the threshold are kept: the first ones in list order
                const bool split = trunc && need < n_eq && !a.tie_rule;
                defer = trunc && need < n_eq && a.tie_rule;
                if (__ballot(split) != 0ull) {
                    // select on the list position among the records whose depth equals the pixel's threshold
                    lds.pgrad[lane] = make_float4(0.f, __uint_as_float(split ? pre : 0xFFFFFFFFu), 0.f, 0.f);
                    __syncthreads();
                    int pbits = 32 - __clz(max(a.FT - 1, 1));  // the tie key is the face id (the list is in near-to-far order)
                    uint32_t ppre = 0u;
                    int pneed = split ? need : 0, peq = 0;
                    auto pos_key = [&](uint32_t idx, uint32_t mt) {
                        // records of other depths get the key 0xFFFFFFFF, which select_sweep ignores
                        return at(crec, idx).a == __float_as_uint(lds.pgrad[mt & 63u].y) ? lst[(mt >> 6) & 0xFFFFu] : 0xFFFFFFFFu;
                    };
                    while (pbits > 0 && __ballot(pneed > 0) != 0ull) {
                        const int b = min(SEL_BITS, pbits);
                        select_sweep(lds, crec, n_cmp, pbits, b, lane, ppre, pneed, pos_key);
                        pick_digit(lds.hist, lane, b, ppre, pneed, peq);
                        pbits -= b;
                        __syncthreads();
                    }
                    if (split) tie_cut = (int)ppre;
                }
                // the compact records still in the stream (those of the last bucket examined) that made it: depth below the
                // threshold, or at it up to the tie cut
                lds.pgrad[lane] = make_float4(0.f, __uint_as_float(trunc ? pre : 0u), __int_as_float(tie_cut), 0.f);
                const bool any_split_sel = __ballot(tie_cut != 0x7FFFFFFF) != 0ull;
                __syncthreads();
                for (int g0 = 0; g0 < n_cmp; g0 += DGROUP * WAVE) {
                    uint32_t kk[DGROUP], mt[DGROUP];
                    float lf[DGROUP];
#pragma unroll
                    for (int u = 0; u < DGROUP; ++u) {
                        const uint32_t idx = (uint32_t)min(g0 + u * WAVE + lane, n_cmp - 1);
                        const Rec3 q = at(crec, idx);
                        kk[u] = q.a; mt[u] = q.b; lf[u] = __uint_as_float(q.c);
                    }
#pragma unroll
                    for (int u = 0; u < DGROUP; ++u) {
                        const float4 pg = lds.pgrad[mt[u] & 63u];
                        const uint32_t zt_ = __float_as_uint(pg.y);
                        // a record AT the threshold depth of a pixel whose tie group straddles K is kept up to the cut in face id
                        // (rare: the id is fetched only then)
                        const bool in_range = g0 + u * WAVE + lane < n_cmp;
                        bool tie_ok = true;
                        if (any_split_sel) {  // wave-uniform
                            const int cut = __float_as_int(pg.z);
                            int fid = 0;
                            if (in_range & (kk[u] == zt_) & (cut != 0x7FFFFFFF)) fid = (int)lst[(mt[u] >> 6) & 0xFFFFu];
                            tie_ok = fid <= cut;
                        }
                        const bool keep = in_range & ((kk[u] < zt_) | ((kk[u] == zt_) & tie_ok));
                        if (keep & (lf[u] != 0.f)) atomicAdd(&lds.plog[mt[u] & 63u], (double)lf[u]);
                    }
                }
                __syncthreads();
                }
            }
            TMARK(2)
            TSUB(5)
            HOOK_STOP_AFTER(3, { if (!next_sub_tile()) break; continue; })
            STAT(22, n_cmp) STAT(23, __popcll(__ballot(trunc))) STAT(24, __popcll(__ballot(lds.plog[lane] != 0.0)))
            STAT(40, any_trunc ? 1 : 0) STAT(41, may_truncate ? 1 : 0) STAT(42, any_trunc ? vbase : 0) STAT(43, may_truncate ? vbase : 0) STAT(44, __popcll(__ballot(tie_cut != 0x7FFFFFFF)))
            const double plog_px = lds.plog[lane];
            const float alpha = exp2f((float)plog_px);
            TMARK(3)

            // ---------------- epilogue: silhouette value, loss, upstream gradient --------------------
            const float silv = 1.0f - alpha;
            const bool own = in_img && mine && !defer;
            tie_acc |= __ballot(in_img && mine && defer);
            float g = 0.f;
            if (MODE == MODE_FWD) {
                if (own) a.sil[pix] = silv;
            } else if (MODE == MODE_BWD) {
                if (own) g = a.grad_sil[pix];
            } else {
                float lsum = 0.f;
                if (own) {
                    const float tg = a.target_u8 ? (float)a.target_u8[pix] : a.target[pix];
                    const float diff = silv - tg;
                    lsum = fabsf(diff) - fabsf(tg);  // loss_img starts at sum |0 - target|
                    g = a.pix_scale[n] * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));
                    if (a.sil) a.sil[pix] = silv;
                }
                lsum = wave_sum(lsum);
                if (lane == 0 && lsum != 0.f) atomicAdd(&a.loss_acc[n], (unsigned long long)(long long)rint((double)lsum * 4294967296.0));
            }

            // ---------------- pass 3: lane = record -------------------------------------------------
            // d sil / d dist_k = -alpha p_k / sigma   (alpha = prod_j (1 - p_j); exact also when 1 - p_k == 0)
            const float coef = -g * alpha * a.inv_sigma;
            // (a pixel whose records all have 1 - p == 1 in fp32 - or that has none - hands nothing back: its coefficient must not enter
            // the fixed-point bound below either, or a tile of empty pixels sets the resolution for its one contributing pixel)
            const bool active = own && (g != 0.f) && (alpha > ALPHA_GRAD_EPS) && (plog_px != 0.0);
            const bool any_split = __ballot(tie_cut != 0x7FFFFFFF) != 0ull;  // a pixel whose tie group at the K-th depth is cut by face id
            TSUB(6)
            STAT(25, __popcll(__ballot(active)))
            if (MODE != MODE_FWD && __ballot(active) != 0ull) {
                float *dn = a.d_ndc + (size_t)n * a.V * 2;
                // Fixed point for the LDS accumulators.  One accumulator component receives at most one record per pixel,
                // each of magnitude <= 2 |r| |coef_pixel| p_k max(t, 1 - t) <= 2 r_max |coef_pixel|, so no partial sum
                // exceeds bound = 2 r_max sum |coef_pixel|.  With scale = the power of two that maps `bound` into [2^29, 2^30)
                // every rounded contribution sum stays below 2^31 (plus at most 64 half-units of rounding), the scaling is
                // exact, and the resolution is bound / 2^30: ~1e-9 of the tile's largest possible gradient sum, below the
                // fp32 rounding of the global atomics the sums end in.  Integer sums are order independent.
                const float csum = wave_sum(active ? fabsf(coef) : 0.f);
                const float bound = 2.0f * sqrtf(wave_max(rmax2)) * csum;
                // Packed launches accumulate in the IMAGE's fixed-point scale right away (image_fx_scale: no vertex component of the
                // image can overflow it, so no partial sum can): every contribution is rounded once, per record, and from there on
                // all sums - LDS, flush, memory-side atomics - are integer adds, exact in any order and any grouping of faces.
                // (an image with cut faces stays on float atomics, see k_raster_setup)
                const bool img_fixed = MODE == MODE_FUSED && a.packed && a.clip.xcount[n] == 0u;  // (wave-uniform)
                const float fx_scale = img_fixed ? image_fx_scale(a.img_bound[n], a.pix_scale[n], a.inv_sigma)
                                       : (bound > 0.f && bound < 3.0e38f) ? exp2f(fminf(29.0f - floorf(log2f(bound)), 100.0f)) : 0.f;
                const float fx_inv = fx_scale > 0.f ? 1.0f / fx_scale : 0.f;
                lds.pgrad[lane] = make_float4(active ? coef * fx_scale : 0.f, __uint_as_float(zt_bits), __int_as_float(tie_cut), 0.f);
                __syncthreads();
                constexpr int GR = GCHUNK / DCHUNK;
                static_assert(GCHUNK == WAVE, "pass 3: lane = face of the group");
                const uint32_t copy_off = (uint32_t)(lane & (GCOPIES - 1)) * (GCHUNK * 3);
                float *const xg_n = a.clip.xg + (size_t)n * CLIP_VX * 2;  // gradient rows of the image's new vertices (cut faces)
                // the group's projected vertices, from which a record's edge parameter t is recomputed (4 bytes less written and
                // read per record than storing it); the table lives where the selection histograms were
                float2 *const fv = reinterpret_cast<float2 *>(lds.hist);  // [GCHUNK][3]
                static_assert(GCHUNK * 3 * sizeof(float2) <= sizeof(lds.hist), "the vertex table of a group lives in the histogram area");
                TP3_START
                for (int ch = 0; ch < chunks_done; ch += GR) {
                    const int i_beg = (int)chunk_start(ch), i_end = (int)chunk_start(min(ch + GR, chunks_done));  // (registers: no memory round trip)
                    if (i_beg == i_end) continue;
                    TP3(0)
                    // lane = face of the group: its projected vertices and vertex ids as pass 1 left them in the tile's table (one round
                    // trip, requested together with the first records; the list -> face -> vertex chain they replace was three)
                    const int fch = ch * DCHUNK + lane;
                    const bool staged = fch < chunks_done * DCHUNK && fch < list_total;
                    const uint32_t fcl = (uint32_t)min(fch, list_total - 1);
                    const float2 tv0 = at(sxy, fcl), tv1 = at(sxy, (uint32_t)a.list_stride + fcl), tv2 = at(sxy, 2u * (uint32_t)a.list_stride + fcl);
                    const TriIds tid = at(sid, fcl);
                    struct GRec { uint32_t z, mt; float sd; };
                    auto load_recs = [&](GRec (&r)[DGROUP], int g0) {
#pragma unroll
                        for (int u = 0; u < DGROUP; ++u) {
                            const uint32_t idx = (uint32_t)min(g0 + u * WAVE + lane, i_end - 1);  // clamped: the tail repeats the last record
                            const Rec3 q = ld_stream(srec, idx);
                            r[u].z = q.a; r[u].mt = q.b; r[u].sd = __uint_as_float(q.c);
                        }
                    };
                    GRec ra[DGROUP], rb[DGROUP];
                    load_recs(ra, i_beg);
                    const int lane_g = opaque_lane(lane);  // (the row's LDS address is recomputed per group, not reloaded from scratch)
                    fv[lane_g * 3 + 0] = tv0;
                    fv[lane_g * 3 + 1] = tv1;
                    fv[lane_g * 3 + 2] = tv2;
                    TP3(1)
                    for (int i_ = lane; i_ < GCOPIES * GCHUNK * 3; i_ += WAVE) (&lds.gacc[0][0])[i_] = 0ull;
                    lds_fence();
                    TP3(2)
                    // One row of records per lane and step, DGROUP rows per buffer.  Straight-line code: every lane computes its record's
                    // contribution whether it is kept or not and only the two accumulator adds are predicated, so that the LDS gathers of
                    // all rows of a buffer are in flight together (a branch per record kept each row's gathers behind the previous row's
                    // conflicting atomics: one exposed LDS round trip per row).
                    // The buffer that meets the group's end is processed for the rows that hold a record of the group only (sweep_rows,
                    // rows.has), and a buffer behind the end is neither loaded nor processed: a group of 10 rows ran 16 before, with every
                    // gather and every instruction of the body.
                    auto grad_rows = [&](auto rows, const GRec (&r)[DGROUP], int g0) {
                        float4 pg[DGROUP];
                        float2 pa[DGROUP], pb[DGROUP], pc[DGROUP];
                        uint32_t oa[DGROUP], ob[DGROUP];
#pragma unroll
                        for (int u = 0; u < DGROUP; ++u) {
                            if (!rows.has(u)) continue;
                            const uint32_t mt = r[u].mt;
                            const uint32_t f3 = ((mt >> 6) & (uint32_t)(GCHUNK - 1)) * 3u;  // (list position % GCHUNK) * 3
                            const uint32_t edge = mt >> 23;
                            oa[u] = f3 + (edge == 2u ? 1u : 0u); ob[u] = f3 + (edge == 0u ? 1u : 2u);  // end points of the closest edge
                            pg[u] = lds.pgrad[mt & 63u];
                            pa[u] = fv[oa[u]]; pb[u] = fv[ob[u]]; pc[u] = lds.pixt[mt & 63u];
                        }
#pragma unroll
                        for (int u = 0; u < DGROUP; ++u) {
                            if (!rows.has(u)) continue;
                            STAT(63, 1)
                            const bool valid = g0 + u * WAVE + lane < i_end;
                            const uint32_t mt = r[u].mt;
                            const uint32_t zt_ = __float_as_uint(pg[u].y);
                            const bool inside = ((mt >> 22) & 1u) != 0u;
                            float gd = pg[u].x * face_prob(r[u].sd, a.inv_sigma_log2e);                 // scale * d L / d (signed dist)
                            gd = inside ? -gd : gd;                                               // ... / d (unsigned squared distance)
                            bool tie_ok = true;  // (as in the blend: only a record at the threshold of a split tie group needs its face id)
                            if (any_split) {  // wave-uniform and rare: the fetch and the wait for it stay out of the common path
                                const int cut = __float_as_int(pg[u].z);
                                int fid = 0;
                                if (valid & (r[u].z == zt_) & (cut != 0x7FFFFFFF)) fid = (int)lst[(mt >> 6) & 0xFFFFu];
                                tie_ok = fid <= cut;
                            }
                            const bool keep = valid & (gd != 0.f) & ((r[u].z < zt_) | ((r[u].z == zt_) & tie_ok));
                            // closest point of that edge: clamped projection of the pixel, as eval_pair computed it (t = 0 for a
                            // degenerate edge); r = closest point - pixel
                            const EdgeGrad eg = edge_gradient(pa[u], pb[u], pc[u], gd);
                            const unsigned long long ga = pack_fx2(eg.ax, eg.ay), gb = pack_fx2(eg.bx, eg.by);
                            if (keep) {
                                unsigned long long *acc = &lds.gacc[0][0] + copy_off;
                                atomicAdd(acc + oa[u], ga);
                                atomicAdd(acc + ob[u], gb);
                            }
                        }
                    };
                    STAT(60, 1) STAT(61, rows_upto(i_beg, i_end)) STAT(62, (i_end - i_beg + 2 * DGROUP * WAVE - 1) / (2 * DGROUP * WAVE) * (2 * DGROUP))  // groups; rows needed; rows of whole turns
                    sweep_rows<DGROUP>(i_beg, i_end, ra, rb, load_recs, grad_rows);
                    TP3(3)
                    lds_fence();
                    TP3(4)
                    if (staged) {  // flush: sum the copies, unpack, one global atomic per touched vertex component
                        const int vi[3] = {tid.a, tid.b, tid.c};
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            unsigned long long tot = 0ull;
#pragma unroll
                            for (int c = 0; c < GCOPIES; ++c) tot += lds.gacc[c][lane * 3 + k];
                            if (img_fixed) {  // wave-uniform: the sum is already in the image's scale
                                if (tot != 0ull) atomicAdd(reinterpret_cast<unsigned long long *>(dn) + vi[k], tot);
                                continue;
                            }
                            const int qy = (int)(uint32_t)tot;
                            const int qx = (int)(uint32_t)((tot - (unsigned long long)(long long)qy) >> 32);
                            float *const row = vi[k] < a.V ? dn + 2 * vi[k] : xg_n + 2 * (vi[k] - a.V);  // (a vertex of a cut face's front part: its own table)
                            if (qx != 0) atomicAdd(row, (float)qx * fx_inv);
                            if (qy != 0) atomicAdd(row + 1, (float)qy * fx_inv);
                        }
                    }
                    lds_fence();  // the accumulators are read before the next group clears them; unlike __syncthreads() this does
                                  // not wait for the flush's global atomics to be acknowledged (a microsecond per group)
                    TP3(5)
                }
            }
            __syncthreads();
            TMARK(4)
            TSUB(7)
            if (!next_sub_tile()) break;
        }
        if (tie_acc != 0ull && lane == 0) {
            atomicOr(&a.tie_mask[(size_t)part * 2u * a.item_cap + item_at], tie_acc);  // (pieces of one tile add their bits)
            atomicAdd(&a.ctr->tie_pixels, (unsigned int)__popcll(tie_acc));
        }
        TUNIT_END
    }
    }  // next partition
    TIMERS_FLUSH
}
