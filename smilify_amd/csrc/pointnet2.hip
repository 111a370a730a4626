// The PointNet++ set-abstraction operations of the point-cloud regressor, for gfx950: farthest point sampling, ball query and grouping.
//
// Replaces (reference): fitter_3d/pointcloud2smil/pointnet2_utils.py farthest_point_sample (:69-90, a Python loop of npoint
// iterations), query_ball_point (:93-113, a sort of a (B, S, N) int64 tensor) and the index_points + cat + permute that feed Conv2d in
// sample_and_group (:131-138) and PointNetSetAbstractionMsg.forward (:249-258).
//
//  * k_fps             one workgroup per cloud.  A thread keeps PPT points and their running distances in registers for the whole call
//                      (point j T + tid in slot j).  Per iteration: the distance update and a per-thread argmax that carries the
//                      point's coordinates along, a wave maximum of the 64-bit key {distance bits, 0xFFFFFFFF - index} (distances are
//                      >= 0: the bits order like the values; the smallest index wins a tie) in DPP steps, and ONE hop through LDS
//                      across the waves: every wave's winner writes {key, x, y, z}, one barrier, every wave reads the <= 16 entries and
//                      reduces them itself.  The entries are double-buffered by the iteration's parity, so ONE barrier per iteration
//                      is enough (iteration i + 2 writes the buffer of iteration i only behind barrier i + 1, which no wave passes
//                      before it has read buffer i).  A cloud of <= 512 points runs in one wave: no LDS, no barrier.
//                      d = (dx dx + dy dy) + dz dz with every operation rounded on its own (contraction off): FPS is chaotic, one
//                      flipped argmax changes every later index.
//  * k_ball_query      one wave per query, 64 candidates per step straight from L2 (the next step's are loaded before this step's
//                      are judged), a ballot per radius, slots from the ballot's prefix population count, a wave-uniform exit once
//                      every radius is full; up to four radii fill their index arrays from the one pass.
//  * k_group_points    the (B, C, K, S) tensor Conv2d reads, through a 64 x 64 LDS tile: feature rows are read along the channels and
//                      stored along the positions, both coalesced.  An index outside [0, N) gives a zero row.
//  * k_group_max / _add / _out   the gradient of the grouped features back to (B, N, D): duplicates of an index (padding makes them
//                      the common case) are summed as int64 fixed point (common.h, "order-independent scatter sums"; magnitude:
//                      the cloud's largest |gradient|, addends: K S).  The tile is the forward's, walked the other way.
#include <algorithm>
#include <cmath>

#include "common.h"

// ---- farthest point sampling ----------------------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long k) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), CTRL, 0xF, 0xF, true);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > k ? o : k;
}

// Maximum over each row of 16 lanes; valid in every lane of the row.
__device__ __forceinline__ unsigned long long row_max_u64(unsigned long long k) {
    k = dpp_max_u64<0xB1>(k);   // quad_perm [1,0,3,2]
    k = dpp_max_u64<0x4E>(k);   // quad_perm [2,3,0,1]
    k = dpp_max_u64<0x141>(k);  // row_half_mirror
    k = dpp_max_u64<0x140>(k);  // row_mirror
    return k;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
    k = row_max_u64(k);
    const unsigned long long r0 = read_lane(k, 0), r1 = read_lane(k, 16), r2 = read_lane(k, 32), r3 = read_lane(k, 48);
    const unsigned long long a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
    return a > b ? a : b;
}

template <int PPT, bool ONE_WAVE>
__global__ void __launch_bounds__(ONE_WAVE ? 64 : 1024) k_fps(const float *xyz, const int *start, int N, int npoint, int *out) {
#pragma clang fp contract(off)  // (dx dx + dy dy) + dz dz, every operation rounded on its own
    __shared__ unsigned long long s_key[2][16];
    __shared__ float s_c[2][16][3];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
    const float *p = xyz + (size_t)b * N * 3;
    float px[PPT], py[PPT], pz[PPT], dist[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int i = j * T + tid;
        const bool ok = i < N;  // a slot behind the cloud: distance 0 for good and an index that loses every tie
        px[j] = ok ? p[3 * (size_t)i] : 0.f;
        py[j] = ok ? p[3 * (size_t)i + 1] : 0.f;
        pz[j] = ok ? p[3 * (size_t)i + 2] : 0.f;
        dist[j] = ok ? 1e10f : 0.f;
    }
    unsigned far = (unsigned)min(max(start[b], 0), N - 1);
    float cx = p[3 * (size_t)far], cy = p[3 * (size_t)far + 1], cz = p[3 * (size_t)far + 2];
    int *o = out + (size_t)b * npoint;
    for (int it = 0; it < npoint; ++it) {
        if (tid == 0) o[it] = (int)far;
        if (it == npoint - 1) break;
        float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bj = 0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const float dx = px[j] - cx, dy = py[j] - cy, dz = pz[j] - cz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            dist[j] = d < dist[j] ? d : dist[j];
            const bool take = dist[j] > best;  // strict: the slots ascend by index, the first of equal distances stays
            best = take ? dist[j] : best;
            bj = take ? j : bj;
            bx = take ? px[j] : bx;
            by = take ? py[j] : by;
            bz = take ? pz[j] : bz;
        }
        const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | (0xFFFFFFFFu - (unsigned)(bj * T + tid));
        unsigned long long m = wave_max_u64(key);
        if (ONE_WAVE) {
            const int w = __builtin_ctzll(__ballot(key == m));  // keys are unique: they hold the index
            cx = read_lane(bx, w);
            cy = read_lane(by, w);
            cz = read_lane(bz, w);
        } else {
            const int par = it & 1, wave = tid >> 6, nw = T >> 6;
            if (key == m) {
                s_key[par][wave] = key;
                s_c[par][wave][0] = bx;
                s_c[par][wave][1] = by;
                s_c[par][wave][2] = bz;
            }
            __syncthreads();  // the iteration's only barrier
            const bool on = lane < nw;
            const unsigned long long k2 = on ? s_key[par][lane] : 0ull;
            const float x2 = on ? s_c[par][lane][0] : 0.f, y2 = on ? s_c[par][lane][1] : 0.f, z2 = on ? s_c[par][lane][2] : 0.f;
            m = read_lane(row_max_u64(k2), 0);  // nw <= 16: the entries sit in the first row
            const int w = __builtin_ctzll(__ballot(on && k2 == m));
            cx = read_lane(x2, w);
            cy = read_lane(y2, w);
            cz = read_lane(z2, w);
        }
        far = 0xFFFFFFFFu - (unsigned)m;
    }
}

template <int PPT, bool ONE_WAVE> static void fps_launch(const float *xyz, const int *start, int B, int N, int npoint, int *out, hipStream_t stream) {
    const int T = ONE_WAVE ? 64 : ceil_div(ceil_div(N, PPT), 64) * 64;
    hipLaunchKernelGGL((k_fps<PPT, ONE_WAVE>), dim3(B), dim3(T), 0, stream, xyz, start, N, npoint, out);
}

extern "C" int smil_fps(const float *xyz, const int32_t *start, int32_t B, int32_t N, int32_t npoint, int32_t *out, void *stream_) {
    SMIL_REQUIRE(B > 0 && N > 0 && npoint > 0 && (int64_t)B * npoint <= 0x7FFFFFFF && (int64_t)B * N <= 0x7FFFFFFF / 3,
                 "smil_fps: bad sizes B=%d N=%d npoint=%d", B, N, npoint);
    if (N > SMIL_FPS_MAX_N) {
        smil_set_error("smil_fps: N=%d above SMIL_FPS_MAX_N=%d (a cloud stays in one workgroup's registers)", N, SMIL_FPS_MAX_N);
        return SMIL_E_UNSUPPORTED;
    }
    SMIL_REQUIRE(xyz && start && out, "smil_fps: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    // points per thread and workgroup size from N: one wave up to 512 points, then 4, 8, 16 points a thread in up to 1024 threads
    if (N <= 256) fps_launch<4, true>(xyz, (const int *)start, B, N, npoint, (int *)out, stream);
    else if (N <= 512) fps_launch<8, true>(xyz, (const int *)start, B, N, npoint, (int *)out, stream);
    else if (N <= 4096) fps_launch<4, false>(xyz, (const int *)start, B, N, npoint, (int *)out, stream);
    else if (N <= 8192) fps_launch<8, false>(xyz, (const int *)start, B, N, npoint, (int *)out, stream);
    else fps_launch<16, false>(xyz, (const int *)start, B, N, npoint, (int *)out, stream);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// ---- ball query -----------------------------------------------------------------------------------------------------------------
#define BQ_WAVES 4  // queries of one workgroup

struct BallArgs {
    const float *xyz;  // (B, N, 3)
    const float *q;    // (B, S, 3)
    int N, S, nr, qblocks;
    float r2[SMIL_BALL_MAX_RADII];
    int K[SMIL_BALL_MAX_RADII];   // min(nsample, N): the row width
    int *out[SMIL_BALL_MAX_RADII];  // (B, S, K[r])
};

__global__ void __launch_bounds__(64 * BQ_WAVES) k_ball_query(BallArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x / a.qblocks, s = (blockIdx.x % a.qblocks) * BQ_WAVES + (threadIdx.x >> 6);
    if (s >= a.S) return;  // (wave-uniform; the kernel has no barrier)
    const int N = a.N;
    const float *p = a.xyz + (size_t)b * N * 3;
    const size_t qi = (size_t)b * a.S + s;
    const float qx = a.q[3 * qi], qy = a.q[3 * qi + 1], qz = a.q[3 * qi + 2];
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt[SMIL_BALL_MAX_RADII], first[SMIL_BALL_MAX_RADII];
#pragma unroll
    for (int r = 0; r < SMIL_BALL_MAX_RADII; ++r) cnt[r] = first[r] = 0;
    size_t ci = (size_t)min(lane, N - 1);
    float nx = p[3 * ci], ny = p[3 * ci + 1], nz = p[3 * ci + 2];
    for (int base = 0; base < N; base += 64) {
        const float x = nx, y = ny, z = nz;
        if (base + 64 < N) {
            ci = (size_t)min(base + 64 + lane, N - 1);
            nx = p[3 * ci];
            ny = p[3 * ci + 1];
            nz = p[3 * ci + 2];
        }
        const int c = base + lane;
        const float dx = x - qx, dy = y - qy, dz = z - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        bool open = false;
#pragma unroll
        for (int r = 0; r < SMIL_BALL_MAX_RADII; ++r) {
            if (r < a.nr && cnt[r] < a.K[r]) {
                const bool in = c < N && d2 <= a.r2[r];
                const unsigned long long m = __ballot(in);
                if (m) {
                    if (cnt[r] == 0) first[r] = base + __builtin_ctzll(m);
                    const int slot = cnt[r] + __popcll(m & below);
                    if (in && slot < a.K[r]) a.out[r][qi * a.K[r] + slot] = c;
                    cnt[r] = min(a.K[r], cnt[r] + (int)__popcll(m));
                }
                open |= cnt[r] < a.K[r];
            }
        }
        if (!open) break;
    }
#pragma unroll
    for (int r = 0; r < SMIL_BALL_MAX_RADII; ++r) {
        if (r < a.nr) {
            const int pad = cnt[r] ? first[r] : N;  // no hit: N in every slot, as the reference's sort leaves it
            for (int k = cnt[r] + lane; k < a.K[r]; k += 64) a.out[r][qi * a.K[r] + k] = pad;
        }
    }
}

extern "C" int smil_ball_query(const float *xyz, const float *new_xyz, int32_t B, int32_t N, int32_t S, int32_t n_radii, const double *radii,
                               const int32_t *nsample, int32_t *const *out, void *stream_) {
    SMIL_REQUIRE(B > 0 && N > 0 && S > 0 && (int64_t)B * N <= 0x7FFFFFFF / 3 && (int64_t)B * ceil_div(S, BQ_WAVES) <= 0x7FFFFFFF,
                 "smil_ball_query: bad sizes B=%d N=%d S=%d", B, N, S);
    SMIL_REQUIRE(n_radii >= 1 && n_radii <= SMIL_BALL_MAX_RADII, "smil_ball_query: n_radii=%d outside 1 .. %d", n_radii, SMIL_BALL_MAX_RADII);
    SMIL_REQUIRE(radii && nsample && out, "smil_ball_query: null argument");
    BallArgs a;
    for (int r = 0; r < SMIL_BALL_MAX_RADII; ++r) {
        a.r2[r] = 0.f; a.K[r] = 0; a.out[r] = nullptr;
    }
    for (int r = 0; r < n_radii; ++r) {
        SMIL_REQUIRE(nsample[r] >= 1, "smil_ball_query: nsample[%d]=%d must be >= 1", r, nsample[r]);
        SMIL_REQUIRE(std::isfinite(radii[r]) && radii[r] >= 0.0, "smil_ball_query: radius[%d]=%g must be finite and >= 0", r, radii[r]);
        a.K[r] = std::min(nsample[r], N);
        SMIL_REQUIRE((int64_t)B * S * a.K[r] <= 0x7FFFFFFF, "smil_ball_query: B S nsample[%d] exceeds 2^31", r);
        a.r2[r] = (float)(radii[r] * radii[r]);  // formed in double, rounded once
        a.out[r] = (int *)out[r];
    }
    SMIL_REQUIRE(xyz && new_xyz, "smil_ball_query: null argument");
    for (int r = 0; r < n_radii; ++r) SMIL_REQUIRE(a.out[r], "smil_ball_query: null output %d", r);
    a.xyz = xyz; a.q = new_xyz; a.N = N; a.S = S; a.nr = n_radii; a.qblocks = ceil_div(S, BQ_WAVES);
    hipLaunchKernelGGL(k_ball_query, dim3(B * a.qblocks), dim3(64 * BQ_WAVES), 0, (hipStream_t)stream_, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

// ---- grouping -------------------------------------------------------------------------------------------------------------------
#define GP_TILE 64  // positions (k S + s) and channels of one LDS tile

struct GroupArgs {
    const float *xyz;      // (B, N, 3) or null: no coordinate channels
    const float *centres;  // (B, S, 3) or null: coordinates as they are
    const float *feat;     // (B, N, D) or null (D = 0)
    const int *idx;        // (B, S, K)
    int N, S, K, D, C, xyz_off, feat_off, tiles;
    float *out;            // (B, C, K, S); in the backward: d_out
    float *d_feat;         // (B, N, D)
    long long *acc;        // (B, N, D) fixed-point sums
    unsigned int *gmax;    // (B) bits of the cloud's largest |gradient|
    int max_blocks;        // workgroups per cloud of k_group_max
};

// the tile's indices (-1: outside [0, N) or behind the last position); position p = k S + s reads idx[b, s, k]
__device__ __forceinline__ void group_tile_indices(const GroupArgs &a, int b, int p0, int *s_idx) {
    if (threadIdx.x < GP_TILE) {
        const int p = p0 + threadIdx.x;
        int i = -1;
        if (p < a.K * a.S) {
            i = a.idx[((size_t)b * a.S + p % a.S) * a.K + p / a.S];
            if ((unsigned)i >= (unsigned)a.N) i = -1;
        }
        s_idx[threadIdx.x] = i;
    }
}

__global__ void __launch_bounds__(256) k_group_points(GroupArgs a) {
    __shared__ float tile[GP_TILE][GP_TILE + 1];
    __shared__ int s_idx[GP_TILE];
    const int b = blockIdx.x / a.tiles, p0 = (blockIdx.x % a.tiles) * GP_TILE, KS = a.K * a.S;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    group_tile_indices(a, b, p0, s_idx);
    __syncthreads();
    if (a.xyz && threadIdx.x < 3 * GP_TILE) {
        const int c = w, p = p0 + lane;
        if (p < KS) {
            const int i = s_idx[lane];
            float v = 0.f;
            if (i >= 0) {
                v = a.xyz[((size_t)b * a.N + i) * 3 + c];
                if (a.centres) v = v - a.centres[((size_t)b * a.S + p % a.S) * 3 + c];
            }
            a.out[((size_t)b * a.C + a.xyz_off + c) * KS + p] = v;
        }
    }
    for (int d0 = 0; d0 < a.D; d0 += GP_TILE) {
        const int d = d0 + lane;
        for (int r = w; r < GP_TILE; r += 4) {
            const int i = s_idx[r];
            tile[r][lane] = (i >= 0 && d < a.D) ? a.feat[((size_t)b * a.N + i) * a.D + d] : 0.f;
        }
        __syncthreads();
        const int p = p0 + lane;
        for (int c = w; c < GP_TILE && d0 + c < a.D; c += 4)
            if (p < KS) a.out[((size_t)b * a.C + a.feat_off + d0 + c) * KS + p] = tile[lane][c];
        __syncthreads();
    }
}

__device__ __forceinline__ int group_fix_exp(const GroupArgs &a, int b) { return fix_unit_exp(fix_max_exp(a.gmax[b]), (unsigned)(a.K * a.S)); }

__global__ void __launch_bounds__(256) k_group_max(GroupArgs a) {
    const int b = blockIdx.x / a.max_blocks, j = blockIdx.x % a.max_blocks;
    const size_t n = (size_t)a.D * a.K * a.S;
    const float *g = a.out + ((size_t)b * a.C + a.feat_off) * a.K * a.S;  // the feature channels are one contiguous range
    float m = 0.f;
    for (size_t i = (size_t)j * 256 + threadIdx.x; i < n; i += (size_t)a.max_blocks * 256) m = fmaxf(m, fabsf(g[i]));
    fix_record_max(&a.gmax[b], m);
}

__global__ void __launch_bounds__(256) k_group_add(GroupArgs a) {
    __shared__ float tile[GP_TILE][GP_TILE + 1];
    __shared__ int s_idx[GP_TILE];
    const int b = blockIdx.x / a.tiles, p0 = (blockIdx.x % a.tiles) * GP_TILE, KS = a.K * a.S;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    group_tile_indices(a, b, p0, s_idx);
    const int fix = group_fix_exp(a, b);
    __syncthreads();
    for (int d0 = 0; d0 < a.D; d0 += GP_TILE) {
        const int p = p0 + lane;
        for (int c = w; c < GP_TILE && d0 + c < a.D; c += 4)
            tile[lane][c] = p < KS ? a.out[((size_t)b * a.C + a.feat_off + d0 + c) * KS + p] : 0.f;
        __syncthreads();
        const int d = d0 + lane;
        for (int r = w; r < GP_TILE; r += 4) {
            const int i = s_idx[r];
            if (i >= 0 && d < a.D) {
                const float v = tile[r][lane];
                if (v != 0.f)
                    fix_add(&a.acc[((size_t)b * a.N + i) * a.D + d], (double)v, fix);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_group_out(GroupArgs a, int B) {
    const size_t per = (size_t)a.N * a.D, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per * B) return;
    a.d_feat[i] = fix_read(a.acc[i], group_fix_exp(a, (int)(i / per)));
}

static bool group_sizes_ok(int64_t B, int64_t N, int64_t S, int64_t K, int64_t D, int64_t C) {
    return B > 0 && N > 0 && S > 0 && K > 0 && D >= 0 && C > 0 && K * S <= 0x7FFFFFFF - GP_TILE && B * S * K <= 0x7FFFFFFF &&
           B * N * std::max<int64_t>(D, 3) <= 0x7FFFFFFF && B * ((K * S + GP_TILE - 1) / GP_TILE) <= 0x7FFFFFFF && D <= 0x7FFFFFFF - GP_TILE;
}

static void group_channels(GroupArgs &a, bool has_xyz, int D, int xyz_last) {
    a.D = D;
    a.C = (has_xyz ? 3 : 0) + D;
    a.xyz_off = xyz_last ? D : 0;
    a.feat_off = (has_xyz && !xyz_last) ? 3 : 0;
}

extern "C" int smil_group_points(const float *xyz, const float *centres, const float *features, const int32_t *idx, int32_t B, int32_t N,
                                 int32_t S, int32_t K, int32_t D, int32_t xyz_last, float *out, void *stream_) {
    GroupArgs a = {};
    group_channels(a, xyz != nullptr, D, xyz_last);
    SMIL_REQUIRE(group_sizes_ok(B, N, S, K, D, a.C), "smil_group_points: bad sizes B=%d N=%d S=%d K=%d D=%d (channels %d)", B, N, S, K, D, a.C);
    SMIL_REQUIRE(idx && out && (D == 0 || features) && (!centres || xyz), "smil_group_points: null argument");
    a.xyz = xyz; a.centres = centres; a.feat = features; a.idx = (const int *)idx; a.out = out;
    a.N = N; a.S = S; a.K = K; a.tiles = ceil_div(K * S, GP_TILE);
    hipLaunchKernelGGL(k_group_points, dim3(B * a.tiles), dim3(256), 0, (hipStream_t)stream_, a);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}

static size_t group_grad_layout(int B, int N, int D, char *base, GroupArgs &a) {
    Workspace w{base};
    a.acc = w.take<long long>((size_t)B * N * D);
    a.gmax = w.take<unsigned int>((size_t)B);
    return w.used;
}

extern "C" size_t smil_group_points_backward_workspace_bytes(int32_t B, int32_t N, int32_t D) {
    GroupArgs a;
    return (B > 0 && N > 0 && D > 0 && (int64_t)B * N * D <= 0x7FFFFFFF) ? group_grad_layout(B, N, D, nullptr, a) : 0;
}

extern "C" int smil_group_points_backward(const float *d_out, const int32_t *idx, int32_t B, int32_t N, int32_t S, int32_t K, int32_t D,
                                          int32_t has_xyz, int32_t xyz_last, float *d_features, void *workspace, void *stream_) {
    GroupArgs a = {};
    group_channels(a, has_xyz != 0, D, xyz_last);
    SMIL_REQUIRE(D > 0 && group_sizes_ok(B, N, S, K, D, a.C), "smil_group_points_backward: bad sizes B=%d N=%d S=%d K=%d D=%d", B, N, S, K, D);
    SMIL_REQUIRE(d_out && idx && d_features && workspace, "smil_group_points_backward: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    group_grad_layout(B, N, D, (char *)workspace, a);
    a.out = const_cast<float *>(d_out); a.idx = (const int *)idx; a.d_feat = d_features;
    a.N = N; a.S = S; a.K = K; a.tiles = ceil_div(K * S, GP_TILE);
    const size_t elems = (size_t)B * N * D;
    a.max_blocks = (int)std::min<size_t>(256, ((size_t)D * K * S + 255) / 256);
    SMIL_REQUIRE((int64_t)B * a.max_blocks <= 0x7FFFFFFF, "smil_group_points_backward: B=%d too large", B);
    SMIL_HIP(hipMemsetAsync(a.acc, 0, elems * sizeof(long long), stream));
    SMIL_HIP(hipMemsetAsync(a.gmax, 0, (size_t)B * sizeof(unsigned int), stream));
    hipLaunchKernelGGL(k_group_max, dim3(B * a.max_blocks), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_group_add, dim3(B * a.tiles), dim3(256), 0, stream, a);
    SMIL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_group_out, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, stream, a, B);
    SMIL_LAUNCH_CHECK();
    return SMIL_OK;
}
