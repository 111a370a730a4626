// The tile sweep of the hard (blur 0, K = 1) rasteriser, shared by the kernels that draw from smil_colour_setup's tables:
// k_colour_tiles (shade.hip: HardPhong) and k_fragment_tiles (fragments.hip: pix_to_face / zbuf / bary / dist).
//
// One wave per 8x8 tile, lane = pixel, grid-stride over the work items, heaviest cost class first.  The tile's list is read 64 entries
// at a time; a face whose nearest vertex is farther than every pixel's current hit is not fetched at all.  The others are gathered in
// parallel (lane = face: vertex ids through the clip tables, affine forms of the three perspective-correct barycentric numerators
// relative to the tile centre) and then evaluated one after the other by all 64 pixels (readlane).  A pixel keeps the smallest
// (depth, parent face, part): the naive kernel's order with clip_faces' numbering.  The winner's barycentrics are mapped back to the
// original face (each vertex of a cut face's part is a known barycentric point of it) and handed to the caller's epilogue.
//
// `Args` is the kernel's own argument struct; the sweep reads its members cs (ColourSetup), verts_ndc (N,V,3), faces (F,3), V, F, S,
// tiles_x and z_clip, so that each kernel keeps the argument layout it had.  `epilogue(img, pix, orig, P0, P1, P2, b, pz)` runs once
// for every pixel with a hit: image, yo * S + xo, original face id and its vertex ids, barycentrics with respect to it, the winner's
// view depth.  Background pixels are never visited: a background kernel writes them first.
#pragma once
#include "common.h"

#define C_EPS 1e-8f  // pytorch3d kEpsilon of the rasteriser

// corner of face (P0, P1, P2) that holds vertex id v (the first one: a face with a repeated vertex has no area and is never drawn)
__device__ __forceinline__ int corner_of(int v, int P0, int P1, int P2) { return v == P0 ? 0 : (v == P1 ? 1 : 2); }

template <class Args, class Epilogue>
__device__ __forceinline__ void hard_tile_sweep(const Args &a, Epilogue epilogue) {
    const ColourSetup &cs = a.cs;
    const int lane = threadIdx.x;
    const int S = a.S, V = a.V, F = a.F, tiles_x = a.tiles_x, n_tiles = tiles_x * tiles_x;
    // work items, heaviest class first: order index k = class * n_parts + part, the counts' inclusive prefix in lane k
    const int nk = cs.n_parts * cs.n_classes;
    uint32_t cnt = 0u;
    if (lane < nk) cnt = cs.n_class[(lane % cs.n_parts) * cs.n_classes + lane / cs.n_parts];
    uint32_t incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += u;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, nk - 1, 64);
    const uint32_t excl = incl - cnt;
    if (lane >= nk) incl = 0xFFFFFFFFu;

    const int xl = lane & (TILE - 1), yl = lane >> 3;
    for (uint32_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int k = __popcll(__ballot(incl <= t));  // (lanes >= nk never count)
        const uint32_t slot = t - (uint32_t)read_lane((int)excl, k);
        const int part = k % cs.n_parts, cls = k / cs.n_parts;
        // (k_raster_setup's own formula, from (class, slot); the silhouette kernels' `item_at` starts from the item's number in its partition)
        const size_t idx = (size_t)(2 * part + (cls >> 1)) * cs.item_cap + ((cls & 1) ? cs.item_cap - 1u - slot : slot);
        const uint4 it = cs.items[idx];
        const int img = (int)(it.x / (uint32_t)n_tiles), tile = (int)(it.x % (uint32_t)n_tiles);
        const int tx = tile % tiles_x, ty = tile / tiles_x;
        const int xo = tx * TILE + xl, yo = ty * TILE + yl;
        const bool in_img = xo < S && yo < S;
        // pixel centre relative to the tile's centre (column xo holds image x index S - 1 - xo, as on the silhouette path)
        const float cx = pix_to_ndc(S - 1 - (tx * TILE + TILE / 2), S), cy = pix_to_ndc(S - 1 - (ty * TILE + TILE / 2), S);
        const float dx = pix_to_ndc(S - 1 - xo, S) - cx, dy = pix_to_ndc(S - 1 - yo, S) - cy;

        const float *vn = a.verts_ndc + (size_t)img * V * 3;
        const float *xv_n = cs.xv + (size_t)img * cs.clip_vx * 3;
        const int *xf_n = cs.xf + (size_t)img * cs.clip_fx * 3;
        const int *xpar_n = cs.xparent + (size_t)img * (cs.clip_fx / 2);
        float bz = __builtin_inff(), bw0 = 0.f, bw1 = 0.f, bw2 = 0.f;
        uint32_t bkey = 0xFFFFFFFFu;
        int bfid = -1;
        float tile_far = __builtin_inff();  // largest current depth over the tile's pixels (inf while one has no hit)

        // one batch of up to 64 candidate faces, face f / nearest vertex depth zmin in lane j
        auto batch = [&](bool valid, int f, float zmin) {
            const bool keep = valid && zmin <= tile_far;
            unsigned long long mask = __ballot(keep);
            if (!mask) return;
            float A0 = 0.f, B0 = 0.f, C0 = 0.f, A1 = 0.f, B1 = 0.f, C1 = 0.f, A2 = 0.f, B2 = 0.f, C2 = 0.f, z0 = 0.f, z1 = 0.f, z2 = 0.f;
            uint32_t key = 0u;
            if (keep) {
                int id[3];
                float X[3], Y[3], Z[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    id[c] = f < F ? a.faces[3 * f + c] : xf_n[3 * (f - cs.FP) + c];
                    const float *p = id[c] < V ? vn + 3 * id[c] : xv_n + 3 * (id[c] - V);
                    X[c] = p[0] - cx; Y[c] = p[1] - cy; Z[c] = p[2];
                }
                key = f < F ? 2u * (uint32_t)f : 2u * (uint32_t)xpar_n[(f - cs.FP) >> 1] + (uint32_t)((f - cs.FP) & 1);
                // b_i = edge_i(p) / area, area = edge(v2; v0, v1) + eps; w_i = b_i z_j z_k (perspective-correct numerators)
                const float area = (X[2] - X[0]) * (Y[1] - Y[0]) - (Y[2] - Y[0]) * (X[1] - X[0]) + C_EPS;
                const float ia = 1.0f / area;
                const float s0 = Z[1] * Z[2] * ia, s1 = Z[0] * Z[2] * ia, s2 = Z[0] * Z[1] * ia;
                // edge(p; a, b) = (px - ax)(by - ay) - (py - ay)(bx - ax)
                A0 = (Y[2] - Y[1]) * s0; B0 = -(X[2] - X[1]) * s0; C0 = (-X[1] * (Y[2] - Y[1]) + Y[1] * (X[2] - X[1])) * s0;
                A1 = (Y[0] - Y[2]) * s1; B1 = -(X[0] - X[2]) * s1; C1 = (-X[2] * (Y[0] - Y[2]) + Y[2] * (X[0] - X[2])) * s1;
                A2 = (Y[1] - Y[0]) * s2; B2 = -(X[1] - X[0]) * s2; C2 = (-X[0] * (Y[1] - Y[0]) + Y[0] * (X[1] - X[0])) * s2;
                z0 = Z[0]; z1 = Z[1]; z2 = Z[2];
            }
            while (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                const float w0 = fmaf(read_lane(A0, j), dx, fmaf(read_lane(B0, j), dy, read_lane(C0, j)));
                const float w1 = fmaf(read_lane(A1, j), dx, fmaf(read_lane(B1, j), dy, read_lane(C1, j)));
                const float w2 = fmaf(read_lane(A2, j), dx, fmaf(read_lane(B2, j), dy, read_lane(C2, j)));
                if (w0 > 0.f && w1 > 0.f && w2 > 0.f) {
                    const float den = fmaxf(w0 + w1 + w2, C_EPS);
                    const float pz = (w0 * read_lane(z0, j) + w1 * read_lane(z1, j) + w2 * read_lane(z2, j)) / den;
                    const uint32_t kj = (uint32_t)read_lane((int)key, j);
                    if (pz >= 0.f && (pz < bz || (pz == bz && kj < bkey))) {
                        bz = pz; bkey = kj; bfid = read_lane(f, j); bw0 = w0; bw1 = w1; bw2 = w2;
                    }
                }
            }
            tile_far = wave_max(in_img ? bz : 0.f);
        };

        if (it.z != 0xFFFFFFFFu) {  // binned list
            const uint2 *lst = cs.lists + (size_t)img * cs.list_cap + it.y;
            for (uint32_t base = 0; base < it.z; base += 64u) {
                const bool valid = base + (uint32_t)lane < it.z;
                const uint2 e = valid ? lst[base + lane] : make_uint2(0u, 0u);
                batch(valid, (int)e.x, __uint_as_float(e.y));
            }
        } else {  // the image's lists did not fit: the faces whose tile box holds the tile, 64-face group by group
            const int n_groups = cs.FT / WAVE;
            for (int g = 0; g < n_groups; ++g) {
                const uint32_t gb = cs.gbox[(size_t)img * n_groups + g];
                if (!((int)(gb & 0xFF) <= tx && tx <= (int)((gb >> 16) & 0xFF) && (int)((gb >> 8) & 0xFF) <= ty && ty <= (int)(gb >> 24))) continue;
                const int f = g * WAVE + lane;
                const uint32_t tb = cs.tbox[(size_t)img * cs.FT + f];
                const bool valid = (int)(tb & 0xFF) <= tx && tx <= (int)((tb >> 16) & 0xFF) && (int)((tb >> 8) & 0xFF) <= ty && ty <= (int)(tb >> 24);
                batch(valid, f, valid ? cs.fzr[(size_t)img * cs.FT + f].x : 0.f);
            }
        }

        if (!in_img) continue;
        const size_t pix = (size_t)yo * S + xo;
        if (bfid < 0) {  // (the background pass has written this pixel)
            continue;
        }
        // barycentrics of the winner (unclipped, perspective-corrected), mapped to the original face
        const float iden = 1.0f / fmaxf(bw0 + bw1 + bw2, C_EPS);
        const float p[3] = {bw0 * iden, bw1 * iden, bw2 * iden};
        int orig;
        float b[3];
        int P0, P1, P2;
        if (bfid < F) {
            orig = bfid;
            P0 = a.faces[3 * orig]; P1 = a.faces[3 * orig + 1]; P2 = a.faces[3 * orig + 2];
            b[0] = p[0]; b[1] = p[1]; b[2] = p[2];
        } else {
            const int r = bfid - cs.FP;
            orig = xpar_n[r >> 1];
            P0 = a.faces[3 * orig]; P1 = a.faces[3 * orig + 1]; P2 = a.faces[3 * orig + 2];
            b[0] = 0.f; b[1] = 0.f; b[2] = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s = xf_n[3 * r + c];
                if (s < V) {
                    b[corner_of(s, P0, P1, P2)] += p[c];
                } else {  // new vertex on edge (u, w): view-space point (1 - t) X_u + t X_w, t = (z_u - z_clip) / (z_u - z_w)
                    const int2 e = cs.xsrc[(size_t)img * cs.clip_vx + (s - V)];
                    const float zu = vn[3 * e.x + 2], zw = vn[3 * e.y + 2];
                    const float tw = (zu - a.z_clip) / (zu - zw);
                    b[corner_of(e.x, P0, P1, P2)] += p[c] * (1.0f - tw);
                    b[corner_of(e.y, P0, P1, P2)] += p[c] * tw;
                }
            }
        }
        epilogue(img, pix, orig, P0, P1, P2, b, bz);
    }
}
