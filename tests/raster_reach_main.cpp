// Stand-alone host program around smilify_amd/csrc/raster_reach.h for tests/test_raster_rounded_boxes_cpu.py: walks faces the way
// k_raster_setup (pixel box -> tile box -> corner flags) and stage_faces (per tile: rows and columns, gaps exchanged, one trim each)
// do, with the header's functions, and writes per face and pixel what became of it.
//   usage: raster_reach_main S sqrt_blur faces.f32 masks.u8      (faces: 6 floats x0 y0 x1 y1 x2 y2 per face, NDC)
//   masks: S x S bytes per face, output order (row yo, column xo): bit 0 in the face's blurred pixel box, bit 1 still there after the
//          corner cull and the trim, bit 2 still there after the trim alone (a tile-built list: no cull)
//   stdout: "tiles T culled C slots B kept A": (face, tile) entries, culled ones, pixels of the boxes before and after
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "raster_reach.h"

static const int TILE = 8;

// rows b0 .. b1 and columns bx0 .. bx1 of tile (tx, ty) as stage_faces leaves them: each axis's gap, then each trimmed by the other's
static void stage_trim(float vx0, float vx1, float vy0, float vy1, int S, int tx, int ty, float lim2, int &bx0, int &bx1, int &b0, int &b1) {
    const int ex = S - 1 - tx * TILE, ey = S - 1 - ty * TILE;
    const float gx = bx0 <= bx1 ? reach_gap(vx0, vx1, ex - bx1, ex - bx0) : 0.f;
    const float gy = b0 <= b1 ? reach_gap(vy0, vy1, ey - b1, ey - b0) : 0.f;
    if (bx0 <= bx1) {
        int lo = ex - bx1, hi = ex - bx0;
        reach_trim(vx0, vx1, gy, lim2, lo, hi);
        bx0 = ex - hi; bx1 = ex - lo;
    }
    if (b0 <= b1) {
        int lo = ey - b1, hi = ey - b0;
        reach_trim(vy0, vy1, gx, lim2, lo, hi);
        b0 = ey - hi; b1 = ey - lo;
    }
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int S = atoi(argv[1]);
    const float sqrt_blur = (float)atof(argv[2]), fS = (float)S;
    FILE *in = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    if (!in || !out || S <= 0 || S % TILE) return 2;
    const float lim2 = reach_limit2(sqrt_blur, fS);
    const bool cull_ok = sqrt_blur * fS * 0.5f + REACH_SLACK_PX <= (float)TILE;
    long long n_tiles = 0, n_culled = 0, slots_before = 0, slots_after = 0;
    std::vector<unsigned char> mask((size_t)S * S);
    float v[6];
    while (fread(v, sizeof(float), 6, in) == 6) {
        std::fill(mask.begin(), mask.end(), 0);
        const float fx0 = fminf(fminf(v[0], v[2]), v[4]), fx1 = fmaxf(fmaxf(v[0], v[2]), v[4]);
        const float fy0 = fminf(fminf(v[1], v[3]), v[5]), fy1 = fmaxf(fmaxf(v[1], v[3]), v[5]);
        // the blurred pixel box (flipped axis) as k_raster_setup's emit takes it
        const float xlo = fx0 - sqrt_blur, xhi = fx1 + sqrt_blur, ylo = fy0 - sqrt_blur, yhi = fy1 + sqrt_blur;
        const float vxl = fminf(fmaxf(((xlo + 1.0f) * fS - 1.0f) * 0.5f - 0.01f, -1.0f), fS), vxh = fminf(fmaxf(((xhi + 1.0f) * fS - 1.0f) * 0.5f + 0.01f, -1.0f), fS);
        const float vyl = fminf(fmaxf(((ylo + 1.0f) * fS - 1.0f) * 0.5f - 0.01f, -1.0f), fS), vyh = fminf(fmaxf(((yhi + 1.0f) * fS - 1.0f) * 0.5f + 0.01f, -1.0f), fS);
        const int xi_lo = std::max((int)ceilf(vxl), 0), xi_hi = std::min((int)floorf(vxh), S - 1);
        const int yi_lo = std::max((int)ceilf(vyl), 0), yi_hi = std::min((int)floorf(vyh), S - 1);
        if (xi_lo <= xi_hi && yi_lo <= yi_hi) {
            const int xo0 = S - 1 - xi_hi, xo1 = S - 1 - xi_lo, yo0 = S - 1 - yi_hi, yo1 = S - 1 - yi_lo;
            const int tx0 = xo0 / TILE, tx1 = xo1 / TILE, ty0 = yo0 / TILE, ty1 = yo1 / TILE;
            const float vx0 = reach_px_of(fx0, fS), vx1 = reach_px_of(fx1, fS), vy0 = reach_px_of(fy0, fS), vy1 = reach_px_of(fy1, fS);
            const unsigned flags = cull_ok ? reach_corner_flags(vx0, vx1, vy0, vy1, xo0, xo1, yo0, yo1, tx0, tx1, ty0, ty1, S, TILE, lim2) : 0u;
            for (int ty = ty0; ty <= ty1; ++ty)
                for (int tx = tx0; tx <= tx1; ++tx) {
                    const bool culled = reach_corner_culled(flags, tx, ty, tx0, tx1, ty0, ty1);
                    ++n_tiles;
                    n_culled += culled ? 1 : 0;
                    // the square inside the tile (tile-local output rows / columns, every pixel open), then the trim
                    const int sx0 = std::max(xo0 - tx * TILE, 0), sx1 = std::min(xo1 - tx * TILE, TILE - 1);
                    const int sy0 = std::max(yo0 - ty * TILE, 0), sy1 = std::min(yo1 - ty * TILE, TILE - 1);
                    int bx0 = sx0, bx1 = sx1, b0 = sy0, b1 = sy1;
                    stage_trim(vx0, vx1, vy0, vy1, S, tx, ty, lim2, bx0, bx1, b0, b1);
                    const bool any = bx0 <= bx1 && b0 <= b1;
                    slots_before += (long long)(sx1 - sx0 + 1) * (sy1 - sy0 + 1);
                    if (any && !culled) slots_after += (long long)(bx1 - bx0 + 1) * (b1 - b0 + 1);
                    for (int y = sy0; y <= sy1; ++y)
                        for (int x = sx0; x <= sx1; ++x) {
                            const bool in = any && x >= bx0 && x <= bx1 && y >= b0 && y <= b1;
                            mask[(size_t)(ty * TILE + y) * S + tx * TILE + x] = 1 | (in && !culled ? 2 : 0) | (in ? 4 : 0);
                        }
                }
        }
        fwrite(mask.data(), 1, mask.size(), out);
    }
    fclose(out);
    printf("tiles %lld culled %lld slots %lld kept %lld\n", n_tiles, n_culled, slots_before, slots_after);
    return 0;
}
