// Tiled inference past the query cap (infer.py --tiles RxC): the three device steps around the grouped forward of an image's tiles.
//
// cdetr_tile_images        : one image [3][H][W] -> its T tiles [T][3][Hm][Wm] (a crop, or a crop upsampled by 2) and the padding mask.
// cdetr_exemplar_group_fwd : the exemplar feature of a GROUP of G tiles, pooled over all of them, written to each of the G rows.
// cdetr_tile_stitch        : the tiles' outputs -> one virtual image of slots * Q queries in whole-image coordinates; a query that is not
//                            centred in its tile's core loses its prob to NaN, which no reader counts.
//
// Everything must EQUAL the host rule (counting_detr_amd/tiling.py, numpy fp32), operation by operation: a pass of the upsampling is
// 0.75f * a + 0.25f * b, a stitched coordinate v * a + o, each multiply and each add rounded once, so contraction is switched off for this
// translation unit.  The exemplar cell is exemplar_fwd_kernel's expression (glue.hip), which the compiler does not fuse there either:
// separate products, one add, a halving, a truncation.  No atomics: every output element has one writer.
//
// These are small bandwidth-bound kernels.  The image kernel gives a thread four neighbouring pixels of a tile row: 16-byte stores (and, for
// a plain crop whose row start is aligned, 16-byte loads), the mask as one 4-byte word.
#pragma clang fp contract(off)

#include <cmath>

#include "common.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int REC = CDETR_TILE_RECORD_INTS, COEF = CDETR_TILE_COEF_FLOATS;
constexpr int TI_THREADS = 64;             // x 4 pixels: a workgroup covers 256 pixels of one tile row

// One thread = 4 neighbouring pixels (xb .. xb + 3) of row y of tile t, all three channels and the mask.  `vec`: Wm % 4 == 0 and the output
// bases are 16-byte aligned (vector stores); `vec_in`: W % 4 == 0 and the image base is 16-byte aligned (vector loads where the crop's
// column lands on a multiple of 4).
__global__ __launch_bounds__(TI_THREADS) void tile_images_kernel(const float* __restrict__ img, int H, int W, const int32_t* __restrict__ rec, int Hm,
                                                                 int Wm, float* __restrict__ tiles, uint8_t* __restrict__ mask, int vec, int vec_in) {
    const int t = blockIdx.z, y = blockIdx.y;
    const int xb = (blockIdx.x * TI_THREADS + threadIdx.x) * 4;
    if (xb >= Wm) return;
    // the tile's record is range-checked before it addresses anything: a bad one gives an all-padding tile
    const int32_t* r = rec + (size_t)t * REC;
    const int x0 = r[0], y0 = r[1], tw = r[2], th = r[3], s = r[4];
    const bool ok = (s == 1 || s == 2) && x0 >= 0 && y0 >= 0 && tw >= 1 && th >= 1 && x0 < W && y0 < H && tw <= W - x0 && th <= H - y0 &&
                    tw * s <= Wm && th * s <= Hm;
    const int ow = ok ? tw * s : 0, oh = ok ? th * s : 0;
    const int n = min(4, Wm - xb);
    const size_t plane = (size_t)Hm * Wm;
    const size_t at = (size_t)t * plane + (size_t)y * Wm + xb;              // in the mask; channel c of the tiles: (3 t + c) planes further
    const bool row_in = y < oh;

    uint8_t m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = (row_in && xb + i < ow) ? 0 : 1;
    if (vec) {
        *reinterpret_cast<uchar4*>(mask + at) = make_uchar4(m[0], m[1], m[2], m[3]);
    } else {
        for (int i = 0; i < n; ++i) mask[at + i] = m[i];
    }

    // source rows / columns (scale 2: the near pixel and its neighbour on the side the sample leans to, clamped to the IMAGE)
    int yn = 0, yf = 0;
    if (row_in) {
        if (s == 1) {
            yn = yf = y0 + y;
        } else {
            yn = y0 + (y >> 1);
            yf = min(max((y & 1) ? yn + 1 : yn - 1, 0), H - 1);
        }
    }
    for (int c = 0; c < 3; ++c) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (row_in && xb < ow) {
            const float* pn = img + ((size_t)c * H + yn) * W;
            if (s == 1) {
                const int xs = x0 + xb;
                if (vec_in && xb + 4 <= ow && (xs & 3) == 0) {
                    const float4 q = *reinterpret_cast<const float4*>(pn + xs);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (xb + i < ow) v[i] = pn[xs + i];
                }
            } else {
                const float* pf = img + ((size_t)c * H + yf) * W;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int x = xb + i;
                    if (x < ow) {
                        const int xn = x0 + (x >> 1);
                        const int xf = min(max((x & 1) ? xn + 1 : xn - 1, 0), W - 1);
                        const float hn = 0.75f * pn[xn] + 0.25f * pn[xf];       // horizontal pass on the near and on the far row
                        const float hf = 0.75f * pf[xn] + 0.25f * pf[xf];
                        v[i] = 0.75f * hn + 0.25f * hf;                         // vertical pass over its result
                    }
                }
            }
        }
        float* o = tiles + (size_t)(3 * t + c) * plane + (size_t)y * Wm + xb;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int i = 0; i < n; ++i) o[i] = v[i];
        }
    }
}

// grid (C / 256 rounded up, B / G).  exemplar_fwd_kernel (glue.hip) with per_image set, the sum running on over the G tiles of a group.
__global__ __launch_bounds__(256) void exemplar_group_fwd_kernel(const float* __restrict__ x, const float* __restrict__ rects,
                                                                 const float* __restrict__ extent, int G, int h, int w, int C, int K,
                                                                 int* __restrict__ idx, float* __restrict__ pf) {
    const int g = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.f;
    int cnt = 0;
    for (int b = g * G; b < (g + 1) * G; ++b) {
        const float hv = extent[2 * b], wv = extent[2 * b + 1];
        for (int k = 0; k < K; ++k) {
            const float* r = rects + ((long)b * K + k) * 4;
            const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
            int cell = -1;
            if (x2 >= 0.f) {
                const int xc = min(max((int)((x1 * wv + x2 * wv) / 2.f), 0), w - 1);
                const int yc = min(max((int)((y1 * hv + y2 * hv) / 2.f), 0), h - 1);
                cell = yc * w + xc;
                ++cnt;
                if (c < C) acc += x[((long)b * h * w + cell) * C + c];
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) idx[b * K + k] = cell;
        }
    }
    const float ic = 1.f / (float)max(cnt, 1);
    if (c < C) {
        const float v = acc * ic;
        for (int b = g * G; b < (g + 1) * G; ++b) pf[(long)b * C + c] = v;
    }
}

// One thread = one virtual query.
__global__ __launch_bounds__(256) void tile_stitch_kernel(const float* __restrict__ prob, const float* __restrict__ boxes,
                                                          const float* __restrict__ points, const float* __restrict__ coef, int T, int Q, int Qv,
                                                          float Wf, float Hf, float* __restrict__ prob_out, float* __restrict__ boxes_out,
                                                          float* __restrict__ points_out) {
    const int vq = blockIdx.x * 256 + threadIdx.x;
    if (vq >= Qv) return;
    const int t = vq / Q;
    float p = __builtin_nanf("");
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 r = make_float2(0.f, 0.f);
    if (t < T) {                            // (a slot without a tile: NaN, zero boxes and points)
        const float* k = coef + (size_t)t * COEF;
        const float ax = k[0], ox = k[1], ay = k[2], oy = k[3], lox = k[4], hix = k[5], loy = k[6], hiy = k[7];
        const float4 bi = reinterpret_cast<const float4*>(boxes)[vq];
        const float2 ri = reinterpret_cast<const float2*>(points)[vq];
        b.x = bi.x * ax + ox;  b.y = bi.y * ay + oy;  b.z = bi.z * ax;  b.w = bi.w * ay;
        r.x = ri.x * ax + ox;  r.y = ri.y * ay + oy;
        const float px = b.x * Wf, py = b.y * Hf;
        const float ninf = -INFINITY, pinf = INFINITY;
        const bool own = (lox == ninf || px >= lox) && (hix == pinf || px < hix) && (loy == ninf || py >= loy) && (hiy == pinf || py < hiy);
        if (own) p = prob[vq];
    }
    prob_out[vq] = p;
    reinterpret_cast<float4*>(boxes_out)[vq] = b;
    reinterpret_cast<float2*>(points_out)[vq] = r;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int cdetr_tile_images(const float* image, int32_t H, int32_t W, const int32_t* records, int32_t T, int32_t Hm, int32_t Wm, float* tiles,
                                 uint8_t* mask, void* stream) {
    CDETR_CHECK_ARG(image && records && tiles && mask, "cdetr_tile_images: null pointer");
    CDETR_CHECK_ARG(H > 0 && W > 0 && T > 0 && Hm > 0 && Wm > 0, "cdetr_tile_images: bad sizes H = %d, W = %d, T = %d, Hm = %d, Wm = %d", H, W, T, Hm, Wm);
    if (H > CDETR_TILE_MAX_SIDE || W > CDETR_TILE_MAX_SIDE || Hm > CDETR_TILE_MAX_SIDE || Wm > CDETR_TILE_MAX_SIDE || T > CDETR_TILE_MAX_VIRTUAL) {
        cdetr_set_error("cdetr_tile_images: H = %d, W = %d, Hm = %d, Wm = %d (limit %d a side) or T = %d tiles (limit %d) not supported", H, W, Hm, Wm,
                        CDETR_TILE_MAX_SIDE, T, CDETR_TILE_MAX_VIRTUAL);
        return CDETR_ERR_UNSUPPORTED;
    }
    const int vec = Wm % 4 == 0 && aligned16(tiles) && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    const int vec_in = W % 4 == 0 && aligned16(image);
    const dim3 grid(((Wm + 3) / 4 + TI_THREADS - 1) / TI_THREADS, Hm, T);
    hipLaunchKernelGGL(tile_images_kernel, grid, dim3(TI_THREADS), 0, reinterpret_cast<hipStream_t>(stream), image, H, W, records, Hm, Wm, tiles, mask,
                       vec, vec_in);
    return cdetr_launch_status("cdetr_tile_images");
}

extern "C" int cdetr_exemplar_group_fwd(const float* x, const float* rects, const float* extent, int32_t B, int32_t G, int32_t h, int32_t w,
                                        int32_t C, int32_t K, int32_t* idx, float* pf, void* stream) {
    CDETR_CHECK_ARG(x && rects && extent && idx && pf && B > 0 && h > 0 && w > 0 && C > 0 && K > 0, "cdetr_exemplar_group_fwd: bad args");
    CDETR_CHECK_ARG(G > 0 && B % G == 0, "cdetr_exemplar_group_fwd: B = %d tiles do not divide into groups of G = %d", B, G);
    if (B / G > 65535) {
        cdetr_set_error("cdetr_exemplar_group_fwd: %d groups per call (limit 65535) not supported", B / G);
        return CDETR_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(exemplar_group_fwd_kernel, dim3((C + 255) / 256, B / G), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, rects, extent, G,
                       h, w, C, K, idx, pf);
    return cdetr_launch_status("cdetr_exemplar_group_fwd");
}

extern "C" int cdetr_tile_stitch(const float* prob, const float* boxes, const float* points, const float* coef, int32_t T, int32_t Q, int32_t slots,
                                 int32_t H, int32_t W, float* prob_out, float* boxes_out, float* points_out, void* stream) {
    CDETR_CHECK_ARG(prob && boxes && points && coef && prob_out && boxes_out && points_out, "cdetr_tile_stitch: null pointer");
    CDETR_CHECK_ARG(T > 0 && Q > 0 && slots >= T && H > 0 && W > 0, "cdetr_tile_stitch: bad sizes T = %d, Q = %d, slots = %d, H = %d, W = %d", T, Q,
                    slots, H, W);
    if ((int64_t)slots * Q > CDETR_TILE_MAX_VIRTUAL) {
        cdetr_set_error("cdetr_tile_stitch: %d slots of %d queries are %lld virtual queries (limit %d): not supported", slots, Q,
                        (long long)slots * Q, CDETR_TILE_MAX_VIRTUAL);
        return CDETR_ERR_UNSUPPORTED;
    }
    CDETR_CHECK_ARG(aligned16(boxes) && aligned16(boxes_out) && (reinterpret_cast<uintptr_t>(points) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(points_out) & 7) == 0, "cdetr_tile_stitch: boxes must be 16-byte, points 8-byte aligned");
    CDETR_CHECK_ARG(prob_out != prob && boxes_out != boxes && points_out != points, "cdetr_tile_stitch: an output aliases its input");
    const int Qv = slots * Q;
    hipLaunchKernelGGL(tile_stitch_kernel, dim3((Qv + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), prob, boxes, points, coef, T, Q,
                       Qv, (float)W, (float)H, prob_out, boxes_out, points_out);
    return cdetr_launch_status("cdetr_tile_stitch");
}
