// Box overlays drawn on the device (counting_detr_amd/render.py states the rule and is the host implementation; infer.py --render_worst /
// --render_ids): the chosen images of a split with their detections (true positive / false positive / ignored at IoU 0.5), centre dots,
// ground truths and exemplars, from the boxes and flags cdetr_coco_match left in device memory.
//
// cdetr_render_boxes : one workgroup per (tile of TILE_H x TILE_W pixels, canvas), one pixel per thread.  The canvas's primitives are ONE
//   list in priority order -- detection dots, detection outlines (both in evaluation order), ground-truth outlines, exemplar outlines -- and
//   a pixel takes the colour of the FIRST primitive of the list that covers it.  (Painting the list from its end to its start, every
//   primitive over what is there, leaves each pixel with the colour of the last one painted over it = the first of the list: the same image.)
//   The workgroup walks the list in chunks of CHUNK, one primitive per thread:
//     1. the thread turns its primitive into integer corners + thickness (a dot is a filled square: thickness = radius + 1) and tests its
//        band against the tile: the corners' rectangle meets the tile and the tile does not lie inside the band's hole;
//     2. ballot + popcount prefix inside the wave, the waves' counts through LDS (the idiom of detections.hip): the survivors land in LDS in
//        list order;
//     3. every undecided pixel scans the survivors up to its first hit;
//     4. a decided pixel skips later chunks, and the workgroup leaves the loop when the ballots say no pixel is left.
//   A tile beyond its canvas (the grid is sized by the largest) returns before any barrier, the whole workgroup at once.
//
// Must EQUAL the host implementation: every corner is one IEEE double add, floor, clamp and conversion; the centre x + w * 0.5 is a
// product and an add, kept apart: contraction into FMAs is switched off for this translation unit as in coco_eval.hip.  No atomics, one
// writer per byte, nothing depends on the order workgroups run in.
#pragma clang fp contract(off)

#include "common.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int TILE_H = CDETR_RENDER_TILE_H;
constexpr int TILE_W = CDETR_RENDER_TILE_W;
constexpr int CHUNK = CDETR_RENDER_CHUNK;
constexpr int THREADS = TILE_H * TILE_W;
constexpr int WAVES = THREADS / 64;
static_assert(THREADS == CHUNK && THREADS % 64 == 0, "one primitive and one pixel per thread");
constexpr int RENDER_MAX_SIDE = 16384;
constexpr int RENDER_MAX_K = 65535;

// floor(v) clamped to [-2, 32768] (v is finite or an infinity, never a NaN here)
__device__ __forceinline__ int corner(double v) { return (int)fmin(fmax(floor(v), -2.0), 32768.0); }

struct prim {
    int x0, y0, x1, y1, t;
    bool ok;
};

// the integer corners of box[4]; `dot` >= 0: the filled square of that radius around the centre instead
__device__ __forceinline__ prim prim_of(const double* __restrict__ box, int t, int dot) {
    const double x = box[0], y = box[1], w = box[2], h = box[3];
    prim p;
    p.ok = isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h);
    p.x0 = p.y0 = p.x1 = p.y1 = 0;
    p.t = t;
    if (!p.ok) return p;
    p.x0 = corner(x); p.y0 = corner(y); p.x1 = corner(x + w); p.y1 = corner(y + h);
    p.ok = p.x1 >= p.x0 && p.y1 >= p.y0;
    if (p.ok && dot >= 0) {
        const double hw = w * 0.5, hh = h * 0.5;
        const int cx = corner(x + hw), cy = corner(y + hh);
        p.x0 = cx - dot; p.x1 = cx + dot; p.y0 = cy - dot; p.y1 = cy + dot;
        p.t = dot + 1;
    }
    return p;
}

// the segment off[i] .. off[i + 1] when it lies inside 0 .. total, else an empty one
__device__ __forceinline__ void segment(const int32_t* __restrict__ off, int i, int total, int& lo, int& n) {
    lo = 0; n = 0;
    if (off == nullptr || total <= 0) return;
    const int a = off[i], b = off[i + 1];
    if (a >= 0 && b >= a && b <= total) { lo = a; n = b - a; }
}

__global__ __launch_bounds__(THREADS) void render_boxes_kernel(
    const uint8_t* __restrict__ pix, const int64_t* __restrict__ pix_off, const int32_t* __restrict__ size, const int32_t* __restrict__ sel,
    const double* __restrict__ dt_boxes, const int32_t* __restrict__ dt_off, const int32_t* __restrict__ dt_cnt,
    const uint8_t* __restrict__ matched, const uint8_t* __restrict__ det_ignored, const double* __restrict__ gt_boxes,
    const int32_t* __restrict__ gt_off, const double* __restrict__ ex_boxes, const int32_t* __restrict__ ex_off,
    const uint8_t* __restrict__ style, int K, int B, int D, int G, int E, int max_h, int max_w, int dot, long long pix_bytes,
    uint8_t* __restrict__ out) {
    __shared__ int4 s_rect[CHUNK];
    __shared__ int s_t[CHUNK];
    __shared__ unsigned s_rgb[CHUNK];
    __shared__ int s_cnt[WAVES];
    __shared__ int s_open[WAVES];

    const int k = blockIdx.z;
    const int H = size[2 * k], W = size[2 * k + 1];
    if (H < 1 || W < 1 || H > max_h || W > max_w) return;                       // not a canvas of this launch: uniform
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    if (tx0 >= W || ty0 >= H) return;                                           // a surplus tile: uniform, before any barrier
    const long long base = pix_off[k], bytes = 3ll * H * W;
    if (base < 0 || base > pix_bytes - bytes) return;                           // the canvas does not lie inside the buffers: uniform
    const int tx1 = min(tx0 + TILE_W, W) - 1, ty1 = min(ty0 + TILE_H, H) - 1;   // the tile clipped to the canvas, inclusive

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = tx0 + (int)(threadIdx.x % TILE_W), py = ty0 + (int)(threadIdx.x / TILE_W);
    const bool inside = px < W && py < H;

    const int b = sel[k];
    int d0 = 0, nd = 0, g0 = 0, ng = 0, e0 = 0, ne = 0;
    if (b >= 0 && b < B) {
        segment(dt_off, b, D, d0, nd);
        if (dt_cnt != nullptr) nd = min(nd, max(dt_cnt[b], 0));
        segment(gt_off, b, G, g0, ng);
    }
    segment(ex_off, k, E, e0, ne);
    const int n_dots = dot >= 0 ? nd : 0;
    const long long all = (long long)n_dots + nd + ng + ne;                     // four terms below 2^31 each
    const int total = (int)(all < (1ll << 30) ? all : (1ll << 30));             // the loop's index stays inside int32

    bool decided = !inside;                                                     // a thread outside the canvas has nothing to decide
    unsigned rgb = 0;
    for (int c0 = 0; c0 < total; c0 += CHUNK) {
        // 1. this thread's primitive
        const int p = c0 + (int)threadIdx.x;
        bool keep = false;
        prim q;
        q.x0 = q.y0 = q.x1 = q.y1 = q.t = 0;
        unsigned colour = 0;
        if (p < total) {
            int cls;
            if (p < n_dots + nd) {
                const bool is_dot = p < n_dots;
                const int i = d0 + (is_dot ? p : p - n_dots);
                cls = det_ignored[i] != 0 ? 2 : (matched[i] != 0 ? 0 : 1);
                q = prim_of(dt_boxes + 4 * (size_t)i, style[4 * cls + 3], is_dot ? dot : -1);
            } else if (p < n_dots + nd + ng) {
                cls = 3;
                q = prim_of(gt_boxes + 4 * (size_t)(g0 + (p - n_dots - nd)), style[4 * cls + 3], -1);
            } else {
                cls = 4;
                q = prim_of(ex_boxes + 4 * (size_t)(e0 + (p - n_dots - nd - ng)), style[4 * cls + 3], -1);
            }
            colour = (unsigned)style[4 * cls] | ((unsigned)style[4 * cls + 1] << 8) | ((unsigned)style[4 * cls + 2] << 16);
            const bool meets = q.x0 <= tx1 && q.x1 >= tx0 && q.y0 <= ty1 && q.y1 >= ty0;
            const bool in_hole = tx0 >= q.x0 + q.t && tx1 <= q.x1 - q.t && ty0 >= q.y0 + q.t && ty1 <= q.y1 - q.t;
            keep = q.ok && q.t > 0 && meets && !in_hole;
        }
        // 2. compaction in list order
        const unsigned long long m = __ballot(keep);
        const unsigned long long open = __ballot(!decided);
        if (lane == 0) {
            s_cnt[wave] = __popcll(m);
            s_open[wave] = open != 0ull;
        }
        __syncthreads();
        int before = 0, kept = 0, any_open = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            kept += s_cnt[w];
            any_open |= s_open[w];
        }
        if (!any_open) break;                                                   // uniform: every thread read the same words
        if (keep) {
            const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
            s_rect[pos] = make_int4(q.x0, q.y0, q.x1, q.y1);
            s_t[pos] = q.t;
            s_rgb[pos] = colour;
        }
        __syncthreads();
        // 3. first hit
        if (!decided) {
            for (int j = 0; j < kept; ++j) {
                const int4 r = s_rect[j];
                if (px >= r.x && px <= r.z && py >= r.y && py <= r.w && min(min(px - r.x, r.z - px), min(py - r.y, r.w - py)) < s_t[j]) {
                    rgb = s_rgb[j];
                    decided = true;
                    break;
                }
            }
        }
        // the next round's s_cnt / s_open are written after this round's reads (the barrier above) and its list after this round's scans
        // (the barrier below them)
    }
    if (!inside) return;
    const long long at = base + 3ll * ((long long)py * W + px);
    if (decided) {
        out[at] = (uint8_t)(rgb & 255u); out[at + 1] = (uint8_t)((rgb >> 8) & 255u); out[at + 2] = (uint8_t)((rgb >> 16) & 255u);
    } else {
        out[at] = pix[at]; out[at + 1] = pix[at + 1]; out[at + 2] = pix[at + 2];
    }
}

}  // namespace

extern "C" int cdetr_render_boxes(const uint8_t* pix, const int64_t* pix_off, const int32_t* size, const int32_t* sel, const int32_t* sel_host,
                                  const double* dt_boxes, const int32_t* dt_off, const int32_t* dt_cnt, const uint8_t* matched,
                                  const uint8_t* det_ignored, const double* gt_boxes, const int32_t* gt_off, const double* ex_boxes,
                                  const int32_t* ex_off, const uint8_t* style, int32_t K, int32_t B, int32_t D, int32_t G, int32_t E, int32_t max_h,
                                  int32_t max_w, int32_t dot, int64_t pix_bytes, uint8_t* out, void* stream) {
    CDETR_CHECK_ARG(K >= 0 && B >= 0 && D >= 0 && G >= 0 && E >= 0 && pix_bytes >= 0,
                    "cdetr_render_boxes: bad sizes K = %d, B = %d, D = %d, G = %d, E = %d, pix_bytes = %lld", K, B, D, G, E, (long long)pix_bytes);
    if (K > RENDER_MAX_K) {
        cdetr_set_error("cdetr_render_boxes: K = %d canvases per call (limit %d) not supported", K, RENDER_MAX_K);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (K == 0) return CDETR_OK;                  // no canvas: nothing to write
    CDETR_CHECK_ARG(pix && pix_off && size && sel && style && out, "cdetr_render_boxes: null canvas / offset / size / sel / style / output pointer");
    CDETR_CHECK_ARG(D == 0 || (dt_boxes && dt_off && matched && det_ignored), "cdetr_render_boxes: null detection box / offset / flag pointer");
    CDETR_CHECK_ARG(G == 0 || (gt_boxes && gt_off), "cdetr_render_boxes: null ground-truth box / offset pointer");
    CDETR_CHECK_ARG(E == 0 || (ex_boxes && ex_off), "cdetr_render_boxes: null exemplar box / offset pointer");
    if (max_h < 1 || max_h > RENDER_MAX_SIDE || max_w < 1 || max_w > RENDER_MAX_SIDE) {
        cdetr_set_error("cdetr_render_boxes: canvases of up to H = %d, W = %d, supported 1 .. %d", max_h, max_w, RENDER_MAX_SIDE);
        return CDETR_ERR_UNSUPPORTED;
    }
    const int gx = (max_w + TILE_W - 1) / TILE_W, gy = (max_h + TILE_H - 1) / TILE_H;
    if ((long long)gx * gy * K * THREADS > 0x7fffffffll || dot > RENDER_MAX_SIDE) {
        cdetr_set_error("cdetr_render_boxes: %d x %d tiles x %d canvases exceed one launch (2^31 threads), or dot = %d (limit %d)", gx, gy, K, dot,
                        RENDER_MAX_SIDE);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (2ll * D + G + E > (1ll << 30)) {          // the kernel's primitive index is an int32
        cdetr_set_error("cdetr_render_boxes: D = %d, G = %d, E = %d boxes: more than 2^30 primitives not supported", D, G, E);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (sel_host != nullptr) {
        for (int k = 0; k < K; ++k) {
            if (sel_host[k] < 0 || sel_host[k] >= B) {
                cdetr_set_error("cdetr_render_boxes: sel[%d] = %d names no image of the pack (B = %d)", k, sel_host[k], B);
                return CDETR_ERR_UNSUPPORTED;
            }
        }
    }
    hipLaunchKernelGGL(render_boxes_kernel, dim3(gx, gy, K), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), pix, pix_off, size, sel,
                       dt_boxes, dt_off, dt_cnt, matched, det_ignored, gt_boxes, gt_off, ex_boxes, ex_off, style, K, B, D, G, E, max_h, max_w, dot,
                       (long long)pix_bytes, out);
    return cdetr_launch_status("cdetr_render_boxes");
}
