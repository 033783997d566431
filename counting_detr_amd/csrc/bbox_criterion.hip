// bbox_criterion.hip -- the 1st-stage BoundingBoxCriterion (A1/models/anchor_detr.py:317-337) as one forward + one backward launch.
//
// With M = B*N matched pairs (query n of image b <-> exemplar n: no matcher in stage 1), src = [tgt_points, pred_wh] and
// tgt = [tgt_points, tgt_whs] (cxcywh, concentric by construction):
//   loss_wh   = mean |pred_wh - tgt_whs|                        over 2M elements (F.l1_loss)
//   loss_giou = sum (1 - GIoU(xyxy(src), xyxy(tgt))) / M        (box_ops.generalized_box_iou_pairs)
//   total     = w_wh * loss_wh + w_giou * loss_giou             (A1/engine.py: sum of loss_dict[k] * weight_dict[k])
// cdetr_bbox_criterion_fwd reads pred_wh IN PLACE (pointer + row stride: the [..., 2:] columns of the box head's [B,Q,4] output), writes
// the three scalars and the per-element gradient of each loss w.r.t. pred_wh; cdetr_bbox_criterion_bwd is the scaled sum of the two.
// The GIoU gradient is the reverse-mode chain of the torch composition, node by node, with torch's subgradients: sign(0) = 0,
// torch.max / torch.min split the gradient evenly at equal operands, clamp(min=0) passes it at 0.  Ties are the common case here, not a
// measure-zero event: the boxes are concentric, so pred_w == tgt_w makes BOTH x corners equal.
// ONE workgroup; every thread owns a fixed, strided set of pairs; per-wave shuffle tree then a serial sum over the waves: bit-reproducible,
// no atomics, any M >= 1.
#include "../../include/cdetr_hip.h"
#include "common.h"

// no a*b+c contraction in this file: every product and sum rounds on its own, as in the torch composition it restates
#pragma clang fp contract(off)

namespace {

constexpr int BC_THREADS = 256;
constexpr int BC_WAVES = BC_THREADS / 64;

__host__ __device__ __forceinline__ float bc_sgn(float x) { return (float)((x > 0.f) - (x < 0.f)); }
// d max(a, b) / d a  and  d min(a, b) / d a  (torch.maximum / torch.minimum: an equal pair splits the gradient evenly)
__host__ __device__ __forceinline__ float bc_wmax(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__host__ __device__ __forceinline__ float bc_wmin(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }
__host__ __device__ __forceinline__ float bc_max(float a, float b) { return a > b ? a : (b > a ? b : a); }
__host__ __device__ __forceinline__ float bc_min(float a, float b) { return a < b ? a : (b < a ? b : a); }

struct BcPair {
    float l1;           // |dw| + |dh|
    float one_m_giou;   // 1 - GIoU
    float gw, gh;       // d (1 - GIoU) / d (w, h)   (unit upstream gradient per pair)
};

// One pair.  The forward follows box_ops.generalized_box_iou_pairs expression by expression; the backward visits the same nodes in
// reverse with torch's derivative formulas (div: d num = g / den, d den = -g * ((num / den) / den)).
__host__ __device__ __forceinline__ BcPair bc_pair(float cx, float cy, float pw, float ph, float tw, float th) {
    BcPair r;
    const float ew = pw - tw, eh = ph - th;
    r.l1 = fabsf(ew) + fabsf(eh);
    const float hpw = 0.5f * pw, hph = 0.5f * ph, htw = 0.5f * tw, hth = 0.5f * th;
    const float x1 = cx - hpw, y1 = cy - hph, x2 = cx + hpw, y2 = cy + hph;
    const float u1 = cx - htw, v1 = cy - hth, u2 = cx + htw, v2 = cy + hth;
    const float a1w = x2 - x1, a1h = y2 - y1, a2w = u2 - u1, a2h = v2 - v1;
    const float a1 = a1w * a1h, a2 = a2w * a2h;
    const float ltx = bc_max(x1, u1), lty = bc_max(y1, v1), rbx = bc_min(x2, u2), rby = bc_min(y2, v2);
    const float iw0 = rbx - ltx, ih0 = rby - lty;
    const float iw = iw0 < 0.f ? 0.f : iw0, ih = ih0 < 0.f ? 0.f : ih0;
    const float inter = iw * ih;
    const float uni = (a1 + a2) - inter;
    const float iou = inter / uni;
    const float ex1 = bc_min(x1, u1), ey1 = bc_min(y1, v1), ex2 = bc_max(x2, u2), ey2 = bc_max(y2, v2);
    const float cw0 = ex2 - ex1, ch0 = ey2 - ey1;
    const float cw = cw0 < 0.f ? 0.f : cw0, ch = ch0 < 0.f ? 0.f : ch0;
    const float area = cw * ch;
    const float num = area - uni;
    const float q = num / area;
    const float giou = iou - q;
    r.one_m_giou = 1.f - giou;
    // ---- reverse mode, upstream d(1 - giou) = 1  ->  d giou = -1
    const float d_giou = -1.f;
    const float d_iou = d_giou, d_q = -d_giou;
    const float d_num = d_q / area;
    float d_area = -d_q * (q / area);
    d_area += d_num;
    float d_uni = -d_num;
    float d_inter = d_iou / uni;
    d_uni += -d_iou * (iou / uni);
    const float d_a1 = d_uni;
    d_inter += -d_uni;
    // enclosing box
    const float d_cw = d_area * ch, d_ch = d_area * cw;
    const float d_cw0 = cw0 >= 0.f ? d_cw : 0.f, d_ch0 = ch0 >= 0.f ? d_ch : 0.f;
    // intersection
    const float d_iw = d_inter * ih, d_ih = d_inter * iw;
    const float d_iw0 = iw0 >= 0.f ? d_iw : 0.f, d_ih0 = ih0 >= 0.f ? d_ih : 0.f;
    // area of the source box
    const float d_a1w = d_a1 * a1h, d_a1h = d_a1 * a1w;
    // corners of the source box: x2 / y2 from rb (min), ex2 (max), a1; x1 / y1 from lt (max), ex1 (min), a1
    const float d_x2 = d_iw0 * bc_wmin(x2, u2) + d_cw0 * bc_wmax(x2, u2) + d_a1w;
    const float d_y2 = d_ih0 * bc_wmin(y2, v2) + d_ch0 * bc_wmax(y2, v2) + d_a1h;
    const float d_x1 = -d_iw0 * bc_wmax(x1, u1) - d_cw0 * bc_wmin(x1, u1) - d_a1w;
    const float d_y1 = -d_ih0 * bc_wmax(y1, v1) - d_ch0 * bc_wmin(y1, v1) - d_a1h;
    // x1 = cx - 0.5 w, x2 = cx + 0.5 w
    r.gw = 0.5f * d_x2 - 0.5f * d_x1;
    r.gh = 0.5f * d_y2 - 0.5f * d_y1;
    return r;
}

// valid rows of image b: clamp(lens[b], 0, N)
__device__ __forceinline__ int bc_len(const int32_t* __restrict__ lens, int b, int N) { return min(max(lens[b], 0), N); }

// LENS (cdetr_bbox_criterion_lens_*): `rows` = B*N rows of B images, row n of image b is a pair iff n < lens[b]; the normaliser M = sum(lens) is
// formed HERE from device memory (every thread sums the same B words in the same order), so a captured graph follows new counts.  A padded
// row is skipped by branch -- its prediction and targets are never read -- and gets exact-zero gradients.  The pair -> thread map is the
// dense kernel's over B*N, so with every lens[b] == N each partial sum, and the result, is the dense kernel's bit for bit.
template <bool LENS>
__global__ __launch_bounds__(BC_THREADS) void bbox_criterion_fwd_kernel(const float* __restrict__ pred_wh, const int64_t pred_stride,
                                                                         const float* __restrict__ tgt_points, const float* __restrict__ tgt_whs,
                                                                         const int rows, const float w_wh, const float w_giou,
                                                                         float* __restrict__ losses, float* __restrict__ g_wh,
                                                                         float* __restrict__ g_giou, const int32_t* __restrict__ lens, const int N) {
    __builtin_amdgcn_s_setprio(3);                   // one workgroup on the step's critical path (as criterion_fwd_kernel)
    __shared__ float wred[2][BC_WAVES];
    const int tid = threadIdx.x;
    int M = rows;
    if constexpr (LENS) {
        M = 0;
        for (int b = 0; b < rows / N; ++b) M += bc_len(lens, b, N);
    }
    const bool any = !LENS || M > 0;
    const float inv_2m = any ? 1.f / (float)(2 * M) : 0.f, inv_m = any ? 1.f / (float)M : 0.f;
    float l1 = 0.f, gl = 0.f;
    for (int i = tid; i < rows; i += BC_THREADS) {   // fixed pair -> thread map: the partial sums do not depend on timing
        if constexpr (LENS) {
            if (i % N >= bc_len(lens, i / N, N)) {
                g_wh[2 * i] = 0.f; g_wh[2 * i + 1] = 0.f; g_giou[2 * i] = 0.f; g_giou[2 * i + 1] = 0.f;
                continue;
            }
        }
        const float* p = pred_wh + (int64_t)i * pred_stride;
        const BcPair r = bc_pair(tgt_points[2 * i], tgt_points[2 * i + 1], p[0], p[1], tgt_whs[2 * i], tgt_whs[2 * i + 1]);
        l1 += r.l1;
        gl += r.one_m_giou;
        g_wh[2 * i] = bc_sgn(p[0] - tgt_whs[2 * i]) * inv_2m;
        g_wh[2 * i + 1] = bc_sgn(p[1] - tgt_whs[2 * i + 1]) * inv_2m;
        g_giou[2 * i] = r.gw * inv_m;
        g_giou[2 * i + 1] = r.gh * inv_m;
    }
    l1 = wave_sum(l1);
    gl = wave_sum(gl);
    if ((tid & 63) == 0) {
        wred[0][tid >> 6] = l1;
        wred[1][tid >> 6] = gl;
    }
    __syncthreads();
    if (tid == 0) {
        float s1 = 0.f, s2 = 0.f;
        for (int w = 0; w < BC_WAVES; ++w) {
            s1 += wred[0][w];
            s2 += wred[1][w];
        }
        const float lwh = any ? s1 / (float)(2 * M) : 0.f, lgi = any ? s2 / (float)M : 0.f;
        losses[0] = lwh;
        losses[1] = lgi;
        losses[2] = __fadd_rn(__fmul_rn(lwh, w_wh), __fmul_rn(lgi, w_giou));      // (no contraction: the host-side sum's rounding)
    }
}

// d_coord [M][4] = (0, 0, e_wh * g_wh + e_giou * g_giou) with e_k = g3[k] + g3[2] * w_k
template <bool LENS>
__global__ __launch_bounds__(BC_THREADS) void bbox_criterion_bwd_kernel(const float* __restrict__ g3, const float w_wh, const float w_giou,
                                                                         const float* __restrict__ g_wh, const float* __restrict__ g_giou,
                                                                         float* __restrict__ d_coord, const int M,
                                                                         const int32_t* __restrict__ lens, const int N) {
    const float e_wh = __fadd_rn(g3[0], __fmul_rn(g3[2], w_wh)), e_gi = __fadd_rn(g3[1], __fmul_rn(g3[2], w_giou));
    for (int i = blockIdx.x * BC_THREADS + threadIdx.x; i < M; i += gridDim.x * BC_THREADS) {
        if constexpr (LENS) {
            if (i % N >= bc_len(lens, i / N, N)) {   // padded pair: exact zeros whatever the upstream gradient holds
                *reinterpret_cast<float4*>(d_coord + 4 * (int64_t)i) = make_float4(0.f, 0.f, 0.f, 0.f);
                continue;
            }
        }
        // e_wh g_wh + e_gi g_giou with the roundings spelled out: one product rounds, the other is fused into the sum -- which one, per
        // column, is what the compiler made of the plain product-sum in the dense kernel all along (the intrinsics contract); written as
        // fmaf so that both instantiations round alike whatever surrounds them
        const float dw = fmaf(e_wh, g_wh[2 * i], e_gi * g_giou[2 * i]);
        const float dh = fmaf(e_gi, g_giou[2 * i + 1], e_wh * g_wh[2 * i + 1]);
        *reinterpret_cast<float4*>(d_coord + 4 * (int64_t)i) = make_float4(0.f, 0.f, dw, dh);
    }
}

}  // namespace

extern "C" int cdetr_bbox_criterion_fwd(const float* pred_wh, int64_t pred_stride, const float* tgt_points, const float* tgt_whs, int32_t M,
                                        float w_wh, float w_giou, float* losses, float* g_wh, float* g_giou, void* stream) {
    CDETR_CHECK_ARG(pred_wh && tgt_points && tgt_whs && losses && g_wh && g_giou, "cdetr_bbox_criterion_fwd: null pointer");
    CDETR_CHECK_ARG(M > 0 && M <= (1 << 28) && pred_stride >= 2, "cdetr_bbox_criterion_fwd: bad sizes (M %d, pred_stride %lld)", M,
                    (long long)pred_stride);
    hipLaunchKernelGGL(bbox_criterion_fwd_kernel<false>, dim3(1), dim3(BC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), pred_wh, pred_stride,
                       tgt_points, tgt_whs, M, w_wh, w_giou, losses, g_wh, g_giou, nullptr, 1);
    return cdetr_launch_status("cdetr_bbox_criterion_fwd");
}

extern "C" int cdetr_bbox_criterion_bwd(const float* g3, float w_wh, float w_giou, const float* g_wh, const float* g_giou, float* d_coord,
                                        int32_t M, void* stream) {
    CDETR_CHECK_ARG(g3 && g_wh && g_giou && d_coord && M > 0 && M <= (1 << 28), "cdetr_bbox_criterion_bwd: bad args");
    CDETR_CHECK_ARG((reinterpret_cast<uintptr_t>(d_coord) & 15) == 0, "cdetr_bbox_criterion_bwd: d_coord must be 16-byte aligned");
    int blocks = (M + BC_THREADS - 1) / BC_THREADS;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(bbox_criterion_bwd_kernel<false>, dim3(blocks), dim3(BC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), g3, w_wh, w_giou,
                       g_wh, g_giou, d_coord, M, nullptr, 1);
    return cdetr_launch_status("cdetr_bbox_criterion_bwd");
}

extern "C" int cdetr_bbox_criterion_lens_fwd(const float* pred_wh, int64_t pred_stride, const float* tgt_points, const float* tgt_whs,
                                             const int32_t* lens, int32_t B, int32_t N, float w_wh, float w_giou, float* losses, float* g_wh,
                                             float* g_giou, void* stream) {
    CDETR_CHECK_ARG(pred_wh && tgt_points && tgt_whs && lens && losses && g_wh && g_giou, "cdetr_bbox_criterion_lens_fwd: null pointer");
    CDETR_CHECK_ARG(B > 0 && N > 0 && (int64_t)B * N <= (1 << 28) && pred_stride >= 2,
                    "cdetr_bbox_criterion_lens_fwd: bad sizes (B %d, N %d, pred_stride %lld)", B, N, (long long)pred_stride);
    hipLaunchKernelGGL(bbox_criterion_fwd_kernel<true>, dim3(1), dim3(BC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), pred_wh, pred_stride,
                       tgt_points, tgt_whs, B * N, w_wh, w_giou, losses, g_wh, g_giou, lens, N);
    return cdetr_launch_status("cdetr_bbox_criterion_lens_fwd");
}

extern "C" int cdetr_bbox_criterion_lens_bwd(const float* g3, float w_wh, float w_giou, const float* g_wh, const float* g_giou,
                                             const int32_t* lens, float* d_coord, int32_t B, int32_t N, void* stream) {
    CDETR_CHECK_ARG(g3 && g_wh && g_giou && lens && d_coord, "cdetr_bbox_criterion_lens_bwd: null pointer");
    CDETR_CHECK_ARG(B > 0 && N > 0 && (int64_t)B * N <= (1 << 28), "cdetr_bbox_criterion_lens_bwd: bad sizes (B %d, N %d)", B, N);
    CDETR_CHECK_ARG((reinterpret_cast<uintptr_t>(d_coord) & 15) == 0, "cdetr_bbox_criterion_lens_bwd: d_coord must be 16-byte aligned");
    const int M = B * N;
    int blocks = (M + BC_THREADS - 1) / BC_THREADS;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(bbox_criterion_bwd_kernel<true>, dim3(blocks), dim3(BC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), g3, w_wh, w_giou,
                       g_wh, g_giou, d_coord, M, lens, N);
    return cdetr_launch_status("cdetr_bbox_criterion_lens_bwd");
}
