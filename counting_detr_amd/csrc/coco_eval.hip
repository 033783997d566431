// COCO box-AP evaluation on the device (counting_detr_amd/coco_ap.py is the host restatement and the checker).
//
// cdetr_box_iou_xywh : the float64 IoU matrix of xywh boxes, operation by operation what coco_ap.box_iou_xywh evaluates in numpy.
// cdetr_coco_match   : COCOeval's greedy matcher (coco_ap._evaluate_image) for a whole batch of images in one launch:
//                      one workgroup per (image, area range), one wave per IoU threshold, lanes over the ground truths.
//
// Both must agree with numpy BIT FOR BIT: a detection is matched on `iou >= threshold` and ties between ground truths are decided
// by `==`.  IEEE double +, -, *, / are correctly rounded on gfx950 as on the host; what would differ is a*b + c contracted into one
// FMA (hipcc's default), so contraction is switched off for this translation unit.  No fast-math anywhere in the build.
#pragma clang fp contract(off)

#include "records.h"      // iou_xywh
#include "../../include/cdetr_hip.h"

namespace {

constexpr int COCO_MAX_T = 16;        // IoU thresholds = waves of a workgroup
constexpr int COCO_MAX_G = 4096;      // ground truths per image: 64 lanes x the 64 bits of a lane's taken-mask; 4 x 8 B x 4096 = 128 KiB of LDS

__global__ __launch_bounds__(256) void box_iou_kernel(const double* __restrict__ dt, int D, const double* __restrict__ gt, int G,
                                                      double* __restrict__ iou) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int d0 = blockIdx.y * 16;
    if (g >= G) return;
    const double gx = gt[4 * (size_t)g], gy = gt[4 * (size_t)g + 1], gw = gt[4 * (size_t)g + 2], gh = gt[4 * (size_t)g + 3];
    for (int d = d0; d < min(d0 + 16, D); ++d) {
        const double dx = dt[4 * (size_t)d], dy = dt[4 * (size_t)d + 1], dw = dt[4 * (size_t)d + 2], dh = dt[4 * (size_t)d + 3];
        iou[(size_t)d * G + g] = iou_xywh(dx, dy, dw, dh, gx, gy, gw, gh);
    }
}

// arg-max of the key (iou, index) over the wave: the larger IoU, among equal IoUs the larger index.  A lane without a candidate carries
// (threshold, -1): a real candidate at exactly the threshold beats it on the index.  Every lane ends with the same pair.
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (ov > v || (ov == v && oi > i)) { v = ov; i = oi; }
    }
}

// One workgroup = one (image b, area range a); wave ti = IoU threshold ti; lane l owns the ground truths l, l + 64, ... (bit k of the
// lane's 64-bit masks = ground truth 64 k + l).  The detections arrive in evaluation order and are walked serially; the IoU of a pair is
// recomputed by every wave (a [D, G] float64 matrix per image would be 33 MB at 1100 x 3731).  The boxes sit in LDS as four planes
// (x | y | w | h, `cap` doubles each: lanes read consecutive doubles).  No communication beyond the wave after the staging barrier.
__global__ __launch_bounds__(1024) void coco_match_kernel(cdetr_coco_match_desc p, int cap) {
    extern __shared__ double lds_box[];
    const int b = blockIdx.x, a = blockIdx.y;
    const int lane = threadIdx.x & 63, ti = threadIdx.x >> 6;
    const int g0 = p.gt_off[b], g1 = p.gt_off[b + 1], d0 = p.dt_off[b], d1 = p.dt_off[b + 1];
    const int G = g1 - g0, D = d1 - d0;
    // an offset table that does not describe this launch's buffers: touch nothing (the host wrapper builds the tables and Gmax together)
    if (g0 < 0 || G < 0 || g1 > p.Gtot || d0 < 0 || D < 0 || d1 > p.Dtot || G > cap) return;
    const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];

    for (int i = threadIdx.x; i < G; i += blockDim.x) {
        const double* s = p.gt_boxes + 4 * (size_t)(g0 + i);
        lds_box[i] = s[0];
        lds_box[cap + i] = s[1];
        lds_box[2 * cap + i] = s[2];
        lds_box[3 * cap + i] = s[3];
    }
    const int K = (G + 63) >> 6;                  // <= 64
    unsigned long long ign = 0, taken = 0;
    int n_real = 0;
    for (int k = 0; k < K; ++k) {
        const int gi = k * 64 + lane;
        if (gi < G) {
            const double ar = p.gt_area[g0 + gi];
            const bool ig = p.gt_ignore[g0 + gi] != 0 || ar < lo || ar > hi;
            if (ig) ign |= 1ull << k;
            else ++n_real;
        }
    }
    __syncthreads();
    if (ti == 0) {
        for (int m = 32; m >= 1; m >>= 1) n_real += __shfl_xor(n_real, m);
        if (lane == 0) p.npig[(size_t)a * p.B + b] = n_real;
    }
    const double thr = p.iou_thrs[ti];
    uint8_t* __restrict__ out_m = p.matched + ((size_t)a * p.T + ti) * p.Dtot + d0;
    uint8_t* __restrict__ out_i = p.det_ignored + ((size_t)a * p.T + ti) * p.Dtot + d0;

    for (int di = 0; di < D; ++di) {
        const double* dp = p.dt_boxes + 4 * (size_t)(d0 + di);
        const double dx = dp[0], dy = dp[1], dw = dp[2], dh = dp[3];
        const double da = dw * dh, dx2 = dx + dw, dy2 = dy + dh;
        double best_r = thr, best_i = thr;        // per lane: best unmatched real / ignored ground truth with IoU >= thr
        int idx_r = -1, idx_i = -1;               // ascending index inside a lane + replace on >= : the highest index among equal IoUs
        for (int k = 0; k < K; ++k) {
            const int gi = k * 64 + lane;
            if (gi >= G || ((taken >> k) & 1)) continue;
            const double gx = lds_box[gi], gy = lds_box[cap + gi], gw = lds_box[2 * cap + gi], gh = lds_box[3 * cap + gi];
            const double w = fmin(dx2, gx + gw) - fmax(dx, gx);
            const double h = fmin(dy2, gy + gh) - fmax(dy, gy);
            const double inter = fmax(w, 0.0) * fmax(h, 0.0);
            double iou = 0.0;                     // disjoint boxes: 0 / union, or the union <= 0 rule: 0 either way, the division is skipped
            if (inter > 0.0) {
                const double uni = (da + gw * gh) - inter;
                iou = uni > 0.0 ? inter / uni : 0.0;
            }
            if ((ign >> k) & 1) {
                if (iou >= best_i) { best_i = iou; idx_i = gi; }
            } else {
                if (iou >= best_r) { best_r = iou; idx_r = gi; }
            }
        }
        int m = -1;
        bool m_ign = false;
        if (__ballot(idx_r >= 0)) {
            wave_argmax(best_r, idx_r);
            m = idx_r;
        } else if (__ballot(idx_i >= 0)) {        // only when no real ground truth is left for it: the ignored ones, same rule
            wave_argmax(best_i, idx_i);
            m = idx_i;
            m_ign = true;
        }
        if (m >= 0 && lane == (m & 63)) taken |= 1ull << (m >> 6);      // taken for good, ignored or not
        if (lane == 0) {
            out_m[di] = m >= 0;
            out_i[di] = m >= 0 ? m_ign : (p.dt_area[d0 + di] < lo || p.dt_area[d0 + di] > hi);
        }
    }
}

}  // namespace

extern "C" int cdetr_box_iou_xywh(const double* dt, int32_t D, const double* gt, int32_t G, double* iou, void* stream) {
    CDETR_CHECK_ARG(D >= 0 && G >= 0 && (int64_t)D * G < ((int64_t)1 << 40), "cdetr_box_iou_xywh: bad sizes D = %d, G = %d", D, G);
    if (D == 0 || G == 0) return CDETR_OK;
    CDETR_CHECK_ARG(dt && gt && iou, "cdetr_box_iou_xywh: null pointer");
    CDETR_CHECK_ARG((D + 15) / 16 <= 65535, "cdetr_box_iou_xywh: D = %d exceeds 16 x 65535 rows per launch", D);
    hipLaunchKernelGGL(box_iou_kernel, dim3((G + 255) / 256, (D + 15) / 16), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dt, D, gt, G, iou);
    return cdetr_launch_status("cdetr_box_iou_xywh");
}

extern "C" int cdetr_coco_match(const cdetr_coco_match_desc* d, void* stream) {
    CDETR_CHECK_ARG(d != nullptr, "cdetr_coco_match: null descriptor");
    CDETR_CHECK_ARG(d->B > 0 && d->A > 0 && d->T > 0 && d->Gtot >= 0 && d->Dtot >= 0 && d->Gmax >= 0,
                    "cdetr_coco_match: bad sizes B = %d, A = %d, T = %d, Gtot = %d, Dtot = %d, Gmax = %d", d->B, d->A, d->T, d->Gtot, d->Dtot, d->Gmax);
    CDETR_CHECK_ARG(d->gt_off && d->dt_off && d->iou_thrs && d->area_rng && d->npig, "cdetr_coco_match: null offset table / threshold / range / npig pointer");
    CDETR_CHECK_ARG(d->Gtot == 0 || (d->gt_boxes && d->gt_area && d->gt_ignore), "cdetr_coco_match: null ground-truth pointer");
    CDETR_CHECK_ARG(d->Dtot == 0 || (d->dt_boxes && d->dt_area && d->matched && d->det_ignored), "cdetr_coco_match: null detection / output pointer");
    if (d->T > COCO_MAX_T || d->A > 65535) {
        cdetr_set_error("cdetr_coco_match: T = %d thresholds (limit %d) or A = %d ranges (limit 65535) not supported", d->T, COCO_MAX_T, d->A);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (d->Gmax > COCO_MAX_G) {
        cdetr_set_error("cdetr_coco_match: %d ground truths in one image exceed the LDS-resident matcher's capacity (%d)", d->Gmax, COCO_MAX_G);
        return CDETR_ERR_UNSUPPORTED;
    }
    const int cap = d->Gmax > 64 ? (d->Gmax + 63) & ~63 : 64;
    const size_t bytes = (size_t)cap * 4 * sizeof(double);
    if (bytes > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(coco_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        cdetr_set_error("cdetr_coco_match: %zu bytes of LDS for %d ground truths exceed the device limit", bytes, d->Gmax);
        return CDETR_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(coco_match_kernel, dim3(d->B, d->A), dim3(64 * d->T), bytes, reinterpret_cast<hipStream_t>(stream), *d, cap);
    return cdetr_launch_status("cdetr_coco_match");
}
