// Why a detection failed, on the device (counting_detr_amd/error_report.py states the rule in numpy and is the checker; infer.py
// --error_report): the single-class TIDE breakdown -- duplicate, localisation, background, missed -- of a whole split in one launch.
//
// cdetr_coco_errors : one workgroup of 16 waves per image.  The image's ground-truth boxes sit in LDS as four planes (x | y | w | h) as in
//   cdetr_coco_match, beside the matched detection of every ground truth (int32) and the hand-over buffers of one chunk of 64 detections.
//     wave 0       : COCOeval's greedy match at iou_fg, serial in the detections exactly as coco_match_kernel walks them (lanes over the
//                    ground truths, a 64-bit taken-mask per lane, a wave arg-max; ignored ground truths only when no real one is left).
//     waves 1 .. 15: the overlaps, which are not serial.  Wave w owns the ground truths of the 64-blocks k = w - 1, w + 14, ... (five at the
//                    most), one per lane and block: for every detection it forms the IoUs with its own ground truths ONCE, keeps each ground
//                    truth's running maximum in registers (replace on >: the lowest detection among equal IoUs) and reduces the detection's
//                    best non-ignored ground truth over the wave (the larger IoU, among equal IoUs the higher index).
//     after a chunk: lane c of wave 1 joins the 15 partial arg-maxima of detection c in wave order with the same rule, reads what wave 0 left
//                    for it, and writes the detection's code, ground truth and IoU; the counts are ballots + popcounts; a LOC detection marks
//                    its best ground truth in the register mask of the lane that owns it, one detection after the other.
//   At the end the owners write their ground truths' codes from the matched detections (LDS), the marks (LDS, written once by wave 1) and the
//   maxima (registers).  No atomics; no floating-point value crosses lanes except through the arg-max's compare.
//
// Must agree with numpy BIT FOR BIT: every IoU is records.h's iou_xywh, every decision a float64 compare.  Contraction into FMAs is
// switched off for this translation unit as in coco_eval.hip.
#pragma clang fp contract(off)

#include "records.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int ERR_MAX_G = 4096;           // ground truths per image: 64 lanes x the 64 bits of a lane's masks; 4 x 8 B x 4096 = 128 KiB of LDS
constexpr int ERR_WAVES = 16;
constexpr int ERR_OWNERS = ERR_WAVES - 1; // the waves that own ground truths
constexpr int ERR_SLOTS = 5;              // 64-blocks of ground truths per owner: 15 x 5 >= 64
constexpr int ERR_CHUNK = 64;             // detections handed over at a time: one per lane of wave 1
// what lies behind the planes and the matched detections: part_v | m_iou | marks | part_i | m_idx | m_ign | cnt, every offset a multiple of 16
constexpr size_t ERR_FIXED_BYTES = (size_t)ERR_CHUNK * ERR_OWNERS * 12 + (size_t)ERR_CHUNK * 16 + 64 * 8 + ERR_WAVES * 4 * 4;

enum : uint8_t { DT_TP = 0, DT_IGN = 1, DT_DUP = 2, DT_LOC = 3, DT_BKG = 4, DT_UNUSED = 255 };
enum : uint8_t { GT_HIT = 0, GT_IGN = 1, GT_MISLOC = 2, GT_MISSED = 3 };

// arg-max of the key (iou, index) over the wave: the larger IoU, among equal IoUs the larger index (coco_eval.hip's).  Every lane ends with
// the same pair.
__device__ __forceinline__ void err_wave_argmax(double& v, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (ov > v || (ov == v && oi > i)) { v = ov; i = oi; }
    }
}

__device__ __forceinline__ int err_wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(64 * ERR_WAVES) void coco_errors_kernel(
    const double* __restrict__ gt_boxes, const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_ignore, const int32_t* __restrict__ gt_off,
    const double* __restrict__ dt_boxes, const double* __restrict__ dt_area, const int32_t* __restrict__ dt_off, const int32_t* __restrict__ dt_cnt,
    int Gtot, int Dtot, double iou_fg, double iou_bg, double area_lo, double area_hi, uint8_t* __restrict__ dt_code, int32_t* __restrict__ dt_gt,
    double* __restrict__ dt_iou, uint8_t* __restrict__ gt_code, int32_t* __restrict__ gt_dt, double* __restrict__ gt_iou, int32_t* __restrict__ counts,
    int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char err_lds[];
    double* const box = reinterpret_cast<double*>(err_lds);                               // [4][cap]
    int* const gtm = reinterpret_cast<int*>(err_lds + (size_t)32 * cap);                  // [cap]: the detection a ground truth was matched to, -1
    unsigned char* const fx = err_lds + (size_t)36 * cap;                                 // cap is a multiple of 64
    double* const part_v = reinterpret_cast<double*>(fx);                                 // [CHUNK][OWNERS]
    double* const m_iou = part_v + ERR_CHUNK * ERR_OWNERS;                                // [CHUNK]
    unsigned long long* const marks = reinterpret_cast<unsigned long long*>(m_iou + ERR_CHUNK);      // [64]: lane l, bit k = ground truth 64 k + l
    int* const part_i = reinterpret_cast<int*>(marks + 64);                               // [CHUNK][OWNERS]
    int* const m_idx = part_i + ERR_CHUNK * ERR_OWNERS;                                   // [CHUNK]
    int* const m_ign = m_idx + ERR_CHUNK;                                                 // [CHUNK]
    int* const cnt = m_ign + ERR_CHUNK;                                                   // [WAVES][4]

    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = gt_off[b], g1 = gt_off[b + 1], d0 = dt_off[b], d1 = dt_off[b + 1];
    int G = g1 - g0, D = d1 - d0;
    // an offset table that does not describe this launch's buffers: the segment counts as empty and nothing of it is read or written
    if (g0 < 0 || G < 0 || g1 > Gtot || G > cap) G = 0;
    if (d0 < 0 || D < 0 || d1 > Dtot) D = 0;
    int n = D;
    if (dt_cnt != nullptr) n = min(D, max(dt_cnt[b], 0));
    const int K = (G + 63) >> 6;                  // <= 64

    for (int i = threadIdx.x; i < G; i += blockDim.x) {
        const double* s = gt_boxes + 4 * (size_t)(g0 + i);
        box[i] = s[0];
        box[cap + i] = s[1];
        box[2 * cap + i] = s[2];
        box[3 * cap + i] = s[3];
        gtm[i] = -1;
    }
    for (int i = n + (int)threadIdx.x; i < D; i += blockDim.x) {      // beyond the prefix
        dt_code[(size_t)d0 + i] = DT_UNUSED;
        dt_gt[(size_t)d0 + i] = -1;
        dt_iou[(size_t)d0 + i] = 0.0;
    }
    // wave 0: every ground truth's ignore bit and the taken bits; an owner: the ignore flags of its own slots
    unsigned long long ign = 0, taken = 0;
    bool ig[ERR_SLOTS];
    double gbest[ERR_SLOTS];
    int gbd[ERR_SLOTS];
#pragma unroll
    for (int j = 0; j < ERR_SLOTS; ++j) {
        ig[j] = false;
        gbest[j] = 0.0;
        gbd[j] = -1;
    }
    if (wave == 0) {
        for (int k = 0; k < K; ++k) {
            const int gi = k * 64 + lane;
            if (gi < G) {
                const double ar = gt_area[g0 + gi];
                if (gt_ignore[g0 + gi] != 0 || ar < area_lo || ar > area_hi) ign |= 1ull << k;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < ERR_SLOTS; ++j) {
            const int gi = (wave - 1 + ERR_OWNERS * j) * 64 + lane;
            if (gi < G) {
                const double ar = gt_area[g0 + gi];
                ig[j] = gt_ignore[g0 + gi] != 0 || ar < area_lo || ar > area_hi;
            }
        }
    }
    unsigned long long mark = 0;                  // wave 1: the MISLOC marks of the ground truths 64 k + lane
    int c_tp = 0, c_ign = 0, c_dup = 0, c_loc = 0, c_bkg = 0;
    __syncthreads();

    for (int c0 = 0; c0 < n; c0 += ERR_CHUNK) {
        const int cn = min(ERR_CHUNK, n - c0);
        if (wave == 0) {
            for (int c = 0; c < cn; ++c) {
                const int di = c0 + c;
                const double* dp = dt_boxes + 4 * (size_t)(d0 + di);
                const double dx = dp[0], dy = dp[1], dw = dp[2], dh = dp[3];
                double best_r = iou_fg, best_i = iou_fg;      // per lane: best unmatched real / ignored ground truth with IoU >= iou_fg
                int idx_r = -1, idx_i = -1;                   // ascending index inside a lane + replace on >= : the highest index among equal IoUs
                for (int k = 0; k < K; ++k) {
                    const int gi = k * 64 + lane;
                    if (gi >= G || ((taken >> k) & 1)) continue;
                    const double iou = iou_xywh(dx, dy, dw, dh, box[gi], box[cap + gi], box[2 * cap + gi], box[3 * cap + gi]);
                    if ((ign >> k) & 1) {
                        if (iou >= best_i) { best_i = iou; idx_i = gi; }
                    } else {
                        if (iou >= best_r) { best_r = iou; idx_r = gi; }
                    }
                }
                int m = -1;
                bool mi = false;
                double mv = 0.0;
                if (__ballot(idx_r >= 0)) {
                    err_wave_argmax(best_r, idx_r);
                    m = idx_r;
                    mv = best_r;
                } else if (__ballot(idx_i >= 0)) {            // only when no real ground truth is left for it: the ignored ones, same rule
                    err_wave_argmax(best_i, idx_i);
                    m = idx_i;
                    mv = best_i;
                    mi = true;
                }
                if (m >= 0 && lane == (m & 63)) taken |= 1ull << (m >> 6);
                if (lane == 0) {
                    m_idx[c] = m;
                    m_ign[c] = mi ? 1 : 0;
                    m_iou[c] = mv;
                    if (m >= 0) gtm[m] = di;
                }
            }
        } else {
            for (int c = 0; c < cn; ++c) {
                const int di = c0 + c;
                const double* dp = dt_boxes + 4 * (size_t)(d0 + di);
                const double dx = dp[0], dy = dp[1], dw = dp[2], dh = dp[3];
                double v = 0.0;                               // the detection's best non-ignored ground truth among the wave's own: an IoU > 0
                int vi = -1;
#pragma unroll
                for (int j = 0; j < ERR_SLOTS; ++j) {
                    const int gi = (wave - 1 + ERR_OWNERS * j) * 64 + lane;
                    if (gi < G) {
                        const double iou = iou_xywh(dx, dy, dw, dh, box[gi], box[cap + gi], box[2 * cap + gi], box[3 * cap + gi]);
                        if (iou > gbest[j]) { gbest[j] = iou; gbd[j] = di; }
                        if (!ig[j] && iou > 0.0 && iou >= v) { v = iou; vi = gi; }
                    }
                }
                err_wave_argmax(v, vi);
                if (lane == 0) {
                    part_v[c * ERR_OWNERS + wave - 1] = v;
                    part_i[c * ERR_OWNERS + wave - 1] = vi;
                }
            }
        }
        __syncthreads();
        if (wave == 1) {
            const bool used = lane < cn;
            uint8_t code = DT_UNUSED;
            int bgt = -1;
            if (used) {
                const int di = c0 + lane;
                double bv = 0.0;
                for (int w = 0; w < ERR_OWNERS; ++w) {
                    const double pv = part_v[lane * ERR_OWNERS + w];
                    const int pi = part_i[lane * ERR_OWNERS + w];
                    if (pv > bv || (pv == bv && pi > bgt)) { bv = pv; bgt = pi; }
                }
                const int m = m_idx[lane];
                const double ar = dt_area[(size_t)d0 + di];
                if (m >= 0) code = m_ign[lane] ? DT_IGN : DT_TP;
                else if (ar < area_lo || ar > area_hi) code = DT_IGN;
                else if (bv >= iou_fg) code = DT_DUP;
                else if (bv >= iou_bg) code = DT_LOC;
                else code = DT_BKG;
                dt_code[(size_t)d0 + di] = code;
                dt_gt[(size_t)d0 + di] = m >= 0 ? m : bgt;
                dt_iou[(size_t)d0 + di] = m >= 0 ? m_iou[lane] : bv;
            }
            c_tp += __popcll(__ballot(code == DT_TP));
            c_ign += __popcll(__ballot(code == DT_IGN));
            c_dup += __popcll(__ballot(code == DT_DUP));
            c_bkg += __popcll(__ballot(code == DT_BKG));
            unsigned long long loc = __ballot(code == DT_LOC);
            c_loc += __popcll(loc);
            while (loc) {                                     // uniform: one LOC detection after the other marks its best ground truth
                const int src = __ffsll((long long)loc) - 1;
                loc &= loc - 1;
                const int g = __shfl(bgt, src);
                if (g >= 0 && lane == (g & 63)) mark |= 1ull << (g >> 6);
            }
        }
        __syncthreads();
    }
    if (wave == 1) marks[lane] = mark;
    __syncthreads();

    int n_hit = 0, n_ign = 0, n_mis = 0, n_miss = 0;
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < ERR_SLOTS; ++j) {
            const int k = wave - 1 + ERR_OWNERS * j;
            const int gi = k * 64 + lane;
            if (gi < G) {
                const int t = gtm[gi];
                uint8_t code;
                if (ig[j]) { code = GT_IGN; ++n_ign; }
                else if (t >= 0) { code = GT_HIT; ++n_hit; }
                else if ((marks[lane] >> k) & 1) { code = GT_MISLOC; ++n_mis; }
                else { code = GT_MISSED; ++n_miss; }
                gt_code[(size_t)g0 + gi] = code;
                gt_dt[(size_t)g0 + gi] = code == GT_HIT ? t : gbd[j];
                gt_iou[(size_t)g0 + gi] = gbest[j];
            }
        }
    }
    n_hit = err_wave_sum(n_hit);
    n_ign = err_wave_sum(n_ign);
    n_mis = err_wave_sum(n_mis);
    n_miss = err_wave_sum(n_miss);
    if (lane == 0) {
        cnt[wave * 4] = n_hit;
        cnt[wave * 4 + 1] = n_ign;
        cnt[wave * 4 + 2] = n_mis;
        cnt[wave * 4 + 3] = n_miss;
    }
    __syncthreads();
    if (threadIdx.x == 64) {                      // lane 0 of wave 1, which holds the detections' counts
        int s[4] = {0, 0, 0, 0};
        for (int w = 0; w < ERR_WAVES; ++w)
            for (int q = 0; q < 4; ++q) s[q] += cnt[w * 4 + q];
        int32_t* o = counts + (size_t)b * 9;
        o[0] = c_tp; o[1] = c_ign; o[2] = c_dup; o[3] = c_loc; o[4] = c_bkg;
        o[5] = s[0]; o[6] = s[1]; o[7] = s[2]; o[8] = s[3];
    }
}

}  // namespace

extern "C" int cdetr_coco_errors(const double* gt_boxes, const double* gt_area, const uint8_t* gt_ignore, const int32_t* gt_off,
                                 const double* dt_boxes, const double* dt_area, const int32_t* dt_off, const int32_t* dt_cnt, int32_t B,
                                 int32_t Gtot, int32_t Dtot, int32_t Gmax, double iou_fg, double iou_bg, double area_lo, double area_hi,
                                 uint8_t* dt_code, int32_t* dt_gt, double* dt_iou, uint8_t* gt_code, int32_t* gt_dt, double* gt_iou,
                                 int32_t* counts, void* stream) {
    CDETR_CHECK_ARG(B >= 0 && Gtot >= 0 && Dtot >= 0 && Gmax >= 0, "cdetr_coco_errors: bad sizes B = %d, Gtot = %d, Dtot = %d, Gmax = %d", B, Gtot,
                    Dtot, Gmax);
    CDETR_CHECK_ARG(iou_fg == iou_fg && iou_bg == iou_bg && area_lo == area_lo && area_hi == area_hi,
                    "cdetr_coco_errors: a NaN among iou_fg = %g, iou_bg = %g, area_lo = %g, area_hi = %g", iou_fg, iou_bg, area_lo, area_hi);
    if (Gmax > ERR_MAX_G) {
        cdetr_set_error("cdetr_coco_errors: %d ground truths in one image exceed the LDS-resident capacity (%d)", Gmax, ERR_MAX_G);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (B == 0) return CDETR_OK;                  // no image: the outputs are empty
    CDETR_CHECK_ARG(gt_off && dt_off && counts, "cdetr_coco_errors: null offset table / counts pointer");
    CDETR_CHECK_ARG(Gtot == 0 || (gt_boxes && gt_area && gt_ignore && gt_code && gt_dt && gt_iou), "cdetr_coco_errors: null ground-truth / output pointer");
    CDETR_CHECK_ARG(Dtot == 0 || (dt_boxes && dt_area && dt_code && dt_gt && dt_iou), "cdetr_coco_errors: null detection / output pointer");
    const int cap = Gmax > 64 ? (Gmax + 63) & ~63 : 64;
    const size_t bytes = (size_t)cap * 36 + ERR_FIXED_BYTES;
    if (bytes > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(coco_errors_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        cdetr_set_error("cdetr_coco_errors: %zu bytes of LDS for %d ground truths exceed the device limit", bytes, Gmax);
        return CDETR_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(coco_errors_kernel, dim3(B), dim3(64 * ERR_WAVES), bytes, reinterpret_cast<hipStream_t>(stream), gt_boxes, gt_area, gt_ignore,
                       gt_off, dt_boxes, dt_area, dt_off, dt_cnt, Gtot, Dtot, iou_fg, iou_bg, area_lo, area_hi, dt_code, dt_gt, dt_iou, gt_code, gt_dt,
                       gt_iou, counts, cap);
    return cdetr_launch_status("cdetr_coco_errors");
}
