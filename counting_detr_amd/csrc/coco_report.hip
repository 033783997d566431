// Per-image evaluation statistics from the flags cdetr_coco_match left in device memory (counting_detr_amd/coco_ap.py: stats_from_flags is
// the host restatement and the checker; infer.py --image_report).
//
// cdetr_coco_image_stats : for every (area range, image, IoU threshold) the true / false positives of the image's first `cut` detections at
//   each maxDets cut, and the image's OWN average precision -- coco_ap._sample on the image's own list: cumulative counts, recall and
//   precision, the envelope from the right, the 101-point sampling, the ordered sum.  One workgroup per (image, area range), one wave per
//   IoU threshold, as cdetr_coco_match is laid out; a wave walks its image's detections in chunks of 64, one detection per lane:
//     pass 1, forward : ballots of `matched & !ignored` / `!matched & !ignored`, popcounts -> the running counts; lane m takes the counts at
//                       cut m when its index falls into the chunk.  The totals are what pass 2 starts from.
//     pass 2, backward: the chunk's counts again (total minus what lies behind), precision per lane, a suffix maximum over the lanes joined
//                       with the maximum of the chunks behind = the envelope.  Recall is monotone, so a recall sample's index lies in the
//                       one chunk whose first and last recall straddle it: the lane that owns the sample searches the chunk's ballot mask
//                       (6 steps) and takes the envelope of the lane it finds.
//   The samples go to LDS and ONE lane adds them in index order.  No atomics; nothing in floating point crosses lanes except through max.
//
// Must agree with numpy BIT FOR BIT: every operation is an IEEE double divide, add of two integers-valued doubles (+ eps), compare or max,
// or an integer count.  Contraction into FMAs is switched off for this translation unit as in coco_eval.hip.
#pragma clang fp contract(off)

#include "records.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int REPORT_MAX_T = 16;          // IoU thresholds = waves of a workgroup
constexpr int REPORT_MAX_M = 64;          // maxDets cuts: one lane each
constexpr int REPORT_MAX_R = 256;         // recall samples: lane l owns l, l + 64, l + 128, l + 192
constexpr int REPORT_RK = REPORT_MAX_R / 64;

__device__ __forceinline__ unsigned long long upto(int lane) {        // bits 0 .. lane
    return lane >= 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
}

__global__ __launch_bounds__(64 * REPORT_MAX_T) void coco_image_stats_kernel(
    const uint8_t* __restrict__ matched, const uint8_t* __restrict__ det_ignored, const int32_t* __restrict__ dt_off,
    const int32_t* __restrict__ dt_cnt, const int32_t* __restrict__ npig, const int32_t* __restrict__ cuts, const double* __restrict__ rec_thrs,
    int B, int T, int Dtot, int M, int R, int32_t* __restrict__ tp, int32_t* __restrict__ fp, double* __restrict__ ap) {
    __shared__ double q_lds[REPORT_MAX_T * REPORT_MAX_R];
    const int b = blockIdx.x, a = blockIdx.y;
    const int lane = threadIdx.x & 63, ti = threadIdx.x >> 6;
    const int d0 = dt_off[b], d1 = dt_off[b + 1];
    int n = d1 - d0;
    if (d0 < 0 || n < 0 || d1 > Dtot) n = 0;      // an offset table that does not describe the flags: the image counts as empty, nothing is read
    if (dt_cnt != nullptr) n = min(n, max(dt_cnt[b], 0));
    const int np = npig[(size_t)a * B + b];
    const size_t row = ((size_t)a * T + ti) * (size_t)Dtot + (size_t)(n > 0 ? d0 : 0);
    const uint8_t* __restrict__ mrow = matched + row;
    const uint8_t* __restrict__ irow = det_ignored + row;
    const size_t cell = ((size_t)a * B + b) * T + ti;
    const unsigned long long le = upto(lane);

    // ---- pass 1: totals, and the counts at the cuts (lane m = cut m)
    const int cut_len = lane < M ? min(max(cuts[lane], 0), n) : 0;        // detections the cut keeps
    int run_tp = 0, run_fp = 0, cut_tp = 0, cut_fp = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const bool valid = i < n;
        const bool m = valid && mrow[i] != 0, g = valid && irow[i] != 0;
        const unsigned long long tpm = __ballot(valid && m && !g), fpm = __ballot(valid && !m && !g);
        const int c = cut_len - 1 - c0;                                   // the cut's last detection, as a lane of this chunk
        if (c >= 0 && c < 64) {
            cut_tp = run_tp + __popcll(tpm & upto(c));
            cut_fp = run_fp + __popcll(fpm & upto(c));
        }
        run_tp += __popcll(tpm);
        run_fp += __popcll(fpm);
    }
    if (lane < M) {
        tp[cell * M + lane] = cut_tp;
        fp[cell * M + lane] = cut_fp;
    }

    // ---- pass 2: envelope and samples, from the last chunk to the first
    double thr[REPORT_RK], q[REPORT_RK];
#pragma unroll
    for (int k = 0; k < REPORT_RK; ++k) {
        const int r = lane + 64 * k;
        thr[k] = r < R ? rec_thrs[r] : 0.0;
        q[k] = 0.0;
    }
    if (np > 0 && n > 0) {
        const double dn = (double)np;
        const double eps = 2.220446049250313e-16;                         // numpy.spacing(1) = 2^-52
        int end_tp = run_tp, end_fp = run_fp;                             // counts up to the end of the chunk at hand
        double carry = 0.0;                                               // largest precision behind the chunk (a precision is never negative)
        for (int c0 = (n - 1) & ~63; c0 >= 0; c0 -= 64) {
            const int i = c0 + lane;
            const bool valid = i < n;
            const bool m = valid && mrow[i] != 0, g = valid && irow[i] != 0;
            const unsigned long long tpm = __ballot(valid && m && !g), fpm = __ballot(valid && !m && !g);
            const int base_tp = end_tp - __popcll(tpm), base_fp = end_fp - __popcll(fpm);
            const int ctp = base_tp + __popcll(tpm & le), cfp = base_fp + __popcll(fpm & le);
            double env = valid ? (double)ctp / (((double)cfp + (double)ctp) + eps) : 0.0;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {                            // suffix maximum over the lanes
                const double o = __shfl_down(env, s);
                if (lane + s < 64) env = fmax(env, o);
            }
            env = fmax(env, carry);
            carry = __shfl(env, 0);
            const double rc_end = (double)end_tp / dn, rc_before = (double)base_tp / dn;
#pragma unroll
            for (int k = 0; k < REPORT_RK; ++k) {
                if (64 * k >= R) break;                                   // uniform
                const bool mine = lane + 64 * k < R && rc_end >= thr[k] && (c0 == 0 || rc_before < thr[k]);
                if (__ballot(mine) == 0) continue;                        // uniform: no sample of this group lands in the chunk
                int lo = 0, hi = 63;                                      // first lane whose recall reaches the sample (lane 63 does, when `mine`)
                while (lo < hi) {                                         // six steps in every lane: the shuffle below is taken by the whole wave
                    const int mid = (lo + hi) >> 1;
                    if ((double)(base_tp + __popcll(tpm & upto(mid))) / dn >= thr[k]) hi = mid;
                    else lo = mid + 1;
                }
                const double v = __shfl(env, lo);
                if (mine) q[k] = v;
            }
            end_tp = base_tp;
            end_fp = base_fp;
        }
    }
#pragma unroll
    for (int k = 0; k < REPORT_RK; ++k) {
        const int r = lane + 64 * k;
        if (r < R) q_lds[ti * REPORT_MAX_R + r] = q[k];
    }
    __syncthreads();
    if (lane == 0) {
        double out = -1.0;
        if (np > 0) {
            double s = q_lds[ti * REPORT_MAX_R];
            for (int r = 1; r < R; ++r) s = s + q_lds[ti * REPORT_MAX_R + r];      // ((q0 + q1) + q2) + ...: numpy.cumsum's order
            out = s / (double)R;
        }
        ap[cell] = out;
    }
}

}  // namespace

extern "C" int cdetr_coco_image_stats(const uint8_t* matched, const uint8_t* det_ignored, const int32_t* dt_off, const int32_t* dt_cnt,
                                      const int32_t* npig, const int32_t* cuts, const double* rec_thrs, int32_t B, int32_t A, int32_t T,
                                      int32_t Dtot, int32_t M, int32_t R, int32_t* tp, int32_t* fp, double* ap, void* stream) {
    CDETR_CHECK_ARG(B >= 0 && A > 0 && T > 0 && Dtot >= 0 && M > 0 && R > 0,
                    "cdetr_coco_image_stats: bad sizes B = %d, A = %d, T = %d, Dtot = %d, M = %d, R = %d", B, A, T, Dtot, M, R);
    if (T > REPORT_MAX_T || M > REPORT_MAX_M || R > REPORT_MAX_R || A > 65535) {
        cdetr_set_error("cdetr_coco_image_stats: T = %d thresholds (limit %d), M = %d cuts (limit %d), R = %d recall samples (limit %d) or "
                        "A = %d ranges (limit 65535) not supported", T, REPORT_MAX_T, M, REPORT_MAX_M, R, REPORT_MAX_R, A);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (B == 0) return CDETR_OK;                  // no image: the outputs are empty
    CDETR_CHECK_ARG(dt_off && npig && cuts && rec_thrs && tp && fp && ap, "cdetr_coco_image_stats: null offset table / npig / cuts / thresholds / output pointer");
    CDETR_CHECK_ARG(Dtot == 0 || (matched && det_ignored), "cdetr_coco_image_stats: null flag pointer");
    hipLaunchKernelGGL(coco_image_stats_kernel, dim3(B, A), dim3(64 * T), 0, reinterpret_cast<hipStream_t>(stream), matched, det_ignored, dt_off,
                       dt_cnt, npig, cuts, rec_thrs, B, T, Dtot, M, R, tp, fp, ap);
    return cdetr_launch_status("cdetr_coco_image_stats");
}
