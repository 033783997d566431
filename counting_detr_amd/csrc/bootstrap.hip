// Bootstrap replicates over images, for the counting metrics and box AP (counting_detr_amd/bootstrap.py states the rule in numpy and is the
// checker; infer.py / main.py --bootstrap R).  A replicate r draws N images with replacement from a counter-based integer generator; the
// workgroup that owns the replicate builds the multiplicities m[0 .. N) in LDS (threads hash their j and add into LDS integer counters:
// integer adds commute, the table does not depend on their order) and accumulates every image / detection ONCE with weight m.
//
// cdetr_bootstrap_counts : one workgroup per replicate; lane c of the first wave owns count column c and adds, in image order,
//   S1 += m err, S2 += m err^2 (int64) and Sn += m (err / gt), Ss += m (err^2 / gt) (float64, a term 0 where gt == 0).
// cdetr_bootstrap_gather : the flags cdetr_coco_match left in device memory -> one 32-bit word per (area range, merged position): bit t = true
//   positive at IoU threshold t, bit 16 + t = false positive.  Run once per matching; the replicates then stream 8 bytes per position.
// cdetr_bootstrap_ap     : grid (replicate, area range), one wave per IoU threshold, as cdetr_coco_image_stats is laid out.  A wave walks the
//   merged list in chunks of 64 positions, one position per lane, weight = m[image of the position]:
//     pass 1, forward : the weighted totals of tp / fp (integer sums).
//     pass 2, backward: the chunk's weighted inclusive prefix sums (wave scan, the total minus what lies behind as the carry), precision per
//                       lane, a suffix maximum over the lanes joined with the maximum of the chunks behind = the envelope.  Recall is
//                       monotone, so a recall sample's index lies in the one chunk whose first and last recall straddle it: the lane that
//                       owns the sample searches the chunk (6 steps) and takes the envelope of the lane it finds.
//   A position of weight 0 repeats the counts of the position before it (precision 0 at the head of the list): it never changes a maximum,
//   which is why it need not be removed.  No atomics outside LDS; nothing in floating point crosses lanes except through max.
//
// Must agree with numpy BIT FOR BIT: the only floating-point operations are the two IEEE double divisions of recall and precision (after one
// add of integer-valued doubles and eps), compares and max, and the products and ordered sums of Sn / Ss.  Contraction is off.
#pragma clang fp contract(off)

#include "records.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int BOOT_MAX_N = 16384;         // images: m is N int32 in LDS, 64 KB
constexpr int BOOT_MAX_R = 10000;         // replicates of one call
constexpr int BOOT_T = 10;                // IoU thresholds = waves of an AP workgroup = bits of half a flag word
constexpr int BOOT_MAX_TC = 32;           // count columns: one lane each
constexpr int BOOT_MAX_REC = 128;         // recall samples: lane l owns l and l + 64
constexpr int BOOT_COUNT_THREADS = 256;

__device__ __forceinline__ uint32_t draw(uint64_t seed_mul, uint32_t r, uint32_t j, uint32_t N) {
    uint64_t x = seed_mul ^ (((uint64_t)r << 32) | (uint64_t)j);
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)(((x >> 32) * (uint64_t)N) >> 32);       // < N
}

// m[0 .. N) of replicate r into LDS: the given table's row, or the draws.  Ends with a barrier.
__device__ __forceinline__ void build_multiplicities(int* m, const int32_t* __restrict__ mult_row, uint64_t seed, uint32_t r, int N) {
    for (int i = threadIdx.x; i < N; i += blockDim.x) m[i] = mult_row != nullptr ? min(max(mult_row[i], 0), BOOT_MAX_N) : 0;
    __syncthreads();
    if (mult_row == nullptr) {
        const uint64_t seed_mul = seed * 0x9E3779B97F4A7C15ull;
        for (int j = threadIdx.x; j < N; j += blockDim.x) atomicAdd(&m[draw(seed_mul, r, (uint32_t)j, (uint32_t)N)], 1);
        __syncthreads();
    }
}

__global__ __launch_bounds__(BOOT_COUNT_THREADS) void bootstrap_counts_kernel(
    const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, int ld, const int32_t* __restrict__ mult, uint64_t seed, int r0, int N,
    int Tc, int64_t* __restrict__ S, double* __restrict__ F) {
    extern __shared__ int m_lds[];
    const int rb = blockIdx.x;
    build_multiplicities(m_lds, mult != nullptr ? mult + (size_t)rb * N : nullptr, seed, (uint32_t)(r0 + rb), N);
    const int c = threadIdx.x;
    if (c >= Tc) return;
    long long s1 = 0, s2 = 0;
    double sn = 0.0, ss = 0.0;
    for (int i = 0; i < N; ++i) {
        const long long w = m_lds[i];
        const int g = gt[i];
        long long e = (long long)g - (long long)pred[(size_t)i * ld + c];
        e = e < 0 ? -e : e;
        const long long e2 = e * e;
        s1 += w * e;
        s2 += w * e2;
        if (g != 0) {
            const double dg = (double)g, dw = (double)w;
            const double tn = dw * ((double)e / dg), ts = dw * ((double)e2 / dg);
            sn = sn + tn;
            ss = ss + ts;
        }
    }
    const size_t cell = ((size_t)rb * Tc + c) * 2;
    S[cell] = s1;
    S[cell + 1] = s2;
    F[cell] = sn;
    F[cell + 1] = ss;
}

__global__ __launch_bounds__(256) void bootstrap_gather_kernel(const uint8_t* __restrict__ matched, const uint8_t* __restrict__ det_ignored,
                                                                 const int32_t* __restrict__ order, int T, int Dtot, int P,
                                                                 uint32_t* __restrict__ words) {
    const int p = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
    if (p >= P) return;
    const int d = order[p];
    uint32_t w = 0;
    if (d >= 0 && d < Dtot) {                       // an order that does not describe the flags: the position counts as ignored, nothing is read
        for (int t = 0; t < T; ++t) {
            const size_t at = ((size_t)a * T + t) * (size_t)Dtot + (size_t)d;
            const bool mt = matched[at] != 0, ig = det_ignored[at] != 0;
            w |= (uint32_t)(mt && !ig) << t;
            w |= (uint32_t)(!mt && !ig) << (16 + t);
        }
    }
    words[(size_t)a * P + p] = w;
}

__device__ __forceinline__ int scan_inclusive(int v, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(v, s);
        if (lane >= s) v += o;
    }
    return v;
}

__global__ __launch_bounds__(64 * BOOT_T) void bootstrap_ap_kernel(
    const uint32_t* __restrict__ words, const int32_t* __restrict__ image, const int32_t* __restrict__ npig, const int32_t* __restrict__ mult,
    const double* __restrict__ rec_thrs, uint64_t seed, int r0, int N, int P, int A, int R, double eps, double* __restrict__ precision) {
    extern __shared__ int m_lds[];
    const int rb = blockIdx.x, a = blockIdx.y;
    const int lane = threadIdx.x & 63, ti = threadIdx.x >> 6;
    build_multiplicities(m_lds, mult != nullptr ? mult + (size_t)rb * N : nullptr, seed, (uint32_t)(r0 + rb), N);

    long long np = 0;                                                     // npig of the replicate: every wave forms it for itself
    for (int i = lane; i < N; i += 64) np += (long long)m_lds[i] * (long long)npig[(size_t)a * N + i];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) np += __shfl_xor(np, s);

    const uint32_t* __restrict__ wrow = words + (size_t)a * P;
    const uint32_t tbit = 1u << ti, fbit = 1u << (16 + ti);
    double thr[2], q[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int r = lane + 64 * k;
        thr[k] = r < R ? rec_thrs[r] : 0.0;
        q[k] = np > 0 ? 0.0 : -1.0;
    }
    if (np > 0 && P > 0) {
        // ---- pass 1: the weighted totals
        long long end_tp = 0, end_fp = 0;
        for (int c0 = 0; c0 < P; c0 += 64) {
            const int i = c0 + lane;
            if (i < P) {
                const int b = image[i];
                const long long w = (b >= 0 && b < N) ? m_lds[b] : 0;     // an image index outside the split: weight 0
                const uint32_t f = wrow[i];
                end_tp += (f & tbit) ? w : 0;
                end_fp += (f & fbit) ? w : 0;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            end_tp += __shfl_xor(end_tp, s);
            end_fp += __shfl_xor(end_fp, s);
        }
        // ---- pass 2: envelope and samples, from the last chunk to the first
        const double dn = (double)np;
        double carry = 0.0;                                               // largest precision behind the chunk (a precision is never negative)
        for (int c0 = (P - 1) & ~63; c0 >= 0; c0 -= 64) {
            const int i = c0 + lane;
            int w = 0;
            uint32_t f = 0;
            if (i < P) {
                const int b = image[i];
                w = (b >= 0 && b < N) ? m_lds[b] : 0;
                f = wrow[i];
            }
            const int stp = scan_inclusive((f & tbit) ? w : 0, lane), sfp = scan_inclusive((f & fbit) ? w : 0, lane);
            const long long base_tp = end_tp - (long long)__shfl(stp, 63), base_fp = end_fp - (long long)__shfl(sfp, 63);
            const long long ctp = base_tp + stp, cfp = base_fp + sfp;
            double env = w > 0 ? (double)ctp / (((double)cfp + (double)ctp) + eps) : 0.0;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {                            // suffix maximum over the lanes
                const double o = __shfl_down(env, s);
                if (lane + s < 64) env = fmax(env, o);
            }
            env = fmax(env, carry);
            carry = __shfl(env, 0);
            const double rc_end = (double)end_tp / dn, rc_before = (double)base_tp / dn;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (64 * k >= R) break;                                   // uniform
                const bool mine = lane + 64 * k < R && rc_end >= thr[k] && (c0 == 0 || rc_before < thr[k]);
                if (__ballot(mine) == 0) continue;                        // uniform: no sample of this group lands in the chunk
                int lo = 0, hi = 63;                                      // first lane whose recall reaches the sample (lane 63 does, when `mine`)
#pragma unroll
                for (int step = 0; step < 6; ++step) {                    // six steps in every lane: the shuffles are taken by the whole wave
                    const int mid = (lo + hi) >> 1;
                    const int smid = __shfl(stp, mid);
                    if (lo < hi) {
                        if ((double)(base_tp + smid) / dn >= thr[k]) hi = mid;
                        else lo = mid + 1;
                    }
                }
                const double v = __shfl(env, lo);
                if (mine) q[k] = v;
            }
            end_tp = base_tp;
            end_fp = base_fp;
        }
    }
    double* __restrict__ out = precision + (((size_t)rb * A + a) * BOOT_T + ti) * (size_t)R;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int r = lane + 64 * k;
        if (r < R) out[r] = q[k];
    }
}

int set_lds(const void* func, int bytes, const char* what) {
    if (bytes <= 48 * 1024) return CDETR_OK;
    hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        cdetr_set_error("%s: hipFuncSetAttribute(%d): %s", what, bytes, hipGetErrorString(e));
        return CDETR_ERR_LAUNCH;
    }
    return CDETR_OK;
}

int check_replicates(const char* what, int32_t N, int32_t R, int32_t r0) {
    if (N > BOOT_MAX_N || R > BOOT_MAX_R || (int64_t)r0 + R > BOOT_MAX_R) {
        cdetr_set_error("%s: N = %d images (limit %d) or replicates %d .. %d (limit %d) not supported", what, N, BOOT_MAX_N, r0, r0 + R - 1, BOOT_MAX_R);
        return CDETR_ERR_UNSUPPORTED;
    }
    return CDETR_OK;
}

}  // namespace

extern "C" int cdetr_bootstrap_counts(const int32_t* gt, const int32_t* pred, int32_t ld, const int32_t* mult, int64_t seed, int32_t r0, int32_t R,
                                      int32_t N, int32_t Tc, int64_t* S, double* F, void* stream) {
    CDETR_CHECK_ARG(N > 0 && R >= 0 && r0 >= 0 && Tc > 0 && ld >= Tc, "cdetr_bootstrap_counts: bad sizes N = %d, R = %d, r0 = %d, Tc = %d, ld = %d", N, R,
                    r0, Tc, ld);
    if (int rc = check_replicates("cdetr_bootstrap_counts", N, R, r0)) return rc;
    if (Tc > BOOT_MAX_TC) {
        cdetr_set_error("cdetr_bootstrap_counts: Tc = %d count columns (limit %d) not supported", Tc, BOOT_MAX_TC);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (R == 0) return CDETR_OK;
    CDETR_CHECK_ARG(gt && pred && S && F, "cdetr_bootstrap_counts: null count / output pointer");
    const int bytes = N * 4;
    if (int rc = set_lds(reinterpret_cast<const void*>(bootstrap_counts_kernel), bytes, "cdetr_bootstrap_counts")) return rc;
    hipLaunchKernelGGL(bootstrap_counts_kernel, dim3(R), dim3(BOOT_COUNT_THREADS), bytes, reinterpret_cast<hipStream_t>(stream), gt, pred, ld, mult,
                       (uint64_t)seed, r0, N, Tc, S, F);
    return cdetr_launch_status("cdetr_bootstrap_counts");
}

extern "C" int cdetr_bootstrap_gather(const uint8_t* matched, const uint8_t* det_ignored, const int32_t* order, int32_t A, int32_t T, int32_t Dtot,
                                      int32_t P, int32_t* words, void* stream) {
    CDETR_CHECK_ARG(A > 0 && Dtot >= 0 && P >= 0 && A <= 65535, "cdetr_bootstrap_gather: bad sizes A = %d, Dtot = %d, P = %d", A, Dtot, P);
    if (T != BOOT_T) {
        cdetr_set_error("cdetr_bootstrap_gather: T = %d IoU thresholds not supported (the flag word holds exactly %d)", T, BOOT_T);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (P == 0) return CDETR_OK;
    CDETR_CHECK_ARG(order && words && (Dtot == 0 || (matched && det_ignored)), "cdetr_bootstrap_gather: null pointer");
    hipLaunchKernelGGL(bootstrap_gather_kernel, dim3((P + 255) / 256, A), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), matched, det_ignored,
                       order, T, Dtot, P, reinterpret_cast<uint32_t*>(words));
    return cdetr_launch_status("cdetr_bootstrap_gather");
}

extern "C" int cdetr_bootstrap_ap(const int32_t* words, const int32_t* image, const int32_t* npig, const int32_t* mult, const double* rec_thrs,
                                  int64_t seed, int32_t r0, int32_t R, int32_t N, int32_t P, int32_t A, int32_t T, int32_t n_rec, double eps,
                                  double* precision, void* stream) {
    CDETR_CHECK_ARG(N > 0 && R >= 0 && r0 >= 0 && P >= 0 && A > 0 && A <= 65535 && n_rec > 0 && eps >= 0.0,
                    "cdetr_bootstrap_ap: bad sizes N = %d, R = %d, r0 = %d, P = %d, A = %d, n_rec = %d", N, R, r0, P, A, n_rec);
    if (int rc = check_replicates("cdetr_bootstrap_ap", N, R, r0)) return rc;
    if (T != BOOT_T || n_rec > BOOT_MAX_REC) {
        cdetr_set_error("cdetr_bootstrap_ap: T = %d IoU thresholds (exactly %d) or %d recall samples (limit %d) not supported", T, BOOT_T, n_rec,
                        BOOT_MAX_REC);
        return CDETR_ERR_UNSUPPORTED;
    }
    if (R == 0) return CDETR_OK;
    CDETR_CHECK_ARG(npig && rec_thrs && precision && (P == 0 || (words && image)), "cdetr_bootstrap_ap: null pointer");
    const int bytes = N * 4;
    if (int rc = set_lds(reinterpret_cast<const void*>(bootstrap_ap_kernel), bytes, "cdetr_bootstrap_ap")) return rc;
    hipLaunchKernelGGL(bootstrap_ap_kernel, dim3(R, A), dim3(64 * BOOT_T), bytes, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t*>(words), image, npig, mult,
                       rec_thrs, (uint64_t)seed, r0, N, P, A, n_rec, eps, precision);
    return cdetr_launch_status("cdetr_bootstrap_ap");
}
