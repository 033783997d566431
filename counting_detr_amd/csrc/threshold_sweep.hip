// The counting rule at T thresholds from one read of the probabilities (infer.py --sweep_thresholds): for every image of a forwarded batch,
// table[first + b][t] = #{q : prob[b][q] >= thresholds[t]} -- the column of the threshold the run counts with is what the plain loop counts.
//
// cdetr_count_sweep : one workgroup per image.  A lane finds, for each query of its share of the row, k = #{t : p >= thresholds[t]} (fp32
//   compares against thresholds held in LDS; a NaN compares false everywhere, k = 0).  The lanes of a wave then vote bin by bin: one ballot
//   and one popcount per bin, lane j keeps bin j's running count in a register, and after the row every wave adds its T + 1 counts into
//   an LDS histogram.  With ascending thresholds p >= thresholds[t] <=> k > t, so the suffix sums of the histogram are the table's row.
//
// Integer arithmetic only; the LDS atomics add integers (order-free), nothing in global memory is atomic and every table cell has one
// writer: the result is deterministic.  Rows of the table outside first .. first + B - 1 are never addressed.
#include "records.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int SWEEP_MAX_T = 32;           // bins 0 .. T fit the 64 lanes of a wave, one bin per lane
constexpr int SWEEP_THREADS = 256;

__global__ __launch_bounds__(SWEEP_THREADS) void count_sweep_kernel(const float* __restrict__ prob, const float* __restrict__ thresholds, int Q, int T,
                                                                   int* __restrict__ table, int first) {
    __shared__ float thr[SWEEP_MAX_T];
    __shared__ int hist[SWEEP_MAX_T + 1];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    if ((int)threadIdx.x < T) thr[threadIdx.x] = thresholds[threadIdx.x];
    if ((int)threadIdx.x <= T) hist[threadIdx.x] = 0;
    __syncthreads();

    const float* __restrict__ pr = prob + (size_t)b * Q;
    int mine = 0;                                       // lane j <= T: queries of this wave's share that fall into bin j
    for (long long q0 = 0; q0 < Q; q0 += SWEEP_THREADS) {      // uniform trip count: every lane of a wave takes part in every ballot
        const long long q = q0 + threadIdx.x;
        int k = -1;                                     // past the row's end: in no bin
        if (q < Q) {
            const float p = pr[q];
            k = 0;
            for (int t = 0; t < T; ++t) k += p >= thr[t] ? 1 : 0;
        }
        for (int j = 0; j <= T; ++j) {
            const int n = __popcll(__ballot(k == j));
            if (lane == j) mine += n;
        }
    }
    if (lane <= T && mine) atomicAdd(&hist[lane], mine);
    __syncthreads();

    if ((int)threadIdx.x < T) {                         // #{k > t} = the bins above t
        int s = 0;
        for (int j = (int)threadIdx.x + 1; j <= T; ++j) s += hist[j];
        table[((size_t)first + b) * T + threadIdx.x] = s;
    }
}

}  // namespace

extern "C" int cdetr_count_sweep(const float* prob, const float* thresholds, int32_t B, int32_t Q, int32_t T, int32_t* table, int32_t N,
                                 int32_t first, void* stream) {
    CDETR_CHECK_ARG(B > 0 && Q > 0 && T > 0 && N > 0 && first >= 0, "cdetr_count_sweep: bad sizes B = %d, Q = %d, T = %d, N = %d, first = %d", B, Q, T,
                    N, first);
    if (T > SWEEP_MAX_T || B > STORE_MAX_B) {
        cdetr_set_error("cdetr_count_sweep: T = %d thresholds (limit %d) or B = %d images per call (limit %d) not supported", T, SWEEP_MAX_T, B,
                        STORE_MAX_B);
        return CDETR_ERR_UNSUPPORTED;
    }
    CDETR_CHECK_ARG((int64_t)first + B <= N, "cdetr_count_sweep: images %d .. %d do not fit a table of N = %d rows", first, first + B - 1, N);
    CDETR_CHECK_ARG(prob && thresholds && table, "cdetr_count_sweep: null pointer");
    hipLaunchKernelGGL(count_sweep_kernel, dim3(B), dim3(SWEEP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), prob, thresholds, Q, T, table,
                       first);
    return cdetr_launch_status("cdetr_count_sweep");
}
