#pragma clang fp contract(off)
// What the record kernels share (detections.hip, stage1_labels.hip; coco_eval.hip for the IoU alone; nms.hip for the IoU, the score order
// and the sum): a device-resident store takes, per image, wire records and evaluation records (cut at max_det) behind the records of the
// images before it.  Here are the deterministic placement of an image's records, the evaluation record itself, the score key and its sort
// in LDS, the float64 IoU and the host-side check of a store's arguments.
//
// Everything these kernels compute must EQUAL numpy on the host, so a product must never be contracted into an FMA with a later
// operation: the first line switches contraction off from here to the end of every translation unit that includes this header.
#pragma once

#include "common.h"

constexpr int STORE_MAX_B = 65535;        // images per call (the grid)
constexpr int STORE_MAX_CAP = 1 << 30;    // records of one section: an offset + one call's records (65535 x 4096 at most) stays inside int32

// integer sum of `v` over a workgroup of WAVES waves, the same value in every thread; `red` holds one slot per wave.  Ends with a
// barrier-protected read: the caller may reuse `red` after its next __syncthreads().  (Integer addition is order-free; the float
// reductions of the criterion kernels, whose order is part of their contract, are their own.)
template <int WAVES, class T>
__device__ __forceinline__ T block_sum(T v, T* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += red[w];
    return s;
}

// ascending key = descending score, equal scores by ascending query: high half = the inverted image of the score under the
// order-preserving map float -> uint32 (sign bit flipped for positives, all bits for negatives; -0 is made +0 first, the two compare equal)
__device__ __forceinline__ unsigned long long sort_key(float p, int q) {
    if (p == 0.0f) p = 0.0f;
    unsigned u = __float_as_uint(p);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)(~u) << 32) | (unsigned)q;
}

// key[0 .. cnt) ascending, in place, by a workgroup of THREADS threads: bitonic sort over the next power of two, which `key` must hold
// (the padding is ~0, above every sort_key).  Every thread calls this (it holds barriers); the keys must have been written before the
// call by the threads that own them, no barrier needed in between.  Distinct keys: the result is the one sorted order.
template <int THREADS>
__device__ __forceinline__ void sort_keys(unsigned long long* key, int cnt) {
    int npad = 1;
    while (npad < cnt) npad <<= 1;
    for (int i = cnt + threadIdx.x; i < npad; i += THREADS) key[i] = ~0ull;
    __syncthreads();
    for (int k2 = 2; k2 <= npad; k2 <<= 1) {
        for (int j = k2 >> 1; j >= 1; j >>= 1) {
            for (int i = threadIdx.x; i < npad; i += THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = key[i], c = key[l];
                    if ((a > c) == ((i & k2) == 0)) { key[i] = c; key[l] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// where the records of image b of a call land, and whether they fit.  T = the type of the running sums: each kernel keeps the one it
// had (int in cdetr_emit_detections, whose checked capacities keep start + B * Q inside int32; long long in cdetr_emit_pseudo_labels)
template <class T>
struct record_place {
    int start_w, start_e;       // the store's running offsets at `first` (written by the previous call, in stream order)
    T w0, e0;                   // the image's first wire / evaluation record: the start + the counts of the call's images before it
    int cnt, ecnt;              // its wire / evaluation (cut at max_det) records
    bool start_ok, fits_w, fits_e;
    // nothing of an image is written unless both ranges fit
    __device__ bool fits() const { return fits_w && fits_e; }
    // what a misfit ORs into the status word: 4 = the running offsets are outside the store, else 1 = wire records, 2 = evaluation records
    __device__ int status_bits() const { return !start_ok ? 4 : ((fits_w ? 0 : 1) | (fits_e ? 0 : 2)); }
};

// count_of(j) = the wire records of image j of the call (the same in every thread).  Every thread of the workgroup of WAVES waves calls
// this (it holds barriers) and gets the same result; `red`: one slot per wave.  No atomic decides where a record lands.  A count outside
// 0 .. cnt_max never fits.  The next offsets are NOT written here: the two kernels keep their own rules for them.
template <int WAVES, class T, class CountOf>
__device__ __forceinline__ record_place<T> place_records(CountOf count_of, int b, int cnt_max, int max_det, const int* wire_off, const int* eval_off,
                                                         int first, int wire_cap, int eval_cap, T* red) {
    T sw = 0, se = 0;
    for (int j = threadIdx.x; j < b; j += 64 * WAVES) {
        const int c = count_of(j);
        sw += c;
        se += min(c, max_det);
    }
    sw = block_sum<WAVES>(sw, red);
    se = block_sum<WAVES>(se, red);
    record_place<T> r;
    r.start_w = wire_off[first];
    r.start_e = eval_off[first];
    r.cnt = count_of(b);
    r.ecnt = min(r.cnt, max_det);
    r.start_ok = r.start_w >= 0 && r.start_w <= wire_cap && r.start_e >= 0 && r.start_e <= eval_cap;
    r.w0 = r.start_w + sw;
    r.e0 = r.start_e + se;
    r.fits_w = r.start_ok && r.cnt >= 0 && r.cnt <= cnt_max && r.w0 + r.cnt <= wire_cap;
    r.fits_e = r.start_ok && r.e0 + r.ecnt <= eval_cap;
    return r;
}

// evaluation record e, the float64 arrays cdetr_coco_match reads: box [x, y, w, h], area = w * h of the integer sides, score
__device__ __forceinline__ void write_eval_record(double* eval_boxes, double* eval_area, double* eval_score, size_t e, double x, double y, int w,
                                                  int h, double score) {
    double* bo = eval_boxes + 4 * e;
    bo[0] = x;
    bo[1] = y;
    bo[2] = (double)w;
    bo[3] = (double)h;
    eval_area[e] = (double)((long long)w * (long long)h);
    eval_score[e] = score;
}

// coco_ap.box_iou_xywh, one pair, operation by operation: da, ga = w * h; union = (da + ga) - inter; 0 where the union is not positive
__device__ __forceinline__ double iou_xywh(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh) {
    const double da = dw * dh, ga = gw * gh;
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    const double inter = fmax(w, 0.0) * fmax(h, 0.0);
    const double uni = (da + ga) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

// The sizes and the store side of an emit entry's descriptor, checked before any launch in the order the entries always had.  `entry`
// names the entry in the messages, `per_image` / `noun` / `cap` / `wire_what` are its own words for n_per_image (queries or rows of one image,
// at most `limit`), for wire_cap and for its arrays per wire record; `inputs` / `wire_arrays`: its input / per-wire-record pointers are all set.
static inline int check_record_store(const char* entry, const char* per_image, const char* noun, const char* cap, const char* wire_what, int B,
                                     int n_per_image, int limit, int N, int first, int max_det, int wire_cap, int eval_cap, bool inputs,
                                     const void* counts, const void* wire_off, const void* eval_off, const void* status, const void* wire,
                                     bool wire_arrays, const void* eval_boxes, const void* eval_area, const void* eval_score) {
    CDETR_CHECK_ARG(B > 0 && n_per_image > 0 && N > 0 && first >= 0 && max_det >= 0 && wire_cap >= 0 && eval_cap >= 0,
                    "%s: bad sizes B = %d, %s = %d, N = %d, first = %d, max_det = %d, %s = %d, eval_cap = %d", entry, B, per_image, n_per_image, N, first,
                    max_det, cap, wire_cap, eval_cap);
    if (n_per_image > limit || B > STORE_MAX_B) {
        cdetr_set_error("%s: %s = %d %s (limit %d) or B = %d images per call (limit %d) not supported", entry, per_image, n_per_image, noun, limit, B,
                        STORE_MAX_B);
        return CDETR_ERR_UNSUPPORTED;
    }
    CDETR_CHECK_ARG((int64_t)first + B <= N, "%s: images %d .. %d do not fit a store of N = %d", entry, first, first + B - 1, N);
    CDETR_CHECK_ARG(wire_cap <= STORE_MAX_CAP && eval_cap <= STORE_MAX_CAP, "%s: capacities %d / %d exceed %d records", entry, wire_cap, eval_cap,
                    STORE_MAX_CAP);
    CDETR_CHECK_ARG(inputs, "%s: null input pointer", entry);
    CDETR_CHECK_ARG(counts && wire_off && eval_off && status, "%s: null counts / offset table / status pointer", entry);
    CDETR_CHECK_ARG(wire_cap == 0 || wire_arrays, "%s: null %s pointer", entry, wire_what);
    CDETR_CHECK_ARG(eval_cap == 0 || (eval_boxes && eval_area && eval_score), "%s: null evaluation-record pointer", entry);
    CDETR_CHECK_ARG((reinterpret_cast<uintptr_t>(wire) & 15) == 0, "%s: wire records must be 16-byte aligned", entry);
    return CDETR_OK;
}
