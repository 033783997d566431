// mha.hip -- fused multi-head self-attention core for the decoder queries (A2/models/transformer.py:337,369-370:
// nn.MultiheadAttention(256, 8) on B x Q = 2 x 300..900 queries, head dim 32, no masks).
//
// The problem is tiny (8 * Q^2 logits per image) and launch/latency bound: the reference path (and round-1's first
// version) spends 5-6 launches forward and ~12 backward on it (scale, bmm, softmax, bmm, permute copies, ...).  Here:
//   mha_fwd_kernel   : o = softmax(scale * q k^T) v, flash-style (online softmax over 64-key LDS tiles), saves the row
//                      log-sum-exp; lane (i, g) owns query i (16 per wave) and every 4th key -> no cross-lane work per key.
//   mha_bwd_q_kernel : dq (lanes own queries) and D_i = <dO_i, O_i>;
//   mha_bwd_kv_kernel: dk, dv (lanes own keys, loop over query tiles) -- no atomics, P recomputed from the saved LSE.
// fp32 VALU throughout (the matrix cores would not be fed by 32-wide heads at this size).
// Layouts: qk [N][L][2E] (q | k), v [N][L][E], o / dO [N][L][E], lse / D [N][nh][L]; E = nh * 32.
//
// Every kernel body is written for the general problem (cdetr_attn_*): q [N][Lq] rows of stride ldq, k / v [N][Lk] rows of strides ldk / ldv
// (head h at columns 32h .. 32h + 31 of a row; image n's rows start at n * L * ld), o / dO [N][Lq][E], lse / D [N][nh][Lq], gradients with
// their own row strides.  cdetr_mha_* is the instance q = qk, k = qk + E (ldq = ldk = 2E), Lq = Lk = L: the same arithmetic, addresses only
// computed differently.  The encoder's self-attention over h*w tokens and the decoder's cross-attention from Q queries to h*w keys of the
// nn.MultiheadAttention variant (A2/models/transformer.py:262-272,393-398) run on the same kernels.
// cdetr_mha_*_lens (stage 1's ragged batches: image n holds lens[n] <= L queries, the rest is padding) is the LENS instantiation of the same
// bodies: addresses by L, every masking bound by the per-image length read from device memory (see image_len below).
#include "../../include/cdetr_hip.h"
#include "common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int D = 32;
constexpr int KT = 64;   // keys (or queries) per LDS tile

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float dot32(const float (&a)[D], const float* __restrict__ b) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
        const float4 t = *reinterpret_cast<const float4*>(b + c4 * 4);
        s0 = fmaf(a[c4 * 4 + 0], t.x, s0);
        s1 = fmaf(a[c4 * 4 + 1], t.y, s1);
        s2 = fmaf(a[c4 * 4 + 2], t.z, s2);
        s3 = fmaf(a[c4 * 4 + 3], t.w, s3);
    }
    return (s0 + s1) + (s2 + s3);
}

__device__ __forceinline__ void axpy32(float (&acc)[D], float p, const float* __restrict__ b) {
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
        const float4 t = *reinterpret_cast<const float4*>(b + c4 * 4);
        acc[c4 * 4 + 0] = fmaf(p, t.x, acc[c4 * 4 + 0]);
        acc[c4 * 4 + 1] = fmaf(p, t.y, acc[c4 * 4 + 1]);
        acc[c4 * 4 + 2] = fmaf(p, t.z, acc[c4 * 4 + 2]);
        acc[c4 * 4 + 3] = fmaf(p, t.w, acc[c4 * 4 + 3]);
    }
}

// rows [r0, r0+KT) of a [L][ld] matrix (32 columns starting at col0) -> LDS tile [KT][32]; zero beyond L
__device__ __forceinline__ void load_tile(float* __restrict__ dst, const float* __restrict__ src, long ld, int col0, int r0, int L) {
    for (int idx = threadIdx.x; idx < KT * 8; idx += blockDim.x) {
        const int r = idx >> 3, c4 = idx & 7;
        const float4 t = (r0 + r < L) ? ld4(src + (long)(r0 + r) * ld + col0 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(dst + r * D + c4 * 4) = t;
    }
}

// cdetr_mha_*_lens: image n's rows still start at n * L, only the masking bound becomes len = clamp(lens[n], 0, L) on the query AND the key side
// (one scalar per workgroup: uniform per blockIdx.y).  Every kernel below takes the row counts twice: Sq / Sk address the images, Lq / Lk
// bound the rows; the dense instantiations (LENS = false) set Lq = Sq, Lk = Sk and are the code they were.
template <bool LENS>
__device__ __forceinline__ int image_len(const int32_t* __restrict__ lens, int n, int L) {
    if constexpr (LENS) return min(max(lens[n], 0), L);
    else return L;
}

template <bool LENS>
__global__ __launch_bounds__(256) void mha_fwd_kernel(const float* __restrict__ qg, long ldq, const float* __restrict__ kg, long ldk,
                                                      const float* __restrict__ vg, long ldv, float* __restrict__ o, float* __restrict__ lse,
                                                      int Sq, int Sk, int nh, float scale, const int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) float Ks[KT * D];
    __shared__ __attribute__((aligned(16))) float Vs[KT * D];
    const int E = nh * D;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int i32 = lane & 15, g = lane >> 4;      // 16 rows per wave, 4-way split of the reduction axis
    const int n = blockIdx.y / nh, head = blockIdx.y % nh;
    const int q = blockIdx.x * 64 + wid * 16 + i32;
    const int Lq = image_len<LENS>(lens, n, Sq), Lk = LENS ? Lq : Sk;
    const bool qv = q < Lq;
    if constexpr (LENS) {
        if (!qv && q < Sq) {                       // padded query: exact zeros, nothing left uninitialised
            float* op = o + ((long)n * Sq + q) * E + head * D + g * 8;
            *reinterpret_cast<float4*>(op) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(op + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g == 0) lse[((long)n * nh + head) * Sq + q] = 0.f;
        }
        if ((int)blockIdx.x * 64 >= Lq) return;    // workgroup-uniform, before any barrier
    }
    const float* qn = qg + (long)n * Sq * ldq;
    const float* kn = kg + (long)n * Sk * ldk;
    const float* vn = vg + (long)n * Sk * ldv;
    float qr[D];
    {
        const float* qp = qn + (long)(qv ? q : 0) * ldq + head * D;
#pragma unroll
        for (int c4 = 0; c4 < 8; ++c4) {
            const float4 t = ld4(qp + c4 * 4);
            qr[c4 * 4 + 0] = t.x * scale; qr[c4 * 4 + 1] = t.y * scale; qr[c4 * 4 + 2] = t.z * scale; qr[c4 * 4 + 3] = t.w * scale;
        }
    }
    float m = -INFINITY, l = 0.f, acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.f;
    for (int k0 = 0; k0 < Lk; k0 += KT) {
        __syncthreads();
        load_tile(Ks, kn, ldk, head * D, k0, Lk);
        load_tile(Vs, vn, ldv, head * D, k0, Lk);
        __syncthreads();
        const int nk = min(KT, Lk - k0);
        float s[KT / 4];
        float tm = -INFINITY;
#pragma unroll
        for (int j = 0; j < KT / 4; ++j) {
            const int kk = 4 * j + g;
            s[j] = (kk < nk) ? dot32(qr, Ks + kk * D) : -INFINITY;
            tm = fmaxf(tm, s[j]);
        }
        const float mn = fmaxf(m, tm);
        if (mn > -INFINITY) {
            const float corr = expf(m - mn);       // m = -inf -> 0
            l *= corr;
#pragma unroll
            for (int c = 0; c < D; ++c) acc[c] *= corr;
#pragma unroll
            for (int j = 0; j < KT / 4; ++j) {
                const int kk = 4 * j + g;
                if (kk < nk) {
                    const float p = expf(s[j] - mn);
                    l += p;
                    axpy32(acc, p, Vs + kk * D);
                }
            }
            m = mn;
        }
    }
    // combine the four key-subset partials of each query
    float mn = fmaxf(m, __shfl_xor(m, 16, 64));
    mn = xhalf_max(mn);
    const float cs = (m > -INFINITY) ? expf(m - mn) : 0.f;
    l *= cs;
    l += __shfl_xor(l, 16, 64);
    l = xhalf_sum(l);
    const float inv = 1.f / l;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        float a = acc[c] * cs;
        a += __shfl_xor(a, 16, 64);
        a = xhalf_sum(a);
        acc[c] = a * inv;
    }
    if (qv) {
        float* op = o + ((long)n * Sq + q) * E + head * D + g * 8;     // each lane group writes 8 channels
#pragma unroll
        for (int c4 = 0; c4 < 2; ++c4)
            *reinterpret_cast<float4*>(op + c4 * 4) = make_float4(acc[g * 8 + c4 * 4 + 0], acc[g * 8 + c4 * 4 + 1],
                                                                  acc[g * 8 + c4 * 4 + 2], acc[g * 8 + c4 * 4 + 3]);
        if (g == 0) lse[((long)n * nh + head) * Sq + q] = mn + logf(l);
    }
}

// dq[i] = scale * sum_j p_ij (dO_i.v_j - D_i) k_j,   D_i = dO_i . O_i   (lanes own queries)
template <bool LENS>
__global__ __launch_bounds__(256) void mha_bwd_q_kernel(const float* __restrict__ qg, long ldq, const float* __restrict__ kg, long ldk,
                                                        const float* __restrict__ vg, long ldv, const float* __restrict__ o,
                                                        const float* __restrict__ dO, const float* __restrict__ lse, float* __restrict__ dq_out,
                                                        long lddq, float* __restrict__ Dbuf, int Sq, int Sk, int nh, float scale,
                                                        const int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) float Ks[KT * D];
    __shared__ __attribute__((aligned(16))) float Vs[KT * D];
    const int E = nh * D;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int i32 = lane & 15, g = lane >> 4;      // 16 rows per wave, 4-way split of the reduction axis
    const int n = blockIdx.y / nh, head = blockIdx.y % nh;
    const int q = blockIdx.x * 64 + wid * 16 + i32;
    const int Lq = image_len<LENS>(lens, n, Sq), Lk = LENS ? Lq : Sk;
    const bool qv = q < Lq;
    if constexpr (LENS) {
        if (!qv && q < Sq) {                       // padded query: d_q is exact zero
            float* out = dq_out + ((long)n * Sq + q) * lddq + head * D + g * 8;
            *reinterpret_cast<float4*>(out) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(out + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if ((int)blockIdx.x * 64 >= Lq) return;    // workgroup-uniform, before any barrier
    }
    const float* qn = qg + (long)n * Sq * ldq;
    const float* kn = kg + (long)n * Sk * ldk;
    const float* vn = vg + (long)n * Sk * ldv;
    float qr[D], dor[D], dq[D];
    float Di = 0.f;
    {
        const long row = (long)n * Sq + (qv ? q : 0);
        const float* qp = qn + (long)(qv ? q : 0) * ldq + head * D;
        const float* dp = dO + row * E + head * D;
        const float* op = o + row * E + head * D;
#pragma unroll
        for (int c4 = 0; c4 < 8; ++c4) {
            const float4 t = ld4(qp + c4 * 4), u = ld4(dp + c4 * 4), w = ld4(op + c4 * 4);
            qr[c4 * 4 + 0] = t.x * scale; qr[c4 * 4 + 1] = t.y * scale; qr[c4 * 4 + 2] = t.z * scale; qr[c4 * 4 + 3] = t.w * scale;
            dor[c4 * 4 + 0] = u.x; dor[c4 * 4 + 1] = u.y; dor[c4 * 4 + 2] = u.z; dor[c4 * 4 + 3] = u.w;
            Di += (u.x * w.x + u.y * w.y) + (u.z * w.z + u.w * w.w);
        }
#pragma unroll
        for (int c = 0; c < D; ++c) dq[c] = 0.f;
    }
    const float li = qv ? lse[((long)n * nh + head) * Sq + q] : 0.f;
    for (int k0 = 0; k0 < Lk; k0 += KT) {
        __syncthreads();
        load_tile(Ks, kn, ldk, head * D, k0, Lk);
        load_tile(Vs, vn, ldv, head * D, k0, Lk);
        __syncthreads();
        const int nk = min(KT, Lk - k0);
        for (int kk = g; kk < nk; kk += 4) {
            const float p = expf(dot32(qr, Ks + kk * D) - li);
            const float ds = p * (dot32(dor, Vs + kk * D) - Di);
            axpy32(dq, ds, Ks + kk * D);
        }
    }
#pragma unroll
    for (int c = 0; c < D; ++c) {
        float a = dq[c];
        a += __shfl_xor(a, 16, 64);
        a = xhalf_sum(a);
        dq[c] = a * scale;
    }
    if (qv) {
        float* out = dq_out + ((long)n * Sq + q) * lddq + head * D;
#pragma unroll
        for (int c4 = 0; c4 < 2; ++c4)
            *reinterpret_cast<float4*>(out + g * 8 + c4 * 4) = make_float4(dq[g * 8 + c4 * 4 + 0], dq[g * 8 + c4 * 4 + 1],
                                                                           dq[g * 8 + c4 * 4 + 2], dq[g * 8 + c4 * 4 + 3]);
        if (g == 0) Dbuf[((long)n * nh + head) * Sq + q] = Di;
    }
}

// dk[j] = scale * sum_i p_ij (dO_i.v_j - D_i) q_i,   dv[j] = sum_i p_ij dO_i   (lanes own keys, query tiles through LDS)
template <bool LENS>
__global__ __launch_bounds__(256) void mha_bwd_kv_kernel(const float* __restrict__ qg, long ldq, const float* __restrict__ kg, long ldk,
                                                         const float* __restrict__ vg, long ldv, const float* __restrict__ dO,
                                                         const float* __restrict__ lse, const float* __restrict__ Dbuf,
                                                         float* __restrict__ dk_out, long lddk, float* __restrict__ dv, long lddv,
                                                         int Sq, int Sk, int nh, float scale, const int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) float Qs[KT * D];
    __shared__ __attribute__((aligned(16))) float Os[KT * D];
    __shared__ float Ls[KT], Dsh[KT];
    const int E = nh * D;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int i32 = lane & 15, g = lane >> 4;      // 16 rows per wave, 4-way split of the reduction axis
    const int n = blockIdx.y / nh, head = blockIdx.y % nh;
    const int j = blockIdx.x * 64 + wid * 16 + i32;
    const int Lq = image_len<LENS>(lens, n, Sq), Lk = LENS ? Lq : Sk;
    const bool jv = j < Lk;
    if constexpr (LENS) {
        if (!jv && j < Sk) {                       // padded key: d_k and d_v are exact zeros
            float* ok = dk_out + ((long)n * Sk + j) * lddk + head * D + g * 8;
            float* ov = dv + ((long)n * Sk + j) * lddv + head * D + g * 8;
            *reinterpret_cast<float4*>(ok) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(ok + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(ov) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(ov + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if ((int)blockIdx.x * 64 >= Lk) return;    // workgroup-uniform, before any barrier
    }
    const float* qn = qg + (long)n * Sq * ldq;
    const float* don = dO + (long)n * Sq * E;
    float kr[D], vr[D], dk[D], dvv[D];
    {
        const float* kp = kg + ((long)n * Sk + (jv ? j : 0)) * ldk + head * D;
        const float* vp = vg + ((long)n * Sk + (jv ? j : 0)) * ldv + head * D;
#pragma unroll
        for (int c4 = 0; c4 < 8; ++c4) {
            const float4 t = ld4(kp + c4 * 4), u = ld4(vp + c4 * 4);
            kr[c4 * 4 + 0] = t.x * scale; kr[c4 * 4 + 1] = t.y * scale; kr[c4 * 4 + 2] = t.z * scale; kr[c4 * 4 + 3] = t.w * scale;
            vr[c4 * 4 + 0] = u.x; vr[c4 * 4 + 1] = u.y; vr[c4 * 4 + 2] = u.z; vr[c4 * 4 + 3] = u.w;
        }
#pragma unroll
        for (int c = 0; c < D; ++c) { dk[c] = 0.f; dvv[c] = 0.f; }
    }
    for (int q0 = 0; q0 < Lq; q0 += KT) {
        __syncthreads();
        load_tile(Qs, qn, ldq, head * D, q0, Lq);
        load_tile(Os, don, E, head * D, q0, Lq);
        for (int r = threadIdx.x; r < KT; r += blockDim.x) {
            const bool ok = q0 + r < Lq;
            Ls[r] = ok ? lse[((long)n * nh + head) * Sq + q0 + r] : INFINITY;    // p = exp(s - inf) = 0 beyond Lq
            Dsh[r] = ok ? Dbuf[((long)n * nh + head) * Sq + q0 + r] : 0.f;
        }
        __syncthreads();
        const int nq = min(KT, Lq - q0);
        for (int r = g; r < nq; r += 4) {
            const float p = expf(dot32(kr, Qs + r * D) - Ls[r]);
            axpy32(dvv, p, Os + r * D);
            const float ds = p * (dot32(vr, Os + r * D) - Dsh[r]);
            axpy32(dk, ds, Qs + r * D);
        }
    }
#pragma unroll
    for (int c = 0; c < D; ++c) {
        float a = dk[c], b = dvv[c];
        a += __shfl_xor(a, 16, 64);
        a = xhalf_sum(a);
        b += __shfl_xor(b, 16, 64);
        b = xhalf_sum(b);
        dk[c] = a * scale;
        dvv[c] = b;
    }
    if (jv) {
        float* ok = dk_out + ((long)n * Sk + j) * lddk + head * D + g * 8;
        float* ov = dv + ((long)n * Sk + j) * lddv + head * D + g * 8;
#pragma unroll
        for (int c4 = 0; c4 < 2; ++c4) {
            *reinterpret_cast<float4*>(ok + c4 * 4) = make_float4(dk[g * 8 + c4 * 4 + 0], dk[g * 8 + c4 * 4 + 1],
                                                                  dk[g * 8 + c4 * 4 + 2], dk[g * 8 + c4 * 4 + 3]);
            *reinterpret_cast<float4*>(ov + c4 * 4) = make_float4(dvv[g * 8 + c4 * 4 + 0], dvv[g * 8 + c4 * 4 + 1],
                                                                  dvv[g * 8 + c4 * 4 + 2], dvv[g * 8 + c4 * 4 + 3]);
        }
    }
}


// ------------------------------------------------------------------------------------------------ matrix-core variants
// split-bf16 (bf16x3) flash attention for the same problem.  Workgroup = 2 waves; a wave OWNS 32 rows (queries for the
// forward / dq kernels, keys for the dk-dv kernel) as the LANES of a transposed accumulator and walks over 32-row tiles of
// the other side:
//   X^T[other, own]  = sum_c Other[other, c] Own[own, c]      A = tile rows (k = c, natural layout), B = own rows (hoisted, split once)
//   Y^T[c, own]     += sum_other W[other, c] Z[other, own]    A = W^T tile (k = other, transposed at staging), B = Z straight
//                                                             from the registers of the first product (slot j of step s = reg 8s + j)
// so softmax statistics, the log-sum-exp and D are per-LANE scalars and no probability ever touches LDS or HBM.  Tiles are
// split into bf16 hi / lo once per workgroup while they are staged ([row][hi 32 | lo 32 | pad 8]); the transposed tiles
// store the reduction index in the order the accumulator registers enumerate it (perm_pos).  Three tiles are in flight in a
// statically indexed register ring (unconditional loads, rows clamped to L-1 and masked arithmetically).
namespace flash {
constexpr int NWF = 2, NTF = 64 * NWF, TS = 72, TILE = 32 * TS;

// first position of the 4-row group starting at row k0 (multiple of 4) inside a transposed tile
__device__ __forceinline__ int perm_pos(int k0) { return (k0 & 16) | ((k0 & 4) << 1) | ((k0 & 8) >> 1); }
// tile-row index that accumulator register r of lane group g enumerates
__device__ __forceinline__ int reg_row(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

struct NatRegs { float4 v[2]; };
struct TrRegs { float t[16]; };      // t[4 kk + c]: plain scalars (a float4 array read component-wise ends up in scratch)
// natural tile: rows r0.. of a [L][ld] matrix, 32 columns from col0; thread -> (row = idx >> 3, c4 = idx & 7), idx = tid + 128 s
__device__ __forceinline__ void nat_fetch(NatRegs& r, const float* __restrict__ src, long ld, int col0, int r0, int L, int tid) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int idx = tid + NTF * s;
        r.v[s] = ld4(src + (long)min(r0 + (idx >> 3), L - 1) * ld + col0 + (idx & 7) * 4);
    }
}
__device__ __forceinline__ void nat_stash(const NatRegs& r, __bf16* tile, int tid) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int idx = tid + NTF * s;
        stash_split4(tile + (idx >> 3) * TS + (idx & 7) * 4, 32, r.v[s].x, r.v[s].y, r.v[s].z, r.v[s].w);
    }
}
// the same with every element multiplied by `mul` before the split (own_frag's `scale` for a staged tile)
__device__ __forceinline__ void nat_stash(const NatRegs& r, __bf16* tile, int tid, float mul) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int idx = tid + NTF * s;
        stash_split4(tile + (idx >> 3) * TS + (idx & 7) * 4, 32, r.v[s].x * mul, r.v[s].y * mul, r.v[s].z * mul, r.v[s].w * mul);
    }
}
// transposed tile (64 threads `t`): block (row quad kq = t & 7, column quad cq = t >> 3) = 4 rows x 4 columns
__device__ __forceinline__ void tr_fetch(TrRegs& r, const float* __restrict__ src, long ld, int col0, int r0, int L, int t) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const float4 v = ld4(src + (long)min(r0 + 4 * (t & 7) + kk, L - 1) * ld + col0 + (t >> 3) * 4);
        r.t[4 * kk] = v.x; r.t[4 * kk + 1] = v.y; r.t[4 * kk + 2] = v.z; r.t[4 * kk + 3] = v.w;
    }
}
__device__ __forceinline__ void tr_stash(const TrRegs& r, __bf16* tile, int t) {
    __bf16* dst = tile + (4 * (t >> 3)) * TS + perm_pos(4 * (t & 7));
#pragma unroll
    for (int c = 0; c < 4; ++c) stash_split4(dst + c * TS, 32, r.t[c], r.t[4 + c], r.t[8 + c], r.t[12 + c]);
}
// acc += A(tile rows, this lane's row i32) * B (hi/lo fragments of the two k-steps); TERMS = 1: hi * hi only (the lo halves are not read)
template <int TERMS = 3>
__device__ __forceinline__ f32x16 mma_tile(f32x16 acc, const __bf16* tile, int i32, int g, const bf16x8 (&bh)[2], const bf16x8 (&bl)[2]) {
    const __bf16* a = tile + i32 * TS + 8 * g;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a + 16 * s);
        if constexpr (TERMS == 1) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[s], acc, 0, 0, 0);
        } else {
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(a + 32 + 16 * s);
            acc = mfma_bf16x3(ah, al, bh[s], bl[s], acc);
        }
    }
    return acc;
}
// hoisted B operand from this lane's own row: columns 16s + 8g .. +7, scaled
__device__ __forceinline__ void own_frag(const float* __restrict__ row, int g, float scale, bf16x8 (&bh)[2], bf16x8 (&bl)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float4 t0 = ld4(row + 16 * s + 8 * g), t1 = ld4(row + 16 * s + 8 * g + 4);
        const float x[8] = {t0.x * scale, t0.y * scale, t0.z * scale, t0.w * scale, t1.x * scale, t1.y * scale, t1.z * scale, t1.w * scale};
        split_bf16x8(x, bh[s], bl[s]);
    }
}
__device__ __forceinline__ void reg_frag(const f32x16& z, bf16x8 (&bh)[2], bf16x8 (&bl)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float x[8] = {z[8 * s], z[8 * s + 1], z[8 * s + 2], z[8 * s + 3], z[8 * s + 4], z[8 * s + 5], z[8 * s + 6], z[8 * s + 7]};
        split_bf16x8(x, bh[s], bl[s]);
    }
}
// transposed accumulator -> 32 contiguous floats of this lane's row (registers r = 4j..4j+3 are columns 8j + 4g ..)
__device__ __forceinline__ void store_own(float* __restrict__ row, int g, const f32x16& a, float mul) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        *reinterpret_cast<float4*>(row + 8 * j + 4 * g) = make_float4(a[4 * j] * mul, a[4 * j + 1] * mul, a[4 * j + 2] * mul, a[4 * j + 3] * mul);
}
__device__ __forceinline__ f32x16 zero16() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// a padded row (len <= row < L) of a lens launch: this lane's 16 of the row's 32 columns as exact zeros
__device__ __forceinline__ void zero_own(float* __restrict__ row, int g) { store_own(row, g, zero16(), 0.f); }

template <bool LENS>
__global__ __launch_bounds__(NTF) void fwd_kernel(const float* __restrict__ qg, long ldq, const float* __restrict__ kg, long ldk,
                                                  const float* __restrict__ vg, long ldv, float* __restrict__ o, float* __restrict__ lse,
                                                  int Sq, int Sk, int nh, float scale, const int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * 2 * TILE];          // [buf][K | V^T]
    const int E = nh * D;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i32 = lane & 31, g = lane >> 5;
    const int n = blockIdx.y / nh, head = blockIdx.y % nh;
    const int q = blockIdx.x * 32 * NWF + wid * 32 + i32;
    const int Lq = image_len<LENS>(lens, n, Sq), Lk = LENS ? Lq : Sk;
    if constexpr (LENS) {
        if (q >= Lq && q < Sq) {
            zero_own(o + ((long)n * Sq + q) * E + head * D, g);
            if (g == 0) lse[((long)n * nh + head) * Sq + q] = 0.f;
        }
        if ((int)blockIdx.x * 32 * NWF >= Lq) return;                          // workgroup-uniform, before any barrier
    }
    const float* kn = kg + (long)n * Sk * ldk;
    const float* vn = vg + (long)n * Sk * ldv;
    bf16x8 qh[2], ql[2];
    own_frag(qg + ((long)n * Sq + min(q, Lq - 1)) * ldq + head * D, g, scale, qh, ql);
    float m = -INFINITY, l = 0.f;
    f32x16 OT = zero16();
    constexpr int PD = 3;                                                      // tiles in flight (register ring, statically indexed)
    struct Ring { NatRegs k; TrRegs v; } r0, r1, r2;          // separate variables, not an array: keeps them in registers
    const int ntile = (Lk + 31) / 32;
    auto fetch = [&](NatRegs& a, TrRegs& b, int t) __attribute__((always_inline)) {
        const int r0 = min(t, ntile - 1) * 32;                                 // surplus prefetches re-read the last tile
        nat_fetch(a, kn, ldk, head * D, r0, Lk, tid);
        tr_fetch(b, vn, ldv, head * D, r0, Lk, lane);       // every wave loads (only wave 0 stages): keeps the ring in registers
    };
    auto stash = [&](const NatRegs& a, const TrRegs& b, int buf) __attribute__((always_inline)) {
        nat_stash(a, lds + buf * 2 * TILE, tid);
        if (wid == 0) tr_stash(b, lds + buf * 2 * TILE + TILE, lane);
    };
    fetch(r0.k, r0.v, 0); fetch(r1.k, r1.v, 1); fetch(r2.k, r2.v, 2);
    stash(r0.k, r0.v, 0);
    __syncthreads();
    auto step = [&](Ring& cur, const Ring& nxt, int t) __attribute__((always_inline)) {
        // steps past the last tile run on a re-read of it with every row masked: numerically a no-op, and the ring stays branch-free
        const int buf = t & 1;
        fetch(cur.k, cur.v, t + PD);                                           // `cur` (tile t) was staged one step ago
        if (t < ntile) {           // workgroup-uniform: the (up to PD - 1) surplus steps of the last ring turn only stage and synchronise
            f32x16 S = mma_tile(zero16(), lds + buf * 2 * TILE, i32, g, qh, ql);
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (t * 32 + reg_row(r, g) >= Lk) S[r] = -INFINITY;
                mx = fmaxf(mx, S[r]);
            }
            mx = xhalf_max(mx);
            const float mn = fmaxf(m, mx);
            const float corr = __expf(m - mn);
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { S[r] = __expf(S[r] - mn); ls += S[r]; }
            ls = xhalf_sum(ls);
            l = l * corr + ls;
            m = mn;
#pragma unroll
            for (int r = 0; r < 16; ++r) OT[r] *= corr;
            bf16x8 ph[2], pl[2];
            reg_frag(S, ph, pl);
            OT = mma_tile(OT, lds + buf * 2 * TILE + TILE, i32, g, ph, pl);
        }
        stash(nxt.k, nxt.v, buf ^ 1);                                          // tile t + 1
        __syncthreads();
    };
    for (int t0 = 0; t0 < ntile; t0 += PD) {
        step(r0, r1, t0);
        step(r1, r2, t0 + 1);
        step(r2, r0, t0 + 2);
    }
    if (q < Lq) {
        store_own(o + ((long)n * Sq + q) * E + head * D, g, OT, 1.f / l);
        if (g == 0) lse[((long)n * nh + head) * Sq + q] = m + logf(l);
    }
}

// The same forward with the KEYS of a query tile cut in two: 4 waves per workgroup -- waves (0, 1) walk the first half of the key tiles, waves (2, 3)
// the second half, for the same 2 x 32 queries -- and merge their (running maximum, sum, O^T) through LDS at the end.  A wave's life is a chain of
// [barrier, two dependent MFMA groups, a softmax update] per key tile with nobody to overlap with (160 waves on 1024 SIMDs at L = 300): half the steps per
// wave.  Each half stages its own tiles (its two waves = the 128 staging threads of fwd_kernel), both halves share the barriers.
template <bool LENS>
__global__ __launch_bounds__(2 * NTF) void fwd_ks_kernel(const float* __restrict__ qg, long ldq, const float* __restrict__ kg, long ldk,
                                                         const float* __restrict__ vg, long ldv, float* __restrict__ o, float* __restrict__ lse,
                                                         int Sq, int Sk, int nh, float scale, const int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) __bf16 lds_all[2 * 2 * 2 * TILE];      // [key half][buf][K | V^T]
    const int E = nh * D;
    const int tid = threadIdx.x & (NTF - 1), lane = tid & 63, wid = tid >> 6, i32 = lane & 31, g = lane >> 5;
    const int kh = threadIdx.x / NTF;                                          // key half of this wave pair
    __bf16* lds = lds_all + kh * (2 * 2 * TILE);
    const int n = blockIdx.y / nh, head = blockIdx.y % nh;
    const int q = blockIdx.x * 32 * NWF + wid * 32 + i32;
    const int Lq = image_len<LENS>(lens, n, Sq), Lk = LENS ? Lq : Sk;
    if constexpr (LENS) {
        if (kh == 0 && q >= Lq && q < Sq) {
            zero_own(o + ((long)n * Sq + q) * E + head * D, g);
            if (g == 0) lse[((long)n * nh + head) * Sq + q] = 0.f;
        }
        if ((int)blockIdx.x * 32 * NWF >= Lq) return;                          // workgroup-uniform, before any barrier
    }
    const float* kn = kg + (long)n * Sk * ldk;
    const float* vn = vg + (long)n * Sk * ldv;
    bf16x8 qh[2], ql[2];
    own_frag(qg + ((long)n * Sq + min(q, Lq - 1)) * ldq + head * D, g, scale, qh, ql);
    float m = -INFINITY, l = 0.f;
    f32x16 OT = zero16();
    constexpr int PD = 3;
    struct Ring { NatRegs k; TrRegs v; } r0, r1, r2;
    const int ntile = (Lk + 31) / 32, nth = (ntile + 1) / 2;                     // tiles in all / per half (the second half may hold fewer)
    const int tbase = kh * nth, nmine = max(0, min(nth, ntile - tbase));
    auto fetch = [&](NatRegs& a, TrRegs& b, int t) __attribute__((always_inline)) {
        const int r0_ = min(tbase + min(t, max(nmine - 1, 0)), ntile - 1) * 32;   // surplus prefetches re-read this half's last tile
        nat_fetch(a, kn, ldk, head * D, r0_, Lk, tid);
        tr_fetch(b, vn, ldv, head * D, r0_, Lk, lane);
    };
    auto stash = [&](const NatRegs& a, const TrRegs& b, int buf) __attribute__((always_inline)) {
        nat_stash(a, lds + buf * 2 * TILE, tid);
        if (wid == 0) tr_stash(b, lds + buf * 2 * TILE + TILE, lane);
    };
    fetch(r0.k, r0.v, 0); fetch(r1.k, r1.v, 1); fetch(r2.k, r2.v, 2);
    stash(r0.k, r0.v, 0);
    __syncthreads();
    auto step = [&](Ring& cur, const Ring& nxt, int t) __attribute__((always_inline)) {
        const int buf = t & 1;
        fetch(cur.k, cur.v, t + PD);
        if (t < nmine) {           // wave-pair-uniform
            f32x16 S = mma_tile(zero16(), lds + buf * 2 * TILE, i32, g, qh, ql);
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if ((tbase + t) * 32 + reg_row(r, g) >= Lk) S[r] = -INFINITY;
                mx = fmaxf(mx, S[r]);
            }
            mx = xhalf_max(mx);
            const float mn = fmaxf(m, mx);
            const float corr = __expf(m - mn);
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { S[r] = __expf(S[r] - mn); ls += S[r]; }
            ls = xhalf_sum(ls);
            l = l * corr + ls;
            m = mn;
#pragma unroll
            for (int r = 0; r < 16; ++r) OT[r] *= corr;
            bf16x8 ph[2], pl[2];
            reg_frag(S, ph, pl);
            OT = mma_tile(OT, lds + buf * 2 * TILE + TILE, i32, g, ph, pl);
        }
        stash(nxt.k, nxt.v, buf ^ 1);
        __syncthreads();
    };
    for (int t0 = 0; t0 < nth; t0 += PD) {         // (both halves run nth steps: the barriers are the workgroup's)
        step(r0, r1, t0);
        step(r1, r2, t0 + 1);
        step(r2, r0, t0 + 2);
    }
    // merge: the second half parks (m, l, O^T) per lane, the first half folds them in and stores
    float* mrg = reinterpret_cast<float*>(lds_all) + (wid * 64 + lane) * 18;     // (the tile buffers are free: every wave is behind the loop's last barrier)
    if (kh == 1) {
        mrg[0] = m; mrg[1] = l;
#pragma unroll
        for (int r = 0; r < 16; ++r) mrg[2 + r] = OT[r];
    }
    __syncthreads();
    if (kh == 0 && q < Lq) {
        const float m2 = mrg[0], l2 = mrg[1];
        const float mn = fmaxf(m, m2);
        const float c1 = (m == -INFINITY) ? 0.f : __expf(m - mn), c2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
        const float lt = l * c1 + l2 * c2;
        f32x16 OM;
#pragma unroll
        for (int r = 0; r < 16; ++r) OM[r] = OT[r] * c1 + mrg[2 + r] * c2;
        store_own(o + ((long)n * Sq + q) * E + head * D, g, OM, 1.f / lt);
        if (g == 0) lse[((long)n * nh + head) * Sq + q] = mn + logf(lt);
    }
}

// (The same split of the walked side was built for the backward -- the halves' accumulators simply add -- and measured: 21 -> 20 us.  The backward holds
// 320 registers per lane (one wave per SIMD): 320 workgroups of four waves are 1280 waves for 1024 slots, a second round eats the halved loop.  Not kept.)
// The backward is ONE launch: workgroups with blockIdx.z == 0 own queries (dq), those with blockIdx.z == 1 own keys (dk, dv).  The two
// halves are independent -- the key half forms D = rowsum(dO * O) of each query tile itself while it stages the tile (it used to read the
// query half's result, which serialised two 17 us launches of 80 workgroups each) -- so they share the chip instead of following each other.
// TB = bf16 MFMAs per product of the four GRADIENT contractions (dP = dO V^T, dQ, dK, dV): 3 = split-bf16 like the forward, 1 = plain bf16 (the
// backward's default arithmetic, ops.PRECISION_BWD 3).  The recomputed scores S = Q K^T keep all three terms in both: p = exp(S - lse) against the
// FORWARD's log-sum-exp turns an error of S into a relative error of every probability of the row.
template <int TB>
__device__ __forceinline__ void bwd_q_body(__bf16* lds, const float* __restrict__ qg, long ldq, const float* __restrict__ kg, long ldk,
                                           const float* __restrict__ vg, long ldv, const float* __restrict__ o, const float* __restrict__ dO,
                                           const float* __restrict__ lse, float* __restrict__ dq_out, long lddq, int Sq, int Sk, int Lq,
                                           int Lk, int nh, float scale) {
    // lds: [buf][K | V | K^T]
    const int E = nh * D;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i32 = lane & 31, g = lane >> 5;
    const int n = blockIdx.y / nh, head = blockIdx.y % nh;
    const int q = blockIdx.x * 32 * NWF + wid * 32 + i32;
    const int qc = min(q, Lq - 1);
    const float* kn = kg + (long)n * Sk * ldk;
    const float* vn = vg + (long)n * Sk * ldv;
    bf16x8 qh[2], ql[2], dh[2], dl[2];
    own_frag(qg + ((long)n * Sq + qc) * ldq + head * D, g, scale, qh, ql);
    const float* dop = dO + ((long)n * Sq + qc) * E + head * D;
    own_frag(dop, g, 1.f, dh, dl);
    float Di = 0.f;
    {
        const float* op = o + ((long)n * Sq + qc) * E + head * D;
#pragma unroll
        for (int c4 = 0; c4 < 8; ++c4) {
            const float4 u = ld4(dop + c4 * 4), w = ld4(op + c4 * 4);
            Di += (u.x * w.x + u.y * w.y) + (u.z * w.z + u.w * w.w);
        }
    }
    const float li = lse[((long)n * nh + head) * Sq + qc];
    f32x16 dQT = zero16();
    constexpr int PD = 3;
    struct Ring { NatRegs k, v; TrRegs kt; } r0, r1, r2;
    const int ntile = (Lk + 31) / 32;
    auto fetch = [&](NatRegs& a, NatRegs& b, TrRegs& c, int t) __attribute__((always_inline)) {
        const int r0 = min(t, ntile - 1) * 32;
        nat_fetch(a, kn, ldk, head * D, r0, Lk, tid);
        nat_fetch(b, vn, ldv, head * D, r0, Lk, tid);
        tr_fetch(c, kn, ldk, head * D, r0, Lk, lane);
    };
    auto stash = [&](const NatRegs& a, const NatRegs& b, const TrRegs& c, int buf) __attribute__((always_inline)) {
        __bf16* nb = lds + buf * 3 * TILE;
        nat_stash(a, nb, tid);
        nat_stash(b, nb + TILE, tid);
        if (wid == 0) tr_stash(c, nb + 2 * TILE, lane);
    };
    fetch(r0.k, r0.v, r0.kt, 0); fetch(r1.k, r1.v, r1.kt, 1); fetch(r2.k, r2.v, r2.kt, 2);
    stash(r0.k, r0.v, r0.kt, 0);
    __syncthreads();
    auto step = [&](Ring& cur, const Ring& nxt, int t) __attribute__((always_inline)) {
        const int buf = t & 1;
        fetch(cur.k, cur.v, cur.kt, t + PD);
        const __bf16* base = lds + buf * 3 * TILE;
        if (t < ntile) {           // workgroup-uniform: surplus steps of the last ring turn only stage and synchronise
            f32x16 S = mma_tile(zero16(), base, i32, g, qh, ql);
            const f32x16 dP = mma_tile<TB>(zero16(), base + TILE, i32, g, dh, dl);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = (t * 32 + reg_row(r, g) < Lk) ? __expf(S[r] - li) : 0.f;
                S[r] = p * (dP[r] - Di);
            }
            bf16x8 sh[2], sl[2];
            reg_frag(S, sh, sl);
            dQT = mma_tile<TB>(dQT, base + 2 * TILE, i32, g, sh, sl);
        }
        stash(nxt.k, nxt.v, nxt.kt, buf ^ 1);
        __syncthreads();
    };
    for (int t0 = 0; t0 < ntile; t0 += PD) {
        step(r0, r1, t0);
        step(r1, r2, t0 + 1);
        step(r2, r0, t0 + 2);
    }
    if (q < Lq) {
        store_own(dq_out + ((long)n * Sq + q) * lddq + head * D, g, dQT, scale);
    }
}

template <int TB>
__device__ __forceinline__ void bwd_kv_body(__bf16* lds, float (*stat)[2][32], const float* __restrict__ qg, long ldq,
                                            const float* __restrict__ kg, long ldk, const float* __restrict__ vg, long ldv,
                                            const float* __restrict__ o, const float* __restrict__ dO, const float* __restrict__ lse,
                                            float* __restrict__ dk_out, long lddk, float* __restrict__ dv, long lddv, int Sq, int Sk, int Lq,
                                            int Lk, int nh, float scale) {
    // lds: [buf][Q | dO | Q^T | dO^T]; stat: [buf][lse | D][query of the tile]
    const int E = nh * D;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i32 = lane & 31, g = lane >> 5;
    const int n = blockIdx.y / nh, head = blockIdx.y % nh;
    const int j = blockIdx.x * 32 * NWF + wid * 32 + i32;
    const int jc = min(j, Lk - 1);
    const float* qn = qg + (long)n * Sq * ldq;
    const float* don = dO + (long)n * Sq * E;
    const float* on = o + (long)n * Sq * E;
    const float* lsn = lse + ((long)n * nh + head) * Sq;
    bf16x8 kh[2], kl[2], vh[2], vl[2];
    // The scale goes on the QUERY side, before the split, as in the forward and in bwd_q_body: S^T is then the sum of the same three bf16
    // products per element as the S behind `lse` (split(q * scale) x split(k)), and the split's truncation -- ~2^-17 of sum |q_c k_c|, 1e-4
    // at the logit magnitudes of peaked or offset rows -- cancels in p = exp(S - lse).  With it on the key side (split(q) x split(k * scale))
    // the two truncations were independent: every p, and with it dV and dK, carried that 1e-4 as a relative error (dQ did not).
    own_frag(kg + ((long)n * Sk + jc) * ldk + head * D, g, 1.f, kh, kl);
    own_frag(vg + ((long)n * Sk + jc) * ldv + head * D, g, 1.f, vh, vl);
    f32x16 dKT = zero16(), dVT = zero16();
    constexpr int PD = 3;
    const float* trsrc = (wid == 0) ? qn : don;                                // wave 0 stages Q^T, wave 1 dO^T
    const long trld = (wid == 0) ? ldq : E;
    struct Ring { NatRegs q, d, o; TrRegs t; float s; } r0, r1, r2;
    const int ntile = (Lq + 31) / 32;
    auto fetch = [&](Ring& r, int t) __attribute__((always_inline)) {
        const int r0 = min(t, ntile - 1) * 32;
        nat_fetch(r.q, qn, ldq, head * D, r0, Lq, tid);
        nat_fetch(r.d, don, E, head * D, r0, Lq, tid);
        nat_fetch(r.o, on, E, head * D, r0, Lq, tid);                      // the forward's output rows of the tile: D = rowsum(dO * O)
        tr_fetch(r.t, trsrc, trld, head * D, r0, Lq, lane);
        const int qq = t * 32 + (tid & 31);                                // lse of the tile (lanes 0-31 of wave 0)
        const float x = lsn[min(qq, Lq - 1)];                              // (true, unclamped index: surplus tiles must be inert)
        r.s = (qq < Lq) ? x : INFINITY;                                    // p = exp(s - inf) = 0 beyond Lq
    };
    auto stash = [&](const Ring& r, int buf) __attribute__((always_inline)) {
        __bf16* nb = lds + buf * 4 * TILE;
        nat_stash(r.q, nb, tid, scale);                                          // Q * scale for S^T; Q^T below stays unscaled (dK is scaled once, at the store)
        nat_stash(r.d, nb + TILE, tid);
        tr_stash(r.t, nb + (wid == 0 ? 2 : 3) * TILE, lane);
        if (tid < 32) stat[buf][0][tid] = r.s;
        // D of the tile's 32 queries: thread (row = idx >> 3, 4 columns) holds a quarter-row product of dO and O; the 8 threads of a row
        // are consecutive lanes (rows past Lq are clamped copies: their p is 0, any finite D will do)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float pd = (r.d.v[s2].x * r.o.v[s2].x + r.d.v[s2].y * r.o.v[s2].y) + (r.d.v[s2].z * r.o.v[s2].z + r.d.v[s2].w * r.o.v[s2].w);
            pd += __shfl_xor(pd, 1, 64);
            pd += __shfl_xor(pd, 2, 64);
            pd += __shfl_xor(pd, 4, 64);
            if ((tid & 7) == 0) stat[buf][1][(tid + NTF * s2) >> 3] = pd;
        }
    };
    fetch(r0, 0); fetch(r1, 1); fetch(r2, 2);
    stash(r0, 0);
    __syncthreads();
    auto step = [&](Ring& cur, const Ring& nxt, int t) __attribute__((always_inline)) {
        const int buf = t & 1;
        fetch(cur, t + PD);
        const __bf16* base = lds + buf * 4 * TILE;
        if (t < ntile) {           // workgroup-uniform: surplus steps of the last ring turn only stage and synchronise
        f32x16 S = mma_tile(zero16(), base, i32, g, kh, kl);                   // S^T[q, key]
        const f32x16 dP = mma_tile<TB>(zero16(), base + TILE, i32, g, vh, vl);     // dP^T[q, key]
        f32x16 P;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const float4 ls4 = *reinterpret_cast<const float4*>(&stat[buf][0][8 * jj + 4 * g]);
            const float4 d4 = *reinterpret_cast<const float4*>(&stat[buf][1][8 * jj + 4 * g]);
            const float lsv[4] = {ls4.x, ls4.y, ls4.z, ls4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float p = __expf(S[4 * jj + b] - lsv[b]);
                P[4 * jj + b] = p;
                S[4 * jj + b] = p * (dP[4 * jj + b] - dvv[b]);
            }
        }
        bf16x8 ph[2], pl[2], sh[2], sl[2];
        reg_frag(P, ph, pl);
        dVT = mma_tile<TB>(dVT, base + 3 * TILE, i32, g, ph, pl);              // dV^T[c, key] += dO^T[c, q] P[q, key]
        reg_frag(S, sh, sl);
        dKT = mma_tile<TB>(dKT, base + 2 * TILE, i32, g, sh, sl);              // dK^T[c, key] += Q^T[c, q] dS[q, key]
        }
        stash(nxt, buf ^ 1);
        __syncthreads();
    };
    for (int t0 = 0; t0 < ntile; t0 += PD) {
        step(r0, r1, t0);
        step(r1, r2, t0 + 1);
        step(r2, r0, t0 + 2);
    }
    if (j < Lk) {
        store_own(dk_out + ((long)n * Sk + j) * lddk + head * D, g, dKT, scale);
        store_own(dv + ((long)n * Sk + j) * lddv + head * D, g, dVT, 1.f);
    }
}

// With Lq != Lk the grid is as wide as the longer side: the surplus workgroups of the shorter one exit at once (workgroup-uniform,
// before any barrier).  Measured against two launches of exactly sized grids: see cdetr_attn_bwd.
template <int TB, bool LENS>
__global__ __launch_bounds__(NTF) void bwd_kernel(const float* __restrict__ qg, long ldq, const float* __restrict__ kg, long ldk,
                                                  const float* __restrict__ vg, long ldv, const float* __restrict__ o,
                                                  const float* __restrict__ dO, const float* __restrict__ lse, float* __restrict__ dq,
                                                  long lddq, float* __restrict__ dk, long lddk, float* __restrict__ dv, long lddv, int Sq,
                                                  int Sk, int nh, float scale, int zbase, const int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * 4 * TILE];
    __shared__ __attribute__((aligned(16))) float stat[2][2][32];
    const int z = blockIdx.z + zbase;
    const int Lq = image_len<LENS>(lens, blockIdx.y / nh, Sq), Lk = LENS ? Lq : Sk;
    if constexpr (LENS) {                          // padded rows of this workgroup's tile: exact zeros (the bodies store rows < len only)
        const int n = blockIdx.y / nh, head = blockIdx.y % nh, lane = threadIdx.x & 63;
        const int row = blockIdx.x * 32 * NWF + (threadIdx.x >> 6) * 32 + (lane & 31), g = lane >> 5;
        if (z == 0 && row >= Lq && row < Sq) zero_own(dq + ((long)n * Sq + row) * lddq + head * D, g);
        if (z != 0 && row >= Lk && row < Sk) {
            zero_own(dk + ((long)n * Sk + row) * lddk + head * D, g);
            zero_own(dv + ((long)n * Sk + row) * lddv + head * D, g);
        }
    }
    if ((int)blockIdx.x * 32 * NWF >= (z == 0 ? Lq : Lk)) return;              // workgroup-uniform, before any barrier
    if (z == 0) bwd_q_body<TB>(lds, qg, ldq, kg, ldk, vg, ldv, o, dO, lse, dq, lddq, Sq, Sk, Lq, Lk, nh, scale);
    else bwd_kv_body<TB>(lds, stat, qg, ldq, kg, ldk, vg, ldv, o, dO, lse, dk, lddk, dv, lddv, Sq, Sk, Lq, Lk, nh, scale);
}
}  // namespace flash


// ------------------------------------------------------------------------------------------------------------ launches
struct Operands {
    const float *q, *k, *v;
    long ldq, ldk, ldv;
    int N, Lq, Lk, nh;
    float scale;
};

template <bool LENS>
void launch_fwd_t(const Operands& a, float* o, float* lse, bool mfma, bool key_split, const int32_t* lens, hipStream_t st) {
    const dim3 grid((a.Lq + 63) / 64, a.N * a.nh);
    if (mfma && key_split)
        hipLaunchKernelGGL(flash::fwd_ks_kernel<LENS>, grid, dim3(2 * flash::NTF), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, o, lse, a.Lq, a.Lk, a.nh,
                           a.scale, lens);
    else if (mfma)
        hipLaunchKernelGGL(flash::fwd_kernel<LENS>, grid, dim3(flash::NTF), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, o, lse, a.Lq, a.Lk, a.nh,
                           a.scale, lens);
    else
        hipLaunchKernelGGL(mha_fwd_kernel<LENS>, grid, dim3(256), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, o, lse, a.Lq, a.Lk, a.nh, a.scale, lens);
}

// lens (device, [N]; only with Lq == Lk): the per-image bound of cdetr_mha_*_lens; nullptr = the dense kernels
void launch_fwd(const Operands& a, float* o, float* lse, bool mfma, bool key_split, hipStream_t st, const int32_t* lens = nullptr) {
    if (lens) launch_fwd_t<true>(a, o, lse, mfma, key_split, lens, st);
    else launch_fwd_t<false>(a, o, lse, mfma, key_split, nullptr, st);
}

// tb: 0 = the two fp32 VALU launches (D through `work`), 3 / 1 = one flash::bwd_kernel launch with split-bf16 / plain-bf16 gradient contractions
template <bool LENS>
void launch_bwd_t(const Operands& a, const float* o, const float* d_o, const float* lse, float* dq, long lddq, float* dk, long lddk, float* dv,
                  long lddv, float* work, int tb, bool two_launches, const int32_t* lens, hipStream_t st) {
    const int gq = (a.Lq + 63) / 64, gk = (a.Lk + 63) / 64, nb = a.N * a.nh;
    if (tb == 0) {
        hipLaunchKernelGGL(mha_bwd_q_kernel<LENS>, dim3(gq, nb), dim3(256), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, o, d_o, lse, dq, lddq, work,
                           a.Lq, a.Lk, a.nh, a.scale, lens);
        hipLaunchKernelGGL(mha_bwd_kv_kernel<LENS>, dim3(gk, nb), dim3(256), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, d_o, lse, work, dk, lddk,
                           dv, lddv, a.Lq, a.Lk, a.nh, a.scale, lens);
        return;
    }
    auto kern = (tb == 1) ? flash::bwd_kernel<1, LENS> : flash::bwd_kernel<3, LENS>;
    if (two_launches) {
        hipLaunchKernelGGL(kern, dim3(gq, nb, 1), dim3(flash::NTF), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, o, d_o, lse, dq, lddq, dk, lddk,
                           dv, lddv, a.Lq, a.Lk, a.nh, a.scale, 0, lens);
        hipLaunchKernelGGL(kern, dim3(gk, nb, 1), dim3(flash::NTF), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, o, d_o, lse, dq, lddq, dk, lddk,
                           dv, lddv, a.Lq, a.Lk, a.nh, a.scale, 1, lens);
    } else {
        hipLaunchKernelGGL(kern, dim3(max(gq, gk), nb, 2), dim3(flash::NTF), 0, st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, o, d_o, lse, dq, lddq,
                           dk, lddk, dv, lddv, a.Lq, a.Lk, a.nh, a.scale, 0, lens);
    }
}

void launch_bwd(const Operands& a, const float* o, const float* d_o, const float* lse, float* dq, long lddq, float* dk, long lddk, float* dv,
                long lddv, float* work, int tb, bool two_launches, hipStream_t st, const int32_t* lens = nullptr) {
    if (lens) launch_bwd_t<true>(a, o, d_o, lse, dq, lddq, dk, lddk, dv, lddv, work, tb, two_launches, lens, st);
    else launch_bwd_t<false>(a, o, d_o, lse, dq, lddq, dk, lddk, dv, lddv, work, tb, two_launches, nullptr, st);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int cdetr_mha_fwd(const float* qk, const float* v, float* o, float* lse, int32_t N, int32_t L, int32_t nh, float scale,
                             int32_t precision, void* stream) {
    CDETR_CHECK_ARG(qk && v && o && lse && N > 0 && L > 0 && nh > 0, "cdetr_mha_fwd: bad args");
    const long E = (long)nh * D;
    const Operands a{qk, qk + E, v, 2 * E, 2 * E, E, N, L, L, nh, scale};
    // the keys of a query tile cut in two (fwd_ks_kernel) from 128 keys on; two waves walking all key tiles cost the step 0.03 ms in three of three
    // rounds (profiles/r5_ab_tail_wgrad.txt)
    const bool mfma = precision == 1;
    launch_fwd(a, o, lse, mfma, mfma && L >= 128, reinterpret_cast<hipStream_t>(stream));
    return cdetr_launch_status("cdetr_mha_fwd");
}

extern "C" int cdetr_mha_bwd(const float* qk, const float* v, const float* o, const float* d_o, const float* lse, float* d_qk,
                             float* d_v, float* work, int32_t N, int32_t L, int32_t nh, float scale, int32_t precision, void* stream) {
    CDETR_CHECK_ARG(qk && v && o && d_o && lse && d_qk && d_v && work && N > 0 && L > 0 && nh > 0, "cdetr_mha_bwd: bad args");
    const long E = (long)nh * D;
    const Operands a{qk, qk + E, v, 2 * E, 2 * E, E, N, L, L, nh, scale};
    // precision 3: split-bf16 scores, plain-bf16 gradient contractions (flash::bwd_q_body); 1: split-bf16 throughout; else fp32
    const int tb = precision == 3 ? 1 : precision == 1 ? 3 : 0;
    launch_bwd(a, o, d_o, lse, d_qk, 2 * E, d_qk + E, 2 * E, d_v, E, work, tb, false, reinterpret_cast<hipStream_t>(stream));
    return cdetr_launch_status("cdetr_mha_bwd");
}

// The ragged form: the same kernels (their LENS instantiations), the same kernel choice by L -- the host never sees the lengths.
extern "C" int cdetr_mha_fwd_lens(const float* qk, const float* v, const int32_t* lens, float* o, float* lse, int32_t N, int32_t L, int32_t nh,
                                  float scale, int32_t precision, void* stream) {
    CDETR_CHECK_ARG(qk && v && lens && o && lse, "cdetr_mha_fwd_lens: null pointer");
    CDETR_CHECK_ARG(N > 0 && L > 0 && nh > 0, "cdetr_mha_fwd_lens: bad sizes (N %d, L %d, nh %d)", N, L, nh);
    CDETR_CHECK_ARG(aligned16(qk) && aligned16(v) && aligned16(o), "cdetr_mha_fwd_lens: operands must be 16-byte aligned");
    const long E = (long)nh * D;
    const Operands a{qk, qk + E, v, 2 * E, 2 * E, E, N, L, L, nh, scale};
    const bool mfma = precision == 1;
    launch_fwd(a, o, lse, mfma, mfma && L >= 128, reinterpret_cast<hipStream_t>(stream), lens);
    return cdetr_launch_status("cdetr_mha_fwd_lens");
}

extern "C" int cdetr_mha_bwd_lens(const float* qk, const float* v, const int32_t* lens, const float* o, const float* d_o, const float* lse,
                                  float* d_qk, float* d_v, float* work, int32_t N, int32_t L, int32_t nh, float scale, int32_t precision,
                                  void* stream) {
    CDETR_CHECK_ARG(qk && v && lens && o && d_o && lse && d_qk && d_v && work, "cdetr_mha_bwd_lens: null pointer");
    CDETR_CHECK_ARG(N > 0 && L > 0 && nh > 0, "cdetr_mha_bwd_lens: bad sizes (N %d, L %d, nh %d)", N, L, nh);
    CDETR_CHECK_ARG(aligned16(qk) && aligned16(v) && aligned16(o) && aligned16(d_o) && aligned16(d_qk) && aligned16(d_v),
                    "cdetr_mha_bwd_lens: operands must be 16-byte aligned");
    const long E = (long)nh * D;
    const Operands a{qk, qk + E, v, 2 * E, 2 * E, E, N, L, L, nh, scale};
    const int tb = precision == 3 ? 1 : precision == 1 ? 3 : 0;
    launch_bwd(a, o, d_o, lse, d_qk, 2 * E, d_qk + E, 2 * E, d_v, E, work, tb, false, reinterpret_cast<hipStream_t>(stream), lens);
    return cdetr_launch_status("cdetr_mha_bwd_lens");
}

// Forward kernel choice for the general problem: the key split (fwd_ks_kernel) from 128 keys on, as for cdetr_mha_fwd.  Measured at N = 2,
// nh = 8 (tools/attn_ab.py, median of 50 launches, fwd_kernel -> fwd_ks_kernel): 300 x 864 keys 43 -> 31 us, 300 x 2500 99 -> 61, 900 x 2500
// 102 -> 65, 2500 x 2500 153 -> 133: with up to 40 query tiles per (image, head) the grid still leaves the chip half empty or runs one round
// of waves, and halving each wave's chain of key tiles wins at every size the variant meets.  The backward's one launch (bwd_kernel, grid
// as wide as the longer side) against two exactly sized launches: 300 x 864 81 vs 98 us, 900 x 2500 190 vs 234, 2500 x 2500 385 vs 478 --
// one launch lets the query and key halves share the chip.
static bool attn_key_split(int Lk) { return Lk >= 128; }

static int attn_check(const cdetr_attn_desc* d, const char* what) {
    CDETR_CHECK_ARG(d && d->q && d->k && d->v && d->o && d->lse && d->N > 0 && d->Lq > 0 && d->Lk > 0 && d->nh > 0, "%s: bad args", what);
    const long E = (long)d->nh * D;
    CDETR_CHECK_ARG(d->ldq >= E && d->ldk >= E && d->ldv >= E && d->ldq % 4 == 0 && d->ldk % 4 == 0 && d->ldv % 4 == 0,
                    "%s: row strides must be multiples of 4 floats and at least nh * 32", what);
    CDETR_CHECK_ARG(aligned16(d->q) && aligned16(d->k) && aligned16(d->v) && aligned16(d->o), "%s: operands must be 16-byte aligned", what);
    CDETR_CHECK_ARG(d->precision == 0 || d->precision == 1 || d->precision == 3, "%s: precision must be 0, 1 or 3", what);
    return 0;
}

extern "C" int cdetr_attn_fwd(const cdetr_attn_desc* d, void* stream) {
    if (int rc = attn_check(d, "cdetr_attn_fwd")) return rc;
    const Operands a{d->q, d->k, d->v, d->ldq, d->ldk, d->ldv, d->N, d->Lq, d->Lk, d->nh, d->scale};
    const bool mfma = d->precision != 0;
    launch_fwd(a, d->o, d->lse, mfma, mfma && attn_key_split(d->Lk), reinterpret_cast<hipStream_t>(stream));
    return cdetr_launch_status("cdetr_attn_fwd");
}

extern "C" int cdetr_attn_bwd(const cdetr_attn_desc* d, void* stream) {
    if (int rc = attn_check(d, "cdetr_attn_bwd")) return rc;
    const long E = (long)d->nh * D;
    CDETR_CHECK_ARG(d->d_o && d->d_q && d->d_k && d->d_v && (d->precision != 0 || d->work), "cdetr_attn_bwd: bad args");
    CDETR_CHECK_ARG(d->ld_dq >= E && d->ld_dk >= E && d->ld_dv >= E && d->ld_dq % 4 == 0 && d->ld_dk % 4 == 0 && d->ld_dv % 4 == 0 &&
                    aligned16(d->d_o) && aligned16(d->d_q) && aligned16(d->d_k) && aligned16(d->d_v),
                    "cdetr_attn_bwd: gradient row strides must be multiples of 4 floats and at least nh * 32, gradients 16-byte aligned");
    static const int two = getenv("CDETR_ATTN_BWD_TWO_LAUNCHES") ? atoi(getenv("CDETR_ATTN_BWD_TWO_LAUNCHES")) : 0;   // A/B
    const Operands a{d->q, d->k, d->v, d->ldq, d->ldk, d->ldv, d->N, d->Lq, d->Lk, d->nh, d->scale};
    const int tb = d->precision == 3 ? 1 : d->precision == 1 ? 3 : 0;
    launch_bwd(a, d->o, d->d_o, d->lse, d->d_q, d->ld_dq, d->d_k, d->ld_dk, d->d_v, d->ld_dv, d->work, tb, two != 0, reinterpret_cast<hipStream_t>(stream));
    return cdetr_launch_status("cdetr_attn_bwd");
}
