// Image batches prepared on the device (counting_detr_amd/data.py: collate_raw -> Prefetcher -> ops.image_prep).
//
// cdetr_image_prep: the un-resized uint8 RGB pixels of a batch -> the fp32 image [B][3][Hm][Wm] and the padding mask [B][Hm][Wm] that
// data.collate builds on the host from PIL's resize + to_normalized_tensor, BIT FOR BIT, in one launch.
//
// Pillow's 8-bit resampler is integer arithmetic, so there is nothing to round differently: per axis a table of int32 coefficients
// (22 fractional bits, built on the host by data.resample_tables with Pillow's own rules), per pass acc = 2^21 + sum pixel * k in int32,
// >> 22, clamp to 0..255; horizontal pass first into uint8, the vertical pass over that.  The normalisation is a 768-entry fp32 table
// the host fills with to_normalized_tensor's own expressions: no division, no FMA question on the device.
//
// One workgroup = one TH x TW tile of the PADDED output of one image.  It stages the tile's columns of every input row the tile's
// vertical taps reach, horizontally resampled, in LDS as three uint8 planes (a row of a plane = TW bytes = the 4-byte words the
// vertical pass reads), runs the vertical pass from LDS, and stores planar fp32 as 16-byte vectors, the mask as 4-byte words.  Every
// byte of image and mask is written by exactly one thread: padding gets 0.0f / 1, no fill launch is needed.
//
// Nothing read from device memory is trusted with an address: the per-image records and every (first, count) pair of the tables are
// checked or clamped against the buffer sizes of the descriptor before they index anything (a bad record yields padding for that
// image, never an out-of-bounds access).  What the tile can hold -- IMAGE_PREP_MAX_TAPS taps per output sample, IMAGE_PREP_MAX_ROWS
// staged rows per TH output rows -- bounds the supported DOWNSCALE at 4x per axis (bicubic: 17 taps, 141 rows); upscales of any
// factor fit.  data.collate_raw resizes anything beyond that on the host and passes it on with identity tables.
#include "common.h"
#include "../../include/cdetr_hip.h"

namespace {

constexpr int TH = CDETR_IMAGE_PREP_TILE_H, TW = CDETR_IMAGE_PREP_TILE_W;
constexpr int KMAX = CDETR_IMAGE_PREP_MAX_TAPS, RMAX = CDETR_IMAGE_PREP_MAX_ROWS;
constexpr int REC = CDETR_IMAGE_PREP_RECORD_INTS;
constexpr int NT = 256;
constexpr int PREC = 22;                   // Pillow's PRECISION_BITS = 32 - 8 - 2
static_assert(TW % 4 == 0 && (TH * (TW / 4)) % NT == 0, "tile / workgroup shapes");

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PREC, 0), 255); }

__global__ __launch_bounds__(NT) void image_prep_kernel(cdetr_image_prep_desc p, int tiles_x) {
    __shared__ __attribute__((aligned(16))) uint8_t s_mid[3][RMAX][TW];      // horizontally resampled rows, one plane per channel
    __shared__ int s_hc[TW][KMAX], s_vc[TH][KMAX];
    __shared__ int s_hmin[TW], s_hcnt[TW], s_vmin[TH], s_vcnt[TH];
    __shared__ float s_lut[768];

    const int b = blockIdx.y, tid = threadIdx.x;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const int Hm = p.Hm, Wm = p.Wm;

    // the image's record (block-uniform): [pixel offset in bytes, in_h, in_w, out_h, out_w, h bounds, h coeffs, h taps, v bounds, v coeffs, v taps, 0]
    const int32_t* rec = p.images + (size_t)b * REC;
    const int64_t pix_off = rec[0];
    const int in_h = rec[1], in_w = rec[2], out_h = rec[3], out_w = rec[4];
    const int hb = rec[5], hc = rec[6], hk = rec[7], vb = rec[8], vc = rec[9], vk = rec[10];
    bool ok = pix_off >= 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0 && out_h <= Hm && out_w <= Wm &&
              pix_off + (int64_t)in_h * in_w * 3 <= p.pixel_bytes && hk >= 1 && hk <= KMAX && vk >= 1 && vk <= KMAX && hb >= 0 && hc >= 0 &&
              vb >= 0 && vc >= 0 && (int64_t)hb + 2 * (int64_t)out_w <= p.table_ints && (int64_t)hc + (int64_t)out_w * hk <= p.table_ints &&
              (int64_t)vb + 2 * (int64_t)out_h <= p.table_ints && (int64_t)vc + (int64_t)out_h * vk <= p.table_ints;
    const int nx = ok ? min(max(out_w - x0, 0), TW) : 0;        // image (not padding) columns / rows of this tile
    const int ny = ok ? min(max(out_h - y0, 0), TH) : 0;
    int r0 = 0, nrows = 0;
    if (nx > 0 && ny > 0) {
        const int first = p.tables[vb + 2 * y0], last = p.tables[vb + 2 * (y0 + ny - 1)], last_n = p.tables[vb + 2 * (y0 + ny - 1) + 1];
        r0 = first;
        nrows = last + last_n - first;
        if (first < 0 || last_n < 0 || nrows <= 0 || nrows > RMAX || (int64_t)first + nrows > in_h) nrows = 0;
    }
    const bool work = nrows > 0;                                 // block-uniform: every barrier below is reached by all or by none

    if (work) {
        for (int i = tid; i < 768; i += NT) s_lut[i] = p.lut[i];
        for (int j = tid; j < nx; j += NT) {                     // (first, count) of the tile's columns, forced inside the source row
            int c = p.tables[hb + 2 * (x0 + j) + 1], m = p.tables[hb + 2 * (x0 + j)];
            c = min(max(c, 0), min(hk, in_w));
            s_hcnt[j] = c;
            s_hmin[j] = min(max(m, 0), in_w - c);
        }
        for (int i = tid; i < nx * hk; i += NT) s_hc[i / hk][i % hk] = p.tables[hc + (size_t)(x0 + i / hk) * hk + i % hk];
        for (int j = tid; j < ny; j += NT) {                     // ... of its rows, relative to the first staged row, forced inside the stage
            int c = p.tables[vb + 2 * (y0 + j) + 1], m = p.tables[vb + 2 * (y0 + j)] - r0;
            c = min(max(c, 0), min(vk, nrows));
            s_vcnt[j] = c;
            s_vmin[j] = min(max(m, 0), nrows - c);
        }
        for (int i = tid; i < ny * vk; i += NT) s_vc[i / vk][i % vk] = p.tables[vc + (size_t)(y0 + i / vk) * vk + i % vk];
        __syncthreads();

        // horizontal pass: source rows r0 .. r0 + nrows, the tile's nx columns, three channels per thread
        const uint8_t* src0 = p.pixels + pix_off;
        for (int i = tid; i < nrows * TW; i += NT) {
            const int r = i / TW, j = i % TW;
            uint8_t o0 = 0, o1 = 0, o2 = 0;
            if (j < nx) {
                const int n = s_hcnt[j];
                const uint8_t* s = src0 + ((size_t)(r0 + r) * in_w + s_hmin[j]) * 3;
                int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
                for (int k = 0; k < n; ++k) {
                    const int c = s_hc[j][k];
                    a0 += (int)s[3 * k] * c;
                    a1 += (int)s[3 * k + 1] * c;
                    a2 += (int)s[3 * k + 2] * c;
                }
                o0 = (uint8_t)clip8(a0); o1 = (uint8_t)clip8(a1); o2 = (uint8_t)clip8(a2);
            }
            s_mid[0][r][j] = o0; s_mid[1][r][j] = o1; s_mid[2][r][j] = o2;
        }
        __syncthreads();
    }

    // vertical pass + normalisation + stores: a thread owns four consecutive columns of one row of one plane
    const bool vec = (Wm & 3) == 0;                              // rows of the outputs start on 16-byte (image) / 4-byte (mask) boundaries
    for (int i = tid; i < 3 * TH * (TW / 4); i += NT) {
        const int ch = i / (TH * (TW / 4)), y = (i / (TW / 4)) % TH, xq = (i % (TW / 4)) * 4;
        const int gy = y0 + y, gx = x0 + xq;
        if (gy >= Hm || gx >= Wm) continue;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (work && y < ny && xq < nx) {
            const int n = s_vcnt[y], m = s_vmin[y];
            int a[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
            for (int k = 0; k < n; ++k) {
                const int c = s_vc[y][k];
                const uint32_t w = *reinterpret_cast<const uint32_t*>(&s_mid[ch][m + k][xq]);
                a[0] += (int)(w & 255u) * c;
                a[1] += (int)((w >> 8) & 255u) * c;
                a[2] += (int)((w >> 16) & 255u) * c;
                a[3] += (int)(w >> 24) * c;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (xq + q < nx) v[q] = s_lut[ch * 256 + clip8(a[q])];
        }
        float* dst = p.image + (((size_t)b * 3 + ch) * Hm + gy) * Wm + gx;
        if (vec) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (gx + q < Wm) dst[q] = v[q];
        }
    }
    for (int i = tid; i < TH * (TW / 4); i += NT) {
        const int y = i / (TW / 4), xq = (i % (TW / 4)) * 4;
        const int gy = y0 + y, gx = x0 + xq;
        if (gy >= Hm || gx >= Wm) continue;
        uint8_t m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = !(work && y < ny && xq + q < nx);
        uint8_t* dst = p.mask + ((size_t)b * Hm + gy) * Wm + gx;
        if (vec) {
            *reinterpret_cast<uint32_t*>(dst) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (gx + q < Wm) dst[q] = m[q];
        }
    }
}

}  // namespace

extern "C" int cdetr_image_prep(const cdetr_image_prep_desc* d, void* stream) {
    CDETR_CHECK_ARG(d != nullptr, "cdetr_image_prep: null descriptor");
    CDETR_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->Hm > 0 && d->Wm > 0 && (int64_t)d->Hm * d->Wm < ((int64_t)1 << 31),
                    "cdetr_image_prep: bad sizes B = %d, Hm = %d, Wm = %d", d->B, d->Hm, d->Wm);
    CDETR_CHECK_ARG(d->pixel_bytes > 0 && d->table_ints > 0 && d->pixel_bytes < ((int64_t)1 << 31) && d->table_ints < ((int64_t)1 << 31),
                    "cdetr_image_prep: bad buffer sizes, %lld pixel bytes, %lld table entries (both must be in 1 .. 2^31 - 1)",
                    (long long)d->pixel_bytes, (long long)d->table_ints);
    CDETR_CHECK_ARG(d->pixels && d->images && d->tables && d->lut && d->image && d->mask, "cdetr_image_prep: null pointer");
    CDETR_CHECK_ARG(((uintptr_t)d->image & 15) == 0 && ((uintptr_t)d->mask & 3) == 0, "cdetr_image_prep: image must be 16-byte and mask 4-byte aligned");
    if (d->max_taps > KMAX || d->max_rows > RMAX) {
        cdetr_set_error("cdetr_image_prep: %d taps per sample / %d staged rows per %d output rows exceed the tile (%d / %d): downscales beyond 4x "
                        "are resized on the host (data.collate_raw)", d->max_taps, d->max_rows, TH, KMAX, RMAX);
        return CDETR_ERR_UNSUPPORTED;
    }
    CDETR_CHECK_ARG(d->max_taps >= 1 && d->max_rows >= 1, "cdetr_image_prep: max_taps = %d, max_rows = %d must be positive", d->max_taps, d->max_rows);
    const int tiles_x = (d->Wm + TW - 1) / TW, tiles_y = (d->Hm + TH - 1) / TH;
    hipLaunchKernelGGL(image_prep_kernel, dim3(tiles_x * tiles_y, d->B), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), *d, tiles_x);
    return cdetr_launch_status("cdetr_image_prep");
}
