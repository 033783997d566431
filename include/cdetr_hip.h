/* cdetr_hip.h -- C-ABI of libcdetr_hip.so: the MI355X (gfx950) kernels of the Counting-DETR hot path.
 *
 * The reference (VinAIResearch/Counting-DETR) is pure Python/PyTorch and has NO FFI of its own; each entry
 * point below replaces the torch-op sequence at the cited reference lines (A2/ = src/CountDETR_147_2nd_stage/,
 * A1/ = src/CountDETR_147_1st_stage/: cdetr_bbox_criterion_fwd / _bwd, the 1st stage's BoundingBoxCriterion).
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add at each site.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (cdetr_last_error() gives the thread-local message);
 *     nothing throws across the boundary;
 *   - every buffer is DEVICE memory allocated by the caller (torch caching allocator); the library never
 *     allocates, never synchronises, holds no mutable global state (re-entrant: it is called from the Python main
 *     thread in forward and from the autograd engine thread in backward);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); kernels are async;
 *   - all tensors are fp32 unless stated; activations are NHWC / row-major [rows][channels];
 *   - arithmetic: fp32 MFMA (v_mfma_f32_32x32x2_f32) -- exact fp32 products, fp32 accumulation.
 */
#ifndef CDETR_HIP_H
#define CDETR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDETR_ABI_VERSION 2

/* row-gather modes of cdetr_conv_geom */
#define CDETR_ROWS_DENSE 0      /* row(m) = m (linear layers, 1x1 stride-1 convs) */
#define CDETR_ROWS_CONV_FWD 1   /* m = output pixel; tap (ky,kx) -> input pixel (zero outside) */
#define CDETR_ROWS_CONV_DGRAD 2 /* m = input pixel;  tap (ky,kx) -> output pixel feeding it (transposed conv) */

typedef struct {
    int32_t mode;
    int32_t Ha, Wa; /* spatial dims of the GATHERED tensor: its row index is (n*Ha + y)*Wa + x            */
    int32_t Hc, Wc; /* spatial dims of the enumerated row space (m = (n*Hc + y)*Wc + x)                    */
    int32_t kh, kw, stride, pad, dil;
} cdetr_conv_geom;

/* C[m][n] = epilogue( sum_tap sum_k A[row(m,tap)][k] * Wt(n,tap,k) )
 * b_layout 0 : Wt(n,tap,k) = B[n*ldb + tap*K + k]          (weight [N][taps][K], k contiguous; forward)
 * b_layout 1 : Wt(n,tap,k) = B[(k*taps + tap)*ldb + n]     (weight [K][taps][N], n contiguous; data-gradient)
 * epilogue   : v = acc (+ bias[n]); v *= out_scale; v += resid[m][n]; if gate: v = gate[m][n] > 0 ? v : 0;
 *              if relu: v = max(v, 0)
 * w_scale    : optional per-output-channel scale of the WEIGHT (frozen-BN fold): index n for b_layout 0,
 *              index k for b_layout 1.
 * Replaces: F.conv2d + FrozenBatchNorm2d + ReLU (+residual) A2/models/resnet.py:140-160, backbone.py:50-60;
 *           F.linear at A2/models/row_column_decoupled_attention.py:165-208,311, transformer.py:412-439; and
 *           their autograd data-gradients.                                                                    */
typedef struct {
    int32_t M, N, K, taps;
    int32_t batch; /* grid.z; per-batch element strides sA/sB/sC (0 = shared); see batch_inner for two-level batches */
    int32_t b_layout;
    int32_t relu;
    int32_t precision; /* 0 = fp32 MFMA (exact fp32 products), 1 = split-bf16 x3 on the bf16 matrix pipe (~1e-5 rel);
                          2 = "bf16x2": B rounded to bf16, A split hi+lo, 2 MFMAs per product (~2^-9 rel per product, random);
                          3 = plain bf16: both operands rounded, 1 MFMA.  2 / 3 are meant for the BACKWARD passes (data / weight
                          gradients); kernels without a reduced-term form (few-row GEMMs, n-contiguous operands) run them as 1. */
    float out_scale;
    const float* A; int64_t lda, sA; /* A may be NULL under the same conditions as C below (the operand exists as its bf16 twin A16 only) */
    const float* B; int64_t ldb, sB;
    float* C; int64_t ldc, sC; /* C may be NULL when C16 is given and the operands are in the direct-to-LDS kernel's formats (A16, B16 or
                                * B_split, K % 64 == 0, 16-byte aligned): only the bf16 copy is written -- an inner activation gradient of
                                * a bottleneck is read by nothing but the next bf16 contractions */
    const float* w_scale;
    const float* bias;
    const float* resid; int64_t ldr;
    const float* gate; int64_t ldg;
    cdetr_conv_geom g;
    const void* B_split; /* optional (NULL = absent), b_layout 0 + precision 1 + batch 1 only: the SAME operand pre-split for the
                          * bf16x3 kernels, w_scale already folded in: row n = [taps*K/32 groups][hi 32 bf16 | lo 32 bf16], i.e.
                          * the byte offsets of (n, tap, k-group) equal those of the fp32 operand (ldb applies unchanged);
                          * written by cdetr_weight_mirror.  Kernels that cannot use it read B / w_scale instead.          */
    int32_t batch_inner; /* 0: batch item z sits at z*s.  > 0: z = outer*batch_inner + inner sits at inner*s + outer*s2      */
    int32_t flags;       /* (e.g. heads inside images: one launch for the per-head GEMMs of every image)
                          * flags: CDETR_GEMM_A_GROUPS / CDETR_GEMM_C_GROUPS below (0 = none)                                       */
    int64_t sA2, sB2, sC2;
    const void* A16;     /* optional: a bf16 TWIN of A (same lda / batch strides, in elements): with precision 3 the tile kernels read it
                          * instead of A -- half the operand bytes, no conversion at staging.  Needs lda and the strides to be multiples
                          * of 8 and a 16-byte aligned base; other kernel classes read A.                                             */
    void* C16;           /* optional (NULL = absent): a bf16 TWIN of C written by the same epilogue (same ldc / batch strides, in
                          * elements) -- the operand format of the plain-bf16 weight gradients (cdetr_wgrad_desc.dY16 / X16).      */
    void* splitk_ws;     /* optional (NULL = never split): device scratch that lets the tile kernels split the reduction of a problem with
                          * too few output tiles to fill 256 CUs (two images per GPU: 5000 rows x 256 channels = 158 workgroups) across
                          * 2-4 workgroups per tile; the partial tiles meet here and the last workgroup to arrive adds them IN SLICE ORDER
                          * (deterministic) and runs the fused epilogue.  Layout: [4096 int32 arrival counters | partial tiles]; the caller
                          * zeroes the counters ONCE (every call leaves them zero) and must not share one scratch between streams that
                          * may run cdetr_gemm concurrently.  16-byte aligned.
                          * ORDERING IS gfx950-SPECIFIC, not a HIP memory-model guarantee: the partial tiles travel as RELAXED agent-scope
                          * atomic stores / loads (sc1: they bypass the XCD-private L2s), `s_waitcnt vmcnt(0)` + the workgroup barrier put
                          * them before the relaxed agent-scope counter RMW.  An acquire / release pair would be the portable form and costs
                          * a write-back + invalidate of a whole 4 MiB L2 per workgroup (+80 us per launch when measured); the same
                          * protocol serves cdetr_gemm_dl's split form and cdetr_rcda_fwd_desc.ws.  tools/splitk_stress.py (4000 launches,
                          * bit-identical results, counters back at zero) is the regression check to re-run after a compiler / runtime
                          * update.                                                                                                  */
    int64_t splitk_ws_bytes; /* size of splitk_ws in bytes (>= 16 KiB + partial tiles; too small = fewer slices or none)            */
    const void* A16lo;   /* optional: the LO plane of A's split-bf16 form, lo = bf16(A - float(A16)) (same shape / strides as A16).  With
                          * A16 + A16lo + B_split the split-bf16 x3 product (precision 1) needs no conversion at all: the direct-to-LDS
                          * tile kernel (igemm_dl_kernel) copies operand tiles HBM -> LDS with global_load_lds and feeds the matrix
                          * pipe from there.  Same arithmetic as splitting the fp32 operand at staging (bit-identical products).       */
    const void* B16;     /* optional, b_layout 0: bf16(B * w_scale), same [N][taps*K] shape and ldb (in elements): what the plain-bf16
                          * (precision 3) direct-to-LDS kernel streams instead of the hi halves of B_split's interleaved groups.   */
    const void* gate16;  /* optional: bf16 twin of `gate` (same ldg, in elements): the direct-to-LDS kernel tests its sign instead of the fp32
                          * tensor's (bf16 rounding keeps sign and zero: the ReLU mask is identical) -- half the bytes of the epilogue's
                          * largest read in the backbone's data gradients.  `gate` must still be given (other kernel classes read it).  */
    void* C16lo;         /* optional: the LO plane of C written by the same epilogue, C16lo = bf16(C - float(C16)) (needs C16): the
                          * next layer's A16lo.  C itself may then be NULL when no consumer reads the fp32 tensor.                     */
} cdetr_gemm_desc;
/* cdetr_gemm_desc.flags (direct-to-LDS kernel, precision 1):
 * CDETR_GEMM_A_GROUPS: A16 holds A pre-split in INTERLEAVED groups, the format of B_split -- row m = [K/32 groups][hi 32 bf16 | lo 32 bf16],
 *   i.e. the byte offset of (m, k-group) equals that of the fp32 operand (lda applies unchanged, 4 bytes per element; lda % 32 == 0; A16lo
 *   unused).  A k-tile of the kernel is then ONE full 128-byte line per row; with the planes A16 / A16lo it is two half lines.
 * CDETR_GEMM_C_GROUPS: C16lo receives C in the same interleaved form ([N/32 groups][hi 32 | lo 32] per row, ldc applies unchanged,
 *   N % 32 == 0, ldc % 32 == 0) -- the next layer's grouped A operand; C16 (the plain hi twin) stays optional.                       */
#define CDETR_GEMM_A_GROUPS 1
#define CDETR_GEMM_C_GROUPS 2
/* CDETR_GEMM_PRIO: the launch's waves run at raised instruction priority (s_setprio): for launches of a step's MAIN chain that share the
 *   chip with another stream's throughput work (the backbone's data gradients beside the weight gradients); results are unaffected.   */
#define CDETR_GEMM_PRIO 4
/* CDETR_GEMM_RESID_GROUPS: `resid` points to a tensor in the interleaved-group form (what CDETR_GEMM_C_GROUPS wrote: a bottleneck's output kept
 *   ONCE as [hi 32 | lo 32] groups instead of fp32 + twin); ldr applies unchanged (4 bytes per element), ldr % 32 == 0, N % 32 == 0; the epilogue
 *   adds hi + lo.  Direct-to-LDS kernel only, like the other two group flags.                                                          */
#define CDETR_GEMM_RESID_GROUPS 8
/* CDETR_GEMM_GATE16_ONLY: `gate` is NOT an fp32 tensor (the gating activation exists as interleaved groups + its twin): only gate16 may be read,
 *   i.e. the problem must run on the direct-to-LDS kernel (CDETR_ERR_ARG otherwise); `gate` must still be non-NULL (it switches the gate on).  */
#define CDETR_GEMM_GATE16_ONLY 16
int cdetr_gemm(const cdetr_gemm_desc* d, void* stream);
/* The direct-to-LDS tile kernel (csrc/igemm_dl.hip) with an explicit configuration -- what cdetr_gemm picks by itself for problems
 * whose operands are given pre-split (A16 [+ A16lo] and B_split); for tests and tile sweeps.  tile: 0 = 128x128, 1 = 128x64,
 * 2 = 64x128, 3 = 64x64 (rows x channels per workgroup); stages: LDS ring depth 2..4 (3 for tile 0), or 13 = the halo-resident form for
 * stride-1 3x3 rows with pad == dil over a same-size map (forward or data-gradient rows; the pixel rows around a tile are staged once per
 * channel chunk, the nine taps read them at row offsets; <= 448 halo rows, <= 160 KB of LDS), or 200 + 10 * slices + ring depth (2 | 3) =
 * the reduction of every output tile cut into 2..8 slices (grid.y): each slice parks its partial tile in cdetr_gemm_desc.splitk_ws
 * (4096 arrival counters + tiles * slices * tile bytes), the slice that arrives last adds the partials in slice order and runs the
 * fused epilogue (bit-identical whichever slice that is; needs slices <= k-tiles).  CDETR_ERR_UNSUPPORTED when the
 * operand formats / alignment do not allow it (cdetr_last_error says why).                                                        */
int cdetr_gemm_dl(const cdetr_gemm_desc* d, int32_t tile, int32_t stages, void* stream);
/* n INDEPENDENT GEMMs submitted together (same results as n cdetr_gemm calls; no problem may read another's output).  Few-row
 * problems and the 64x128-tile class with a pre-split weight run as grouped launches (one kernel for up to 12 problems).
 * Replaces: sibling F.linear calls on independent inputs, e.g. the five in-projections of
 * A2/models/row_column_decoupled_attention.py:165-208 and the memory-side projections of all decoder layers.               */
int cdetr_gemm_group(const cdetr_gemm_desc* descs, int32_t n, void* stream);

/* dW[i][tap][c] += w_scale[i] * sum_p dY[p][i] * X[row(p,tap)][c]      (weight-gradient, split-K + fp32 atomics)
 * dbias[i]      += sum_p dY[p][i]                                       (optional, fused: NULL = skip)
 * Replaces: autograd of F.conv2d / F.linear w.r.t. weight and bias.  dW / dbias must hold the value to accumulate
 * onto (the caller zeroes the gradient arena once per step).                                                  */
typedef struct {
    int32_t P, Nout, Cin, taps;
    int32_t batch;
    int32_t precision; /* as in cdetr_gemm_desc */
    const float* dY; int64_t ldy, sY;
    const float* X; int64_t ldx, sX;
    float* dW; int64_t ldw, sW;
    const float* w_scale;
    float* dbias;
    cdetr_conv_geom g; /* mode DENSE or CONV_FWD (p = output pixel) */
    int32_t batch_inner; /* two-level batch, as in cdetr_gemm_desc */
    int32_t wg_target;   /* 0 = default.  > 0: the number of workgroups the launch (for cdetr_wgrad_group: the grouped launch this problem   */
                         /* becomes part of -- the largest request of its members) should spread its pixel slices over.  The default (768 = 3  */
                         /* per CU; 384 for a single weight of <= 16 tiles) suits a launch that has the chip to itself; a caller that runs the  */
                         /* launch BESIDE another stream's chain asks for 384 (fewer, longer workgroups disturb the chain less), the step's     */
                         /* last weight gradients for several thousand.  Results do not depend on it beyond fp32 summation order.               */
    int64_t sY2, sX2, sW2;
    const void* dY16;  /* optional bf16 TWINS of dY / X (same shapes, leading dimensions and batch strides, in elements): with        */
    const void* X16;   /* precision 3 (plain bf16) the kernel reads these instead -- half the operand bytes, no conversion at staging. */
                       /* Needs both, Nout / Cin / ldy / ldx multiples of 8, 16-byte aligned bases, no dbias; otherwise dY / X are read. */
                       /* dY and / or X may be NULL when the tensor exists as its twin only (an inner gradient written with cdetr_gemm_desc.C  */
                       /* == NULL; an activation kept as interleaved groups + twin): the twin-fed tile kernel must then be the one that runs   */
                       /* (more than 1024 pixels, the conditions above), CDETR_ERR_ARG otherwise -- never a silent read of a missing tensor.   */
                       /* CDETR_WGRAD_KP (environment, under CDETR_TUNING): 32-pixel blocks staged per barrier by the twin-fed kernels, 1 (default) / 2 / 4. */
} cdetr_wgrad_desc;
int cdetr_wgrad(const cdetr_wgrad_desc* d, void* stream);
/* n INDEPENDENT weight-gradient problems submitted together (same semantics as n cdetr_wgrad calls in any order; problems may
 * accumulate into the same dW / dbias).  Problems of the few-pixel and of the 64x64 transpose-read kernel class run as grouped
 * launches (one kernel for up to 16 problems), the rest one by one.  Replaces: the per-parameter autograd weight-gradient nodes of
 * one layer's backward (torch.autograd of F.linear at A2/models/transformer.py:242-279, 337-409), whose results only the
 * optimizer reads.                                                                                                       */
int cdetr_wgrad_group(const cdetr_wgrad_desc* descs, int32_t n, void* stream);

/* out[n] += sum_m X[m][n]   (bias gradients; atomics) */
int cdetr_colsum(const float* X, int64_t ldx, int32_t M, int32_t N, float* out, void* stream);

/* ---- fused optimizer tail over the flat arenas (A2/engine.py:54-57 clip_grad_norm_(0.1) + torch.optim.AdamW) ------
 * cdetr_sumsq:      out[0] = sum_i g[i]^2, bit-reproducible (fixed summation order: data-parallel ranks holding the same
 *                   reduced gradient must compute the same clip coefficient, or their parameters drift apart).
 *                   workspace: CDETR_SUMSQ_WS_FLOATS device floats of scratch (per-block partial sums; a second one-block
 *                   launch adds them in index order).
 * cdetr_adamw_step: g' = g * grad_div; coef = min(max_norm / (||g'|| + 1e-6), 1) (max_norm <= 0: no clip);
 *                   p *= 1 - lr*wd; m = b1 m + (1-b1) g'coef; v = b2 v + (1-b2)(g'coef)^2;
 *                   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps),  lr = lr[i] * state[1], t = state[0] + 1.
 *                   state (device float[4]): [0] step count (incremented), [1] lr scale (StepLR), [2] <- ||g'|| (logging),
 *                   [3] += 1 when ||g'|| is NaN / Inf: that step changes neither p, m, v nor the step count (the reference
 *                   aborts on a non-finite loss BEFORE its optimizer step, A2/engine.py:44-49).                               */
#define CDETR_SUMSQ_MAX_BLOCKS 2048
#define CDETR_SUMSQ_WS_FLOATS CDETR_SUMSQ_MAX_BLOCKS
int cdetr_sumsq(const float* g, int64_t n, float* out, float* workspace, void* stream);
int cdetr_adamw_step(float* p, const float* g, float* m, float* v, const float* lr, int64_t n, const float* sumsq,
                     float* state, float max_norm, float beta1, float beta2, float eps, float weight_decay, float grad_div,
                     void* stream);
/* cdetr_adamw_step2: the same with the learning rates given as TWO values split at element lr_split when lr == NULL (elements
 * [0, lr_split) use lr0, the rest lr1; lr_split a multiple of 4): the reference's parameter groups (A2/main.py:157-183) are two
 * contiguous ranges of the arena, and the per-element table is a 150 MB stream the update does not need.                       */
int cdetr_adamw_step2(float* p, const float* g, float* m, float* v, const float* lr, float lr0, float lr1, int64_t lr_split, int64_t n,
                      const float* sumsq, float* state, float max_norm, float beta1, float beta2, float eps, float weight_decay,
                      float grad_div, void* stream);
/* cdetr_sgd_step: torch.optim.SGD(momentum, dampening 0, no Nesterov, coupled L2 weight decay) after the same clip, in one pass over
 *                 p, g and the momentum buffer buf (A2/main.py:185-186, --sgd):
 *                 g' = g * grad_div; coef = min(max_norm / (||g'|| + 1e-6), 1) (max_norm <= 0: no clip);
 *                 d = g' coef + weight_decay p; buf = momentum buf + d; p -= lr buf,  lr = (lr ? lr[i] : i < lr_split ? lr0 : lr1) * state[1].
 *                 A zero buf before the first step gives buf = d (torch's clone rule).  lr / lr_split and state[4] as in
 *                 cdetr_adamw_step2: [0] step count, [1] lr scale, [2] <- ||g'||, [3] += 1 when ||g'|| is NaN / Inf (p and buf
 *                 unchanged, step count too).                                                                                    */
int cdetr_sgd_step(float* p, const float* g, float* buf, const float* lr, float lr0, float lr1, int64_t lr_split, int64_t n,
                   const float* sumsq, float* state, float max_norm, float momentum, float weight_decay, float grad_div, void* stream);
/* dz[i] = y[i] > 0 ? dy[i] * scale : 0      (ReLU backward of the fused linear+ReLU layers) */
int cdetr_relu_mask(const float* y, const float* dy, float* dz, int64_t n, float scale, void* stream);
/* the same, also writing a bf16 twin of dz (dz16 may be NULL) */
int cdetr_relu_mask2(const float* y, const float* dy, float* dz, void* dz16, int64_t n, float scale, void* stream);

/* ---- transformer-layer glue (HBM-bound, fused so a layer touches its activations as few times as possible) --------
 * cdetr_layernorm_fwd/bwd: nn.LayerNorm over the last dim C (multiple of 256, <= 1024); fwd saves mean/rstd per row;
 *   bwd: dx (+ add), dgamma += ..., dbeta += ... (A2/models/transformer.py:233,274,334-339,420,425).
 * cdetr_posadd2:   Qr = X + Prow (broadcast over h), Qc = X + Pcol (broadcast over w)   (transformer.py:248-255).
 * cdetr_hw_reduce: Or[n,x,:] = sr * sum_y Xr[n,y,x,:] (+ Ar), Oc[n,y,:] = sc * sum_x Xc[n,y,x,:] (+ Ac)
 *                  (forward: the mean-before-project key inputs; backward: sums of gradient maps over the broadcast axis).
 * cdetr_bcast_add2: out = T + sr * Br[n,x,:] + sc * Bc[n,y,:]                                                   */
/* nn.GroupNorm(G, C) on the NHWC activation x [B][P][C] (P = h*w; C / G a multiple of 4, <= 64): fwd saves mean / rstd [B*G];
 * bwd writes dx and ACCUMULATES dgamma / dbeta [C].  Replaces: GroupNorm(32, 256) of the input projection,
 * A2/models/anchor_detr.py:86-92 (evaluated there on an NCHW tensor).                                                       */
int cdetr_groupnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                        int32_t B, int32_t P, int32_t C, int32_t G, float eps, void* stream);
int cdetr_groupnorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx,
                        float* dgamma, float* dbeta, int32_t B, int32_t P, int32_t C, int32_t G, void* stream);
/* The same two calls with the pixels of an image spread over workgroups (C == 256: coalesced 1 KB rows, B * P / 32 workgroups instead of B * G) and the
 * group statistics crossing them through `ws` (>= B * ceil(P / 32) * G * 12 bytes forward, * 8 backward; contents undefined before and after): two
 * launches each -- per-chunk partials (forward: count / mean / centred second moment, merged with Chan's update in chunk order), then merge + apply.
 * Shapes the split form does not cover (C != 256, fewer than 128 pixels, ws too small / NULL) run cdetr_groupnorm_fwd / _bwd.                       */
int cdetr_groupnorm_fwd_ws(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                           int32_t B, int32_t P, int32_t C, int32_t G, float eps, void* ws, int64_t ws_bytes, void* stream);
int cdetr_groupnorm_bwd_ws(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx,
                           float* dgamma, float* dbeta, int32_t B, int32_t P, int32_t C, int32_t G, void* ws, int64_t ws_bytes, void* stream);

int cdetr_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                        int32_t rows, int32_t C, float eps, void* stream);
/* the same forward, plus o1 = y + a1 and (optional pair) o2 = y + a2 in the same pass: the positional adds that consume a decoder
 * LayerNorm's output (tgt + query_pos_x / tgt + query_pos_y, A2/models/transformer.py:385-389; next layer's tgt + query_pos, :369) */
int cdetr_layernorm_fwd_add(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            const float* a1, const float* a2, float* o1, float* o2, int32_t rows, int32_t C, float eps, void* stream);
int cdetr_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        const float* add, float* dx, float* dgamma, float* dbeta, int32_t rows, int32_t C, void* dx16, void* stream);
/* (dx16: optional bf16 twin of dx, C = 256 -- the A16 operand of the plain-bf16 data-gradient GEMM that consumes dx)
 * the same with the incoming gradient given as a sum, dy + g1 + g2 (g2 optional), and the side effects acc1 += g1, acc2 += g2 (optional, in
 * place): cdetr_grad_merge folded into the LayerNorm backward that consumes its result (decoder backward: the gradient of a sub-layer input is
 * the residual branch plus one or two projection branches whose values also accumulate into the stack-wide query-position gradients).  Br / Bc
 * (optional pair, rows = N*H*W): two more addends broadcast over the map, + sr * Br[n,x,:] + sc * Bc[n,y,:] -- cdetr_bcast_add2_sum folded in the
 * same way (encoder backward: the gradient of a layer's input feeds the LayerNorm backward of the layer below).  C = 256.                       */
int cdetr_layernorm_bwd_merge(const float* dy, const float* g1, const float* g2, float* acc1, float* acc2, const float* Br, const float* Bc,
                              float sr, float sc, int32_t H, int32_t W, const float* x, const float* mean, const float* rstd,
                              const float* gamma, const float* add, float* dx, float* dgamma, float* dbeta, int32_t rows, int32_t C,
                              void* dx16, void* stream);
int cdetr_posadd2(const float* X, const float* Prow, const float* Pcol, float* Qr, float* Qc, int32_t N, int32_t H, int32_t W,
                  int32_t C, void* stream);
int cdetr_hw_reduce(const float* Xr, const float* Xc, const float* Ar, const float* Ac, float* Or, float* Oc, int32_t N,
                    int32_t H, int32_t W, int32_t C, float scale_r, float scale_c, void* stream);
/* cdetr_posadd2 and cdetr_hw_reduce(X, X, Prow, Pcol, ...) of one encoder layer as ONE launch (both read the same source and nothing of each
 * other: A2/models/transformer.py:246-252): Qr / Qc = X + Prow / Pcol (broadcast), Kr / Kc = mean over H / W of X, scaled, + Prow / Pcol. */
int cdetr_posadd2_hw_reduce(const float* X, const float* Prow, const float* Pcol, float* Qr, float* Qc, float* Kr, float* Kc, int32_t N,
                            int32_t H, int32_t W, int32_t C, float scale_r, float scale_c, void* stream);
int cdetr_bcast_add2(const float* T, const float* Br, const float* Bc, float* out, int32_t N, int32_t H, int32_t W, int32_t C,
                     float sr, float sc, void* stream);
/* the same with up to two further addends of T's shape (T2, T3; NULL = absent): out = T + T2 + T3 + sr*Br + sc*Bc -- sibling data gradients
 * of one input (the three projections of A2/models/row_column_decoupled_attention.py:165-208 that read src) run as ONE grouped launch into
 * separate buffers and are summed here instead of being chained through residual epilogues.                                           */
int cdetr_bcast_add2_sum(const float* T, const float* T2, const float* T3, const float* Br, const float* Bc, float* out, int32_t N, int32_t H,
                         int32_t W, int32_t C, float sr, float sc, void* stream);
/* decoder-layer glue (A2/models/transformer.py:366-403): cdetr_add2: O1 = T + A, O2 = T + B (B and O2 NULL together);
 * cdetr_grad_merge (backward of those sites): out = base + g1 (+ g2), acc1 += g1, acc2 += g2 (g2 / acc1 / acc2 may be NULL);
 * n = element count, a multiple of 4, all pointers 16-byte aligned.                                                    */
int cdetr_add2(const float* T, const float* A, const float* B, float* O1, float* O2, int64_t n, void* stream);
/* sine positional embedding (A2/models/transformer.py:474-494): out[r][i] = i even ? sin(x) : cos(x),
 * x = pos[r * pstride] * 2 pi / temperature^(2 floor(i/2) / nfeat), rows of `out` / `dout` ldo floats apart;
 * backward: dpos[r * dstride] (+)= sum_i dout[r][i] * d out[r][i] / d pos (accumulate != 0 adds).                       */
int cdetr_sine_embed(const float* pos, int32_t pstride, float* out, int64_t ldo, int32_t rows, int32_t nfeat, float temperature,
                     void* stream);
int cdetr_sine_embed_bwd(const float* pos, int32_t pstride, const float* dout, int64_t ldo, float* dpos, int32_t dstride, int32_t rows,
                         int32_t nfeat, float temperature, int32_t accumulate, void* stream);
int cdetr_grad_merge(const float* base, const float* g1, const float* g2, float* acc1, float* acc2, float* out, int64_t n,
                     void* stream);

/* ---- k-contiguous mirrors of the weights used as data-gradient operands ------------------------------------------------
 * The data-gradient GEMMs of A2/models/resnet.py:140-160 (conv backward) and of every F.linear site contract over the
 * OUTPUT channels of a weight W[o][tap][c]; the matrix pipe wants that axis contiguous.  One launch rewrites every
 * registered weight as Wt[c][tap][o] = W[o][tap][c] * scale[o] (scale = folded FrozenBN, may be NULL) and / or as the
 * pre-split bf16 operand of the bf16x3 GEMM kernels; items live in device memory, `tile0` = prefix sum of
 * ceil(R/32)*ceil(C/32)*taps.                                                                                          */
typedef struct {
    const float* src;     /* W  [R][taps][C]                                                                    */
    float* dst;           /* transpose = 1: Wt [C][taps][R] fp32 (may be NULL)                                  */
    void* dst_split;      /* pre-split bf16 image (may be NULL): transpose = 1: of Wt (needs R % 32 == 0),      */
                          /* transpose = 0: of W itself (needs C % 32 == 0); layout as cdetr_gemm_desc.B_split  */
    const float* scale;   /* [R] or NULL                                                                        */
    int32_t R, C, taps, tile0, transpose, pad_;
    void* dst_hi;         /* optional, transpose = 1: bf16(Wt) [C][taps][R], the plain-bf16 data-gradient operand        */
                          /* (cdetr_gemm_desc.B16: full cache lines of hi values, no interleaved lo halves)             */
} cdetr_mirror_item;
int cdetr_weight_mirror(const cdetr_mirror_item* items_dev, int32_t n_items, int32_t total_tiles, void* stream);
/* the forward images only (every item transpose = 0, 16-byte aligned src / dst_split, C % 32 == 0): a streaming pass, 4 weights per thread;
 * item.tile0 = first block of the item in units of 4096 weights (ceil(R * taps * C / 4096) blocks per item), total_blocks their sum.           */
int cdetr_weight_images(const cdetr_mirror_item* items_dev, int32_t n_items, int32_t total_blocks, void* stream);

/* 3x3 stride-2 pad-1 max pooling, NHWC (A2/models/resnet.py:206,265) */
int cdetr_maxpool3x3s2(const float* X, float* Y, int32_t Nimg, int32_t H, int32_t W, int32_t C, void* stream);
/* the same, also writing the split-bf16 planes of Y (Y16 = bf16(Y), Y16lo = bf16(Y - float(Y16)); either may be NULL) */
int cdetr_maxpool3x3s2_split(const float* X, float* Y, void* Y16, void* Y16lo, int32_t Nimg, int32_t H, int32_t W, int32_t C, void* stream);

/* ---- Row-Column Decoupled Attention core (A2/models/row_column_decoupled_attention.py:215-309) -------------
 * Inputs are the PROJECTED tensors: q_row,q_col [N][L][E]; k_row [N][W][E] (already averaged over H);
 * k_col [N][H][E] (averaged over W); v [N][H][W][E]; E = nh*32.  mask_row [N][W], mask_col [N][H] uint8 (1 = pad)
 * or NULL.  Computes, per (n, head):  A_row = softmax_W(scale*q_row.k_row^T), A_col = softmax_H(scale*q_col.k_col^T),
 * out[n][q][head*32+c] = sum_h sum_w A_col[q][h] A_row[q][w] v[n][h][w][head*32+c].
 * a_row [N][nh][L][Wp], a_col [N][nh][L][Hp] (Wp = W rounded up to 4, Hp = H rounded up to 8; pad = 0) are written
 * for the backward pass; both NULL = inference: nothing is saved (2 x 8 MB of stores per encoder call at 800 x 800).  Feature maps up to
 * 128 x 1024 keys; the MFMA two-step kernels cover W <= 96 (an 800 x 1333 FSCD-LVIS image at stride 16), wider maps the generic kernel.  */
typedef struct {
    int32_t N, L, H, W, nh; /* head dim fixed at 32 */
    int32_t precision;      /* 0 = fp32 MFMA, 1 = split-bf16 x3 (as in cdetr_gemm_desc) */
    float scale;
    const float* q_row; const float* q_col; const float* k_row; const float* k_col; const float* v;
    const uint8_t* mask_row; const uint8_t* mask_col;
    float* out; float* a_row; float* a_col;
    void* ws;               /* optional scratch (zero-initialised once, >= 16 KB + partial outputs; the kernels leave its counters zero): lets the */
    int64_t ws_bytes;       /* two-step forward cut the key rows into slices when (N * nh * L / 128) workgroups would not fill the chip; the     */
                            /* split-reduction scratch of cdetr_gemm_desc.splitk_ws may be passed (launches of one stream do not overlap)      */
} cdetr_rcda_fwd_desc;
int cdetr_rcda_fwd(const cdetr_rcda_fwd_desc* d, void* stream);

/* Backward of the core: given d_out [N][L][E] and the saved a_row/a_col, writes
 * ds_row [N][nh][L][Wp], ds_col [N][nh][L][Hp] (gradients of the PRE-softmax logits, already multiplied by
 * `scale`) and accumulates d_v [N][H][W][E] (must be zeroed by the caller).
 * Optional (NULL = skip): with k_row [N][W][E], k_col [N][H][E] and dq_row / dq_col [N][L][E] given, the same launch also
 * writes the query gradients dq_row[q] = sum_w ds_row[q][w] k_row[w], dq_col[q] = sum_h ds_col[q][h] k_col[h] (per head) --
 * the logits -> projected-query step of the reference's autograd (A2/models/row_column_decoupled_attention.py:230-262).   */
typedef struct {
    int32_t N, L, H, W, nh;
    int32_t precision;
    float scale;
    const float* d_out; const float* a_row; const float* a_col; const float* v;
    float* ds_row; float* ds_col; float* d_v;
    const float* k_row; const float* k_col;
    float* dq_row; float* dq_col;
    const float* q_row; const float* q_col;   /* optional, with dq_*: also ACCUMULATE the key gradients; ds_row / ds_col may then  */
                                              /* both be NULL (the logit gradients never leave the chip)                        */
    float* dk_row; float* dk_col;             /* dk_row[n][w] += sum_q ds_row[q][w] q_row[q] (per head; caller zeroes them)    */
} cdetr_rcda_bwd_desc;
int cdetr_rcda_bwd(const cdetr_rcda_bwd_desc* d, void* stream);
static inline int32_t cdetr_rcda_wp(int32_t W) { return (W + 3) & ~3; }
static inline int32_t cdetr_rcda_hp(int32_t H) { return (H + 7) & ~7; }

/* ---- decoder self-attention core (nn.MultiheadAttention(256, 8) at A2/models/transformer.py:337,369-370) ---------
 * qk [N][L][2E] = projected queries | keys, v [N][L][E], E = nh*32; o = softmax(scale * q k^T) v per head, lse [N][nh][L]
 * saved for backward.  cdetr_mha_bwd writes d_qk [N][L][2E], d_v [N][L][E]; work: N*nh*L floats of scratch (the row sums D of the
 * fp32 mode's two launches; the split-bf16 mode is ONE launch whose key half forms D itself and leaves `work` untouched).
 * cdetr_mha_bwd precision: 0 = fp32, 1 = split-bf16 x3 throughout, 3 = the scores recomputed in split-bf16 x3 (p = exp(s - lse) against the
 * forward's lse) and the four gradient contractions (dP, dQ, dK, dV) in plain bf16, one MFMA per product.                           */
int cdetr_mha_fwd(const float* qk, const float* v, float* o, float* lse, int32_t N, int32_t L, int32_t nh, float scale,
                  int32_t precision, void* stream);
int cdetr_mha_bwd(const float* qk, const float* v, const float* o, const float* d_o, const float* lse, float* d_qk, float* d_v,
                  float* work, int32_t N, int32_t L, int32_t nh, float scale, int32_t precision, void* stream);

/* The ragged form (stage-1 batches whose images carry different numbers of queries).  Layout and arithmetic are cdetr_mha_fwd / _bwd's; image
 * n still starts at row n*L, and lens [N] (int32, DEVICE memory, read by the kernels -- a captured graph follows new lengths) gives the masking
 * bound len = clamp(lens[n], 0, L) on the query AND the key side: rows >= len are no one's keys, their qk / v / d_o values are never read into a
 * valid row (select, not multiplication: NaN there is harmless).  Written for rows >= len: o, lse, d_qk, d_v = exact 0.  lens[n] == 0 gives an
 * all-zero image.  With every lens[n] == L the results are cdetr_mha_fwd / _bwd's bit for bit.  Pointers 16-byte aligned.                    */
int cdetr_mha_fwd_lens(const float* qk, const float* v, const int32_t* lens, float* o, float* lse, int32_t N, int32_t L, int32_t nh,
                       float scale, int32_t precision, void* stream);
int cdetr_mha_bwd_lens(const float* qk, const float* v, const int32_t* lens, const float* o, const float* d_o, const float* lse, float* d_qk,
                       float* d_v, float* work, int32_t N, int32_t L, int32_t nh, float scale, int32_t precision, void* stream);

/* ---- general attention core (nn.MultiheadAttention(256, 8) without masks: the encoder self-attention over all h*w tokens and the
 * decoder cross-attention from Q queries to h*w keys of attention_type "nn.MultiheadAttention", A2/models/transformer.py:262-272,393-398)
 * o = softmax(scale * q k^T) v per head, head dim 32, E = nh*32.  q: N images of Lq rows, row stride ldq (image n starts at row n*Lq);
 * k, v: N images of Lk rows, row strides ldk, ldv; head h reads columns 32h .. 32h+31 of a row.  The strides let q and k be the two halves of
 * one packed [N][L][2E] projection (k = q + E, ldq = ldk = 2E; cdetr_mha_* is exactly that instance) or separate tensors.  Strides are
 * multiples of 4 floats, pointers 16-byte aligned.  o [N][Lq][E] and lse [N][nh][Lq] (the row log-sum-exp, saved for the backward) are
 * dense.  Any Lq, Lk >= 1: rows past either length are masked arithmetically.
 * cdetr_attn_fwd: reads q, k, v; writes o, lse.  precision 0 = fp32 (VALU), 1 or 3 = split-bf16 x3 MFMA.
 * cdetr_attn_bwd: reads q, k, v, o, lse and d_o [N][Lq][E]; writes d_q, d_k, d_v (rows like q, k, v, with their own strides ld_dq,
 * ld_dk, ld_dv: d_q and d_k may be the halves of one packed [N][L][2E] buffer).  precision 0 = fp32 in two launches (work: N*nh*Lq
 * floats of scratch), 1 = split-bf16 x3 throughout, 3 = scores recomputed in split-bf16 x3 and the four gradient contractions in
 * plain bf16 (as cdetr_mha_bwd); 1 and 3 are ONE launch whose query-side workgroups write d_q and whose key-side workgroups write
 * d_k, d_v, and leave `work` untouched.                                                                                                 */
typedef struct {
    const float* q; const float* k; const float* v;
    int64_t ldq, ldk, ldv;
    float* o; float* lse;
    const float* d_o;                   /* backward only */
    float* d_q; float* d_k; float* d_v;
    int64_t ld_dq, ld_dk, ld_dv;
    float* work;                        /* backward, precision 0 only */
    int32_t N, Lq, Lk, nh;
    float scale;
    int32_t precision;
} cdetr_attn_desc;
int cdetr_attn_fwd(const cdetr_attn_desc* d, void* stream);
int cdetr_attn_bwd(const cdetr_attn_desc* d, void* stream);

/* ---- Hungarian matcher (A2/models/matcher.py:197-247 + scipy.optimize.linear_sum_assignment) -------------
 * cdetr_match_cost: per image b, cost[b] = 5*L1 + 2*focal-class + 2*(-GIoU) in fp32 with the reference's expression
 * order, written in SOLVER layout: [nr][nc] with nr = min(Q,T_b), nc = max(Q,T_b) (transposed when T_b < Q,
 * exactly like scipy transposes a tall matrix).  cost_off[b] = float offset of image b's block.
 * logits [B][Q][ncls] (column 0 used: all labels are 0), boxes [B][Q][4] cxcywh, tgt [sum T][4], tgt_off[B+1].    */
int cdetr_match_cost(const float* logits, int32_t ncls, const float* boxes, const float* tgt, const int32_t* tgt_off,
                     const int64_t* cost_off, int32_t B, int32_t Q, float w_class, float w_bbox, float w_giou,
                     float* cost, void* stream);
/* cdetr_lsap: exact rectangular assignment on the device (float64 duals, shortest augmenting paths, the tie rule of
 * scipy's solver) -- one workgroup per image.  Writes idx_i/idx_j (int64, [B][Mmax]) = (query, target) pairs with
 * idx_i ascending -- the (row_ind, col_ind) scipy returns; status[b] = 0 ok / 1 infeasible / 2 invalid cost.
 * nc_max = max(Q, max_b T_b) (host-known; sizes the LDS-resident solver state, limit 3800);
 * Mmax = row stride of idx_i / idx_j (>= max_b min(Q, T_b)).                                                    */
int cdetr_lsap(const float* cost, const int64_t* cost_off, const int32_t* tgt_off, int32_t B, int32_t Q,
               int32_t nc_max, int32_t Mmax, int64_t* idx_i, int64_t* idx_j, int32_t* status, void* stream);

/* ---- SetCriterion (A2/models/anchor_detr.py:143-367, losses [labels, boxes, cardinality, vars], no aux) ----------------
 * cdetr_criterion_fwd: from the raw predictions, the concatenated targets and the matcher's device indices
 * (idx_i / idx_j [B][Mmax], first min(Q, T_b) entries of row b valid) compute
 *   losses[6] = { loss_ce, class_error, cardinality_error, loss_bbox, loss_giou, loss_variance }
 * and the gradient of every differentiable loss w.r.t. its inputs:
 *   g_logits [B,Q,C] = d loss_ce / d logits;  g_l1 / g_giou / g_var_box [B,Q,4] = d {loss_bbox, loss_giou, loss_variance} / d boxes;
 *   g_vars [B,Q,2] = d loss_variance / d vars.   num_boxes is a DEVICE scalar (the data-parallel normaliser).
 * cdetr_criterion_bwd: d_logits = g[0] g_logits; d_boxes = g[3] g_l1 + g[4] g_giou + g[5] g_var_box; d_vars = g[5] g_vars
 * (g = upstream gradient of the six scalars, device; see the prototype for how it is formed).                              */
typedef struct {
    int32_t B, Q, C, num_classes, Mmax;
    float alpha;
    const float* logits;        /* [B,Q,C] */
    const float* boxes;         /* [B,Q,4] cxcywh */
    const float* vars;          /* [B,Q,2] */
    const float* tgt_boxes;     /* [sum T,4] */
    const int64_t* tgt_labels;  /* [sum T] */
    const int32_t* tgt_off;     /* [B+1] */
    const int64_t* idx_i;       /* [B,Mmax] */
    const int64_t* idx_j;       /* [B,Mmax] */
    const float* num_boxes;     /* device scalar */
    float* losses;              /* [6] */
    float* g_logits;
    float* g_l1;
    float* g_giou;
    float* g_var_box;
    float* g_vars;
    const float* loss_weights;  /* optional [6] (NULL = absent): losses[6] <- sum_k loss_weights[k] * losses[k], the weighted total of
                                   A2/engine.py:37 (losses then has 7 elements) */
} cdetr_criterion_desc;
int cdetr_criterion_fwd(const cdetr_criterion_desc* d, void* stream);
/* g6 (upstream gradient of the six scalars) and g_total (upstream gradient of the weighted total, with loss_weights) may each be
 * NULL = zero: the effective gradient of loss k is g6[k] + g_total[0] * loss_weights[k]. */
int cdetr_criterion_bwd(const float* g6, const float* g_total, const float* loss_weights, const float* g_logits, const float* g_l1,
                        const float* g_giou, const float* g_var_box, const float* g_vars, float* d_logits, float* d_boxes, float* d_vars,
                        int32_t BQ, int32_t C, void* stream);

/* cdetr_criterion_eval (csrc/criterion_eval.hip): the evaluation form -- forward only, one workgroup per image (grid = B, no limit of 64 and
 * none on B*Q; LDS holds one image's Q target classes).  Row b of losses [B][7] is what SetCriterion returns for image b evaluated ALONE, as
 * the reference's inference driver does (A2/infer.py:27-122): the normaliser is max(T_b, 1), formed in the kernel from tgt_off (no num_boxes,
 * no all-reduce); cardinality_error = |#object queries of image b - T_b|; the means of loss_variance run over image b's own min(Q, T_b)
 * pairs; without pairs class_error = 100 and loss_bbox = loss_giou = loss_variance = 0; a negative variance gives NaN in its own row only.
 * Same order of the six scalars and same expressions as cdetr_criterion_fwd; losses[b][6] = sum_k loss_weights[k] * losses[b][k] (0 when
 * loss_weights is NULL).  Inputs as in cdetr_criterion_desc; the counts are read from device memory, so a capacity plan and a captured
 * graph serve any target counts.  Ordered reductions (wave tree, then a serial sum over the waves): bit-reproducible, and row b does not
 * depend on the other images of the batch.                                                                                            */
typedef struct {
    int32_t B, Q, C, num_classes, Mmax;
    float alpha;
    const float* logits;        /* [B,Q,C] */
    const float* boxes;         /* [B,Q,4] cxcywh */
    const float* vars;          /* [B,Q,2] */
    const float* tgt_boxes;     /* [sum T,4] */
    const int64_t* tgt_labels;  /* [sum T] */
    const int32_t* tgt_off;     /* [B+1] */
    const int64_t* idx_i;       /* [B,Mmax] */
    const int64_t* idx_j;       /* [B,Mmax] */
    float* losses;              /* [B,7] */
    const float* loss_weights;  /* optional [6] (NULL = absent) */
} cdetr_criterion_eval_desc;
int cdetr_criterion_eval(const cdetr_criterion_eval_desc* d, void* stream);

/* ---- 1st-stage BoundingBoxCriterion (A1/models/anchor_detr.py:317-337; no matcher: query n of image b <-> exemplar n) --------------
 * cdetr_bbox_criterion_fwd: M = B*N pairs, src = [tgt_points, pred_wh], tgt = [tgt_points, tgt_whs] (cxcywh):
 *   losses[3] = { loss_wh = mean |pred_wh - tgt_whs| (2M elements), loss_giou = sum (1 - GIoU(src, tgt)) / M,
 *                 total = w_wh * loss_wh + w_giou * loss_giou }
 * and the per-element gradients g_wh / g_giou [M,2] = d {loss_wh, loss_giou} / d pred_wh (torch's subgradients: sign(0) = 0, equal
 * operands of max / min split the gradient evenly, clamp(min=0) passes it at 0).  pred_wh is read IN PLACE: row r's (w, h) are
 * pred_wh[r * pred_stride + {0, 1}] (the [..., 2:] columns of the box head's [B,Q,4] output: pointer + 2 floats, stride 4).
 * tgt_points / tgt_whs are contiguous [M,2].  One workgroup, ordered reductions: bit-reproducible for any M >= 1.
 * cdetr_bbox_criterion_bwd: d_coord [M,4] (16-byte aligned) = (0, 0, e_wh g_wh + e_giou g_giou) with e_k = g3[k] + g3[2] w_k
 * (g3 = upstream gradient of the three scalars, device).                                                                   */
int cdetr_bbox_criterion_fwd(const float* pred_wh, int64_t pred_stride, const float* tgt_points, const float* tgt_whs, int32_t M,
                             float w_wh, float w_giou, float* losses, float* g_wh, float* g_giou, void* stream);
int cdetr_bbox_criterion_bwd(const float* g3, float w_wh, float w_giou, const float* g_wh, const float* g_giou, float* d_coord,
                             int32_t M, void* stream);

/* The ragged form: B images of N rows, lens [B] (int32, DEVICE memory); row n of image b is a pair iff n < clamp(lens[b], 0, N).  The sums run
 * over the valid pairs and the normaliser M = sum(lens) is formed in the kernel.  Padded rows of pred_wh / tgt_* are never read; their g_wh /
 * g_giou / d_coord rows are exact zeros.  M == 0 gives losses and gradients of 0.  One workgroup, ordered reductions; with every lens[b] == N
 * the losses and gradients are cdetr_bbox_criterion_fwd / _bwd's (M = B*N) bit for bit.                                                      */
int cdetr_bbox_criterion_lens_fwd(const float* pred_wh, int64_t pred_stride, const float* tgt_points, const float* tgt_whs,
                                  const int32_t* lens, int32_t B, int32_t N, float w_wh, float w_giou, float* losses, float* g_wh,
                                  float* g_giou, void* stream);
int cdetr_bbox_criterion_lens_bwd(const float* g3, float w_wh, float w_giou, const float* g_wh, const float* g_giou, const int32_t* lens,
                                  float* d_coord, int32_t B, int32_t N, void* stream);

/* ---- box-AP evaluation (csrc/coco_eval.hip): pycocotools' COCOeval, bbox path, as restated in counting_detr_amd/coco_ap.py -- what the
 * reference's offline evaluator runs on the host (A2/eval_all.py:285-312, 496-531).  All values FLOAT64, finite; contraction into FMAs is
 * switched off in this translation unit, so every IoU equals numpy's bit for bit and `iou >= threshold` / equal-IoU ties resolve as on the host.
 * cdetr_box_iou_xywh: iou [D][G] of dt [D][4] against gt [G][4] (xywh): inter = max(min(x+w) - max(x), 0) * max(min(y+h) - max(y), 0),
 *   union = (dw*dh + gw*gh) - inter, iou = union > 0 ? inter / union : 0 (maskApi bbIou, no crowd).  D == 0 or G == 0: nothing is launched.
 * cdetr_coco_match: COCOeval.evaluateImg for B images x A area ranges x T IoU thresholds in ONE launch (one workgroup per image and range, one
 *   wave per threshold; the image's ground-truth boxes are staged in LDS).  Images are packed: image b owns ground truths gt_off[b] .. gt_off[b+1]
 *   and detections dt_off[b] .. dt_off[b+1]; the detections are ALREADY in evaluation order (descending score, stable, cut at maxDets).
 *   Per (image, range [lo, hi], threshold t), detections in order: a ground truth is ignored when gt_ignore is set or its area is < lo or > hi;
 *   the detection takes the unmatched non-ignored ground truth of highest IoU >= t (the highest index among equal IoUs); only if there is none,
 *   by the same rule an unmatched ignored one, and is then ignored itself; a matched ground truth is taken for good (no crowd re-matching); an
 *   unmatched detection whose area is < lo or > hi is ignored.  npig = the number of non-ignored ground truths.  iou_thrs / area_rng are used as
 *   given (the caller applies min(t, 1 - 1e-10)).  Gmax = the largest ground-truth count of one image (host-known: it sizes the LDS image;
 *   limit 4096, CDETR_ERR_UNSUPPORTED beyond; an image whose count exceeds Gmax is left untouched); any number of detections; T <= 16.
 *   Gtot == 0 / Dtot == 0: the ground-truth / detection and output pointers may be NULL.                                                  */
typedef struct {
    int32_t B, A, T, Gtot, Dtot, Gmax;
    const double* gt_boxes;     /* [Gtot][4] xywh */
    const double* gt_area;      /* [Gtot] */
    const uint8_t* gt_ignore;   /* [Gtot] ignore or iscrowd */
    const int32_t* gt_off;      /* [B+1] */
    const double* dt_boxes;     /* [Dtot][4] xywh */
    const double* dt_area;      /* [Dtot] */
    const int32_t* dt_off;      /* [B+1] */
    const double* iou_thrs;     /* [T] */
    const double* area_rng;     /* [A][2] */
    uint8_t* matched;           /* [A][T][Dtot] */
    uint8_t* det_ignored;       /* [A][T][Dtot] */
    int32_t* npig;              /* [A][B] */
} cdetr_coco_match_desc;
int cdetr_box_iou_xywh(const double* dt, int32_t D, const double* gt, int32_t G, double* iou, void* stream);
int cdetr_coco_match(const cdetr_coco_match_desc* d, void* stream);

/* ---- per-image evaluation statistics (csrc/coco_report.hip; infer.py --image_report): what the reference's evaluator keeps per image
 * (A2/eval_all.py:181, 227-239: count and an `ap` field per image) and the counts behind COCOeval's recall numbers at maxDets 900 / 1000 /
 * 1100, from the flags cdetr_coco_match left in device memory.  FLOAT64 and integers only, contraction into FMAs switched off: every output
 * EQUALS coco_ap.stats_from_flags (numpy) bit for bit.
 * cdetr_coco_image_stats: ONE launch, one workgroup per (image, area range), one wave per IoU threshold.  For (a, b, t) let n be the used
 *   length of image b's segment dt_off[b] .. dt_off[b+1] (the whole segment, or min(dt_cnt[b], segment) with dt_cnt), and over its detections
 *   i in order ctp_i / cfp_i the running counts of `matched & !ignored` / `!matched & !ignored`:
 *     tp / fp [a][b][t][m] = ctp / cfp at index min(cuts[m], n) - 1, 0 when that length is 0.  COCOeval matches once over dt[:maxDets[-1]] and
 *                            slices afterwards, and a greedy match never looks ahead: these ARE the counts of an evaluation at maxDet = cuts[m].
 *     ap [a][b][t]         = -1.0 when npig[a][b] == 0; else with rc_i = ctp_i / npig, pr_i = ctp_i / ((cfp_i + ctp_i) + 2^-52) made
 *                            non-increasing from the right and q[r] = pr[first i with rc_i >= rec_thrs[r]] (0 if there is none):
 *                            (((q[0] + q[1]) + q[2]) + ...) / R, summed in index order by one lane.  n == 0 with npig > 0 gives 0.
 *   Running counts are ballots and popcounts over chunks of 64 detections, the envelope a suffix maximum, a sample's index a search in the
 *   one chunk whose recalls straddle it; no atomics, no floating-point value crosses lanes except through max.
 *   Limits: T <= 16, M <= 64, R <= 256, A <= 65535, CDETR_ERR_UNSUPPORTED beyond, before any launch.  Detections per image: NO limit -- an
 *   image is streamed in chunks of 64 and nothing per detection is held on chip (1100 at T = 10, the evaluator's maxDets, is 18 chunks).
 *   rec_thrs need not be sorted; a cut <= 0 keeps nothing.  A segment that does not lie inside 0 .. Dtot counts as empty and is not read.
 *   B == 0: nothing is launched.  Dtot == 0: the flag pointers may be NULL; the outputs are still written (zeros, -1 where npig is 0).      */
int cdetr_coco_image_stats(const uint8_t* matched, const uint8_t* det_ignored,   /* [A][T][Dtot], cdetr_coco_match's outputs, device */
                           const int32_t* dt_off,      /* [B+1] */
                           const int32_t* dt_cnt,      /* [B] or NULL: use only the first min(dt_cnt[b], segment length) detections of image b */
                           const int32_t* npig,        /* [A][B] */
                           const int32_t* cuts,        /* [M] ascending maxDets cuts */
                           const double* rec_thrs,     /* [R] */
                           int32_t B, int32_t A, int32_t T, int32_t Dtot, int32_t M, int32_t R,
                           int32_t* tp, int32_t* fp,   /* [A][B][T][M] */
                           double* ap,                 /* [A][B][T] */
                           void* stream);

/* ---- error breakdown (csrc/error_report.hip; infer.py --error_report): WHY a detection failed -- the single-class form of the TIDE
 * breakdown, which the reference does not have: duplicate, localisation, background, missed.  counting_detr_amd/error_report.py states the
 * rule in numpy; FLOAT64 and integers only, contraction into FMAs switched off, no atomics: every output EQUALS it bit for bit.
 * cdetr_coco_errors: ONE launch, one workgroup per image.  Images are packed as for cdetr_coco_match (gt_off / dt_off, detections in
 *   evaluation order); of image b the first n = min(dt_cnt[b], segment) detections are used (the whole segment without dt_cnt).  A ground truth
 *   is ignored when gt_ignore is set or its area is < area_lo or > area_hi.  All indices below are LOCAL to the image.
 *     the match    : cdetr_coco_match's greedy rule at the one threshold iou_fg (used as given), serial in the detections.
 *     best overlap : of detection d, the largest IoU over the non-ignored ground truths, taken or not, the highest index among equal IoUs;
 *                    (0.0, -1) when no IoU is > 0.
 *     dt_code      : 0 TP matched to a non-ignored ground truth; 1 IGN matched to an ignored one, or unmatched with an area outside the range;
 *                    else 2 DUP best >= iou_fg, 3 LOC iou_bg <= best < iou_fg, 4 BKG best < iou_bg; 255 beyond the prefix n.
 *     dt_gt, dt_iou: the matched ground truth and the IoU with it; unmatched: the best overlap (-1 and 0.0 when there is none, and beyond n).
 *     gt_code      : 1 IGN ignored; else 0 HIT matched; else 2 MISLOC the best overlap of at least one LOC detection; else 3 MISSED.
 *     gt_iou, gt_dt: the ground truth's largest IoU over the used detections (ignored ground truths too) and the lowest detection that
 *                    reaches it (-1 when it is 0); a HIT ground truth's gt_dt is the detection matched to it.
 *     counts[b]    : { TP, IGN, DUP, LOC, BKG detections; HIT, IGN, MISLOC, MISSED ground truths }.
 *   Wave 0 walks the greedy match (lanes over the ground truths, a taken-mask, a wave arg-max); the other 15 waves own the ground truths
 *   in blocks of 64, form every IoU once, keep the per-ground-truth maxima in registers and reduce each detection's best overlap; chunks
 *   of 64 detections are handed over through LDS and finished by one wave, the MISLOC marks set one detection after the other.
 *   EVERY element of the seven outputs is written exactly once, except the elements of a segment that does not lie inside 0 .. Gtot /
 *   0 .. Dtot or holds more than Gmax ground truths: such a segment counts as empty and is neither read nor written.
 *   Gmax = the largest ground-truth count of one image (host-known: it sizes the LDS image; limit 4096, CDETR_ERR_UNSUPPORTED beyond,
 *   before any launch); any number of detections.  B == 0: nothing is launched.  Gtot == 0 / Dtot == 0: their pointers may be NULL.
 *   Negative sizes, a NaN among the four numbers or a NULL where data is required: CDETR_ERR_ARG, before any launch.                     */
int cdetr_coco_errors(const double* gt_boxes,       /* [Gtot][4] xywh */
                      const double* gt_area,        /* [Gtot] */
                      const uint8_t* gt_ignore,     /* [Gtot] ignore or iscrowd */
                      const int32_t* gt_off,        /* [B+1] */
                      const double* dt_boxes,       /* [Dtot][4] xywh, evaluation order */
                      const double* dt_area,        /* [Dtot] */
                      const int32_t* dt_off,        /* [B+1] */
                      const int32_t* dt_cnt,        /* [B] or NULL */
                      int32_t B, int32_t Gtot, int32_t Dtot, int32_t Gmax, double iou_fg, double iou_bg, double area_lo, double area_hi,
                      uint8_t* dt_code, int32_t* dt_gt, double* dt_iou,    /* [Dtot] */
                      uint8_t* gt_code, int32_t* gt_dt, double* gt_iou,    /* [Gtot] */
                      int32_t* counts,              /* [B][9] */
                      void* stream);

/* ---- box overlays drawn on the device (csrc/render.hip; infer.py --render_worst / --render_ids): what the reference's evaluators draw with
 * cv2.rectangle / cv2.circle under `visualize_res` and never save (L2/offline_lvis_evaluator.py:167-207), as ONE launch over the chosen images
 * of a split, from the boxes and the IoU-0.5 flags cdetr_coco_match left in device memory.  Integers and float64 only, contraction into FMAs
 * switched off: every byte EQUALS counting_detr_amd/render.py's host implementation (the rule is stated there).
 * cdetr_render_boxes: canvas k (size[k] = {H, W}, its HWC bytes at pix + pix_off[k]) shows pack image b = sel[k]: its first
 *   min(dt_cnt[b], segment) detections (the whole segment dt_off[b] .. dt_off[b+1] without dt_cnt), its ground truths gt_off[b] .. gt_off[b+1]
 *   and the canvas's own exemplars ex_off[k] .. ex_off[k+1].  A box [x, y, w, h] has the integer corners x0 = floor(x), y0 = floor(y),
 *   x1 = floor(x + w), y1 = floor(y + h), each clamped to [-2, 32768] in float64 before the conversion; a non-finite field, x1 < x0 or y1 < y0
 *   draws nothing.  Its outline of thickness t: the canvas pixels inside the corners with min(px - x0, x1 - px, py - y0, y1 - py) < t.  A
 *   detection also has a centre dot, the square |px - cx| <= dot, |py - cy| <= dot around cx = floor(x + w * 0.5), cy = floor(y + h * 0.5)
 *   (dot < 0: none).  Detection i is `ignored` when det_ignored[i], else `tp` when matched[i], else `fp`.  A pixel takes the colour of the
 *   FIRST primitive that covers it in the order: dots (evaluation order), detection outlines (evaluation order), ground truths, exemplars;
 *   a pixel nothing covers keeps the image's.  EVERY byte of every canvas of `out` (laid out like pix) is written.
 *   style: [5][4] bytes (r, g, b, thickness) for tp, fp, ignored, ground truth, exemplar.
 *   One workgroup per (tile of CDETR_RENDER_TILE_H x _TILE_W pixels, canvas), the grid sized by max_h x max_w; a workgroup walks the
 *   canvas's primitives in that order in chunks of CDETR_RENDER_CHUNK: one primitive per thread culled against the tile, the survivors
 *   compacted in order into LDS (ballot + prefix), every pixel scanning them up to its first hit; it stops when all its pixels have one.
 *   No atomics, one writer per byte.  Every table entry is range-checked on the device before it addresses anything (B, D, G, E,
 *   pix_bytes): an inconsistent segment counts as empty, a canvas that does not lie inside pix_bytes or exceeds max_h / max_w is skipped.
 *   Validation, before any launch: negative sizes or a NULL where data is required CDETR_ERR_ARG; K > 65535, max_h / max_w outside
 *   1 .. 16384, a grid beyond 2^31 threads, dot > 16384 or an entry of sel_host (the caller's HOST copy of sel, may be NULL) outside
 *   [0, B): CDETR_ERR_UNSUPPORTED.  K == 0: nothing is launched.  D / G / E == 0: their pointers may be NULL.                         */
#define CDETR_RENDER_TILE_H 16
#define CDETR_RENDER_TILE_W 16
#define CDETR_RENDER_CHUNK 256
int cdetr_render_boxes(const uint8_t* pix,          /* canvases, HWC bytes, concatenated; device */
                       const int64_t* pix_off,      /* [K+1] byte offsets */
                       const int32_t* size,         /* [K][2] = H, W */
                       const int32_t* sel,          /* [K] pack image of canvas k */
                       const int32_t* sel_host,     /* HOST copy of sel for the range check, or NULL */
                       const double* dt_boxes,      /* [D][4] xywh, evaluation order */
                       const int32_t* dt_off,       /* [B+1] */
                       const int32_t* dt_cnt,       /* [B] or NULL */
                       const uint8_t* matched, const uint8_t* det_ignored,   /* [D]: row (area all, IoU 0.5) of cdetr_coco_match's outputs */
                       const double* gt_boxes,      /* [G][4] */
                       const int32_t* gt_off,       /* [B+1] */
                       const double* ex_boxes,      /* [E][4] */
                       const int32_t* ex_off,       /* [K+1] */
                       const uint8_t* style,        /* [5][4] */
                       int32_t K, int32_t B, int32_t D, int32_t G, int32_t E, int32_t max_h, int32_t max_w, int32_t dot, int64_t pix_bytes,
                       uint8_t* out, void* stream);

/* ---- image batches prepared on the device (csrc/image_prep.hip): what the reference's readers do per image on the host -- PIL resize,
 * ToTensor + Normalize (A2/data/fsc147.py:22-24, 75-77) -- plus this build's zero-padding to the batch maximum and its padding mask
 * (counting_detr_amd/data.py collate), in ONE launch, BIT-EQUAL to that host path.
 * cdetr_image_prep: image [B][3][Hm][Wm] fp32 and mask [B][Hm][Wm] bytes (1 = padding) from the un-resized uint8 RGB pixels of the batch.
 *   pixels : every image's [in_h][in_w][3] bytes, packed; images: one record of CDETR_IMAGE_PREP_RECORD_INTS int32 per image =
 *            { byte offset into pixels, in_h, in_w, out_h, out_w, h_bounds, h_coeffs, h_taps, v_bounds, v_coeffs, v_taps, 0 },
 *            the four table fields being offsets into `tables` in int32 entries.
 *   tables : per axis, bounds [out][2] = (first source sample, number of taps) and coeffs [out][taps] = Pillow's 8-bit coefficients
 *            (22 fractional bits; data.resample_tables).  Each pass: clamp((2^21 + sum sample * coeff) >> 22, 0, 255), horizontal first
 *            into uint8, vertical over that (Pillow's ImagingResample order); an unchanged axis carries the identity table (1 tap of 2^22).
 *   lut    : [3][256] fp32, the normalised value of byte v in channel c, built on the host with the host path's own expressions.
 *   Output pixel (y, x) of image b: inside out_h x out_w the resampled, normalised value and mask 0, elsewhere 0.0f and mask 1.  EVERY
 *   element of image and mask is written (no fill needed beforehand).  image must be 16-byte, mask 4-byte aligned.
 *   Supported scales, set by the LDS tile (CDETR_IMAGE_PREP_TILE_H x _TILE_W output pixels per workgroup): at most _MAX_TAPS taps per
 *   output sample and _MAX_ROWS source rows under _TILE_H output rows, i.e. DOWNSCALES up to 4x per axis for bicubic and bilinear
 *   (17 taps, 141 rows) and upscales of any factor.  max_taps / max_rows are the batch's own maxima, known on the host:
 *   CDETR_ERR_UNSUPPORTED beyond the limits (data.collate_raw resizes such an image on the host and passes it with identity tables).
 *   Records and table entries are range-checked on the device against pixel_bytes / table_ints before they address anything: an
 *   inconsistent record gives an all-padding image, never an access outside the buffers.                                          */
#define CDETR_IMAGE_PREP_TILE_H 32
#define CDETR_IMAGE_PREP_TILE_W 64
#define CDETR_IMAGE_PREP_MAX_TAPS 20
#define CDETR_IMAGE_PREP_MAX_ROWS 160
#define CDETR_IMAGE_PREP_RECORD_INTS 12
typedef struct {
    int32_t B, Hm, Wm;
    int32_t max_taps, max_rows;  /* largest h_taps / v_taps of the batch; largest source-row span of _TILE_H consecutive output rows */
    int32_t pad_;
    const uint8_t* pixels;
    int64_t pixel_bytes;
    const int32_t* images;       /* [B][CDETR_IMAGE_PREP_RECORD_INTS] */
    const int32_t* tables;
    int64_t table_ints;
    const float* lut;            /* [3][256] */
    float* image;                /* [B][3][Hm][Wm] */
    uint8_t* mask;               /* [B][Hm][Wm] */
} cdetr_image_prep_desc;
int cdetr_image_prep(const cdetr_image_prep_desc* d, void* stream);

/* ---- detections emitted on the device (csrc/detections.hip): what the reference's inference driver does per image on the host between
 * the forward and the evaluator -- threshold, scaling to original pixels, int() of every field (A2/infer.py:75-116) -- plus the evaluator's
 * box conversion (A2/eval_all.py:165-169) and COCOeval's detection order (descending score, stable, cut at maxDets), EQUAL to that host path
 * (infer.py's loop, coco_ap.reference_box, coco_ap.pack_images); FMA contraction is switched off in this translation unit.
 * cdetr_emit_detections: ONE call per forwarded batch (a count kernel and an emit kernel, one workgroup per image, on `stream`), appending
 *   the batch's images first .. first + B - 1 to a device-resident STORE that holds a whole split of N images:
 *     counts [N]       kept queries per image (prob >= threshold; a NaN probability is dropped);
 *     wire_off [N + 1] / eval_off [N + 1]: image n owns wire records wire_off[n] .. wire_off[n + 1] and evaluation records
 *                      eval_off[n] .. eval_off[n + 1].  The call READS entry `first` (written by the previous call in stream order; entry 0 is
 *                      zeroed by the caller once) and writes entries first + 1 .. first + B as running sums of this batch's own counts.
 *                      Placement is deterministic: no atomic decides where or in what order a record lands.
 *     wire [wire_cap][8] int32, QUERY order: with W = (float)ori_w, H = (float)ori_h and fx = box0 * W, fy = box1 * H, fw = box2 * W,
 *                      fh = box3 * H (one fp32 multiply each): { trunc(fx), trunc(fy), trunc(fw), trunc(fh), trunc(fw * fh) (fp32 product of
 *                      the unrounded fw, fh), trunc(px * W), trunc(py * H), the bits of the fp32 score } -- the bbox, area, point and score of a
 *                      predictions json annotation.  Truncation toward zero.
 *     eval_boxes [eval_cap][4], eval_area, eval_score [eval_cap] float64, EVALUATION order (descending score, equal scores in ascending
 *                      query order, at most max_det per image): with cx, cy, w, h the truncated wire integers,
 *                      box = { tdiv2(2 cx - w), tdiv2(2 cy - h), w, h } (integer division by 2 truncating toward zero = int(cx - w / 2); negative
 *                      for a box that overhangs the left / top edge), area = w * h, score = the fp32 score widened -- cdetr_coco_match's
 *                      dt_boxes / dt_area and the scores of the accumulation, image after image.
 *   Every range is checked against wire_cap / eval_cap (records) before anything is addressed: an image that does not fit writes NOTHING and
 *   ORs a bit into *status (1: wire records, 2: evaluation records, 4: the offsets at `first` do not describe this store); the offsets keep
 *   running.  The caller zeroes *status once and raises when it reads the store back.  Limits: Q <= 4096 (the keys of an image are sorted in
 *   LDS), B <= 65535, CDETR_ERR_UNSUPPORTED beyond; first + B <= N; capacities <= 2^30 records; wire 16-byte aligned.                       */
typedef struct {
    int32_t B, Q;               /* images in this batch, queries per image */
    int32_t N, first;           /* images the store holds; store index of this batch's first image */
    int32_t max_det;            /* cut of the evaluation records per image (COCOeval's maxDets[-1], 1100 in the reference) */
    int32_t wire_cap, eval_cap; /* capacities in records (worst case: N * Q and N * min(Q, max_det)) */
    float threshold;            /* a query is kept when prob >= threshold */
    const float* prob;          /* [B][Q] sigmoid(logit[..., 0]) as the counting rule formed it */
    const float* boxes;         /* [B][Q][4] normalised cxcywh */
    const float* points;        /* [B][Q][2] normalised reference points (x, y) */
    const int32_t* orig_hw;     /* [B][2] original (height, width) in pixels */
    int32_t* counts;            /* [N] */
    int32_t* wire_off;          /* [N + 1] */
    int32_t* eval_off;          /* [N + 1] */
    int32_t* wire;              /* [wire_cap][8] */
    double* eval_boxes;         /* [eval_cap][4] xywh */
    double* eval_area;          /* [eval_cap] */
    double* eval_score;         /* [eval_cap] */
    int32_t* status;            /* [1] overflow bits, zeroed by the caller once */
} cdetr_emit_detections_desc;
int cdetr_emit_detections(const cdetr_emit_detections_desc* d, void* stream);

/* ---- the counting rule at T thresholds in one pass (csrc/threshold_sweep.hip; infer.py --sweep_thresholds).
 * cdetr_count_sweep: table[first + b][t] = #{q : prob[b][q] >= thresholds[t]} for the B images of a forwarded batch, fp32 compares (a NaN
 *   probability is never counted), EQUAL to numpy's `prob >= numpy.float32(t)` summed over the row.  One launch, one workgroup per image:
 *   every query's bin k = #{t : p >= thresholds[t]} goes through wave ballots and popcounts into an LDS histogram of T + 1 integer bins,
 *   whose suffix sums are the row -- which is why `thresholds` must be ASCENDING (equal neighbours allowed).  Integer arithmetic only, no
 *   atomic in global memory, one writer per cell: deterministic.  `table` is the device-resident [N][T] table of one split; only rows
 *   first .. first + B - 1 are written.  Limits: any Q >= 1; 1 <= T <= 32 and B <= 65535, CDETR_ERR_UNSUPPORTED beyond; first >= 0 and
 *   first + B <= N, CDETR_ERR_ARG otherwise (B, Q, T < 1 too).  Nothing is launched on an error.                                           */
int cdetr_count_sweep(const float* prob, const float* thresholds, int32_t B, int32_t Q, int32_t T, int32_t* table, int32_t N, int32_t first,
                      void* stream);

/* ---- bootstrap replicates over images (csrc/bootstrap.hip; infer.py / main.py --bootstrap R), which the reference does not have.
 * counting_detr_amd/bootstrap.py states the rule in numpy; integers and FLOAT64 only, contraction into FMAs switched off, no atomics in
 * global memory: every output EQUALS it bit for bit.  Replicate r of a split of N images has the multiplicities m[i] = #{j < N : draw(j) == i},
 * all uint64 modulo 2^64:  x = (seed * 0x9E3779B97F4A7C15) ^ ((r << 32) | j);  x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 * x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^= x >> 31;  draw = ((x >> 32) * N) >> 32.  The workgroup that owns a replicate builds m in
 * LDS (integer adds into LDS counters: order-free).  `mult` [R][N], when not NULL, is taken INSTEAD of the draws (row rb for replicate
 * r0 + rb, every entry clamped into 0 .. 16384): hand-made weights for the tests.  The launch computes replicates r0 .. r0 + R - 1.
 * Limits of all three: N <= 16384 images (m is 64 KB of LDS) and r0 + R <= 10000 replicates, CDETR_ERR_UNSUPPORTED beyond, naming the limit,
 * before any launch; R == 0 launches nothing.
 * cdetr_bootstrap_counts: one workgroup per replicate; for count column c (lane c of the first wave) with err_i = |gt[i] - pred[i][c]|, adding
 *   in image order:  S [rb][c] = { sum m_i err_i, sum m_i err_i^2 } (int64),  F [rb][c] = { sum m_i * (err_i / gt_i), sum m_i * (err_i^2 / gt_i) }
 *   (float64; one division and one product per term, no term where gt_i == 0).  pred is [N][ld] with Tc <= ld: the table cdetr_count_sweep
 *   left on the device, or one uploaded column.  1 <= Tc <= 32.
 * cdetr_bootstrap_gather: the flags of cdetr_coco_match [A][T][Dtot] -> words [A][P], position p = detection order[p] (the merged order,
 *   computed once on the host): bit t = matched && !ignored at IoU threshold t, bit 16 + t = !matched && !ignored.  T == 10 exactly.  An
 *   order entry outside 0 .. Dtot gives the word 0 and nothing is read.
 * cdetr_bootstrap_ap: grid (replicate, area range), one wave per IoU threshold.  With w_p = m[image[p]] (0 for an image index outside
 *   0 .. N), ctp_p / cfp_p the weighted inclusive prefix sums of the tp / fp bits and npig_r = sum_i m_i npig[a][i]:
 *     precision [rb][a][t][s] = -1 when npig_r == 0; else the maximum of ctp_p / ((cfp_p + ctp_p) + eps) over the positions of weight > 0 with
 *                              ctp_p / npig_r >= rec_thrs[s], 0 when there is none
 *   = coco_ap._sample on the weighted list = coco_ap.accumulate on the list with every detection repeated m times.  Any P >= 0 (P == 0: the
 *   pointers may be NULL; zeros, or -1); T == 10 exactly, n_rec <= 128.  Every element of `precision` is written exactly once.             */
int cdetr_bootstrap_counts(const int32_t* gt,          /* [N] ground-truth counts */
                           const int32_t* pred,        /* [N][ld] predicted counts, columns 0 .. Tc - 1 used */
                           int32_t ld,
                           const int32_t* mult,        /* [R][N] or NULL */
                           int64_t seed, int32_t r0, int32_t R, int32_t N, int32_t Tc,
                           int64_t* S,                 /* [R][Tc][2] */
                           double* F,                  /* [R][Tc][2] */
                           void* stream);
int cdetr_bootstrap_gather(const uint8_t* matched, const uint8_t* det_ignored,   /* [A][T][Dtot], cdetr_coco_match's outputs, device */
                           const int32_t* order,       /* [P] */
                           int32_t A, int32_t T, int32_t Dtot, int32_t P,
                           int32_t* words,             /* [A][P] */
                           void* stream);
int cdetr_bootstrap_ap(const int32_t* words,           /* [A][P], cdetr_bootstrap_gather's output */
                       const int32_t* image,           /* [P] image of every position */
                       const int32_t* npig,            /* [A][N] */
                       const int32_t* mult,            /* [R][N] or NULL */
                       const double* rec_thrs,         /* [n_rec] */
                       int64_t seed, int32_t r0, int32_t R, int32_t N, int32_t P, int32_t A, int32_t T, int32_t n_rec,
                       double eps,                     /* numpy.spacing(1) */
                       double* precision,              /* [R][A][T][n_rec] */
                       void* stream);

/* ---- greedy non-maximum suppression ahead of the emit (csrc/nms.hip; infer.py --nms_iou): a FILTER on prob, EQUAL to the host rule of
 * counting_detr_amd/nms.py; FMA contraction is switched off in this translation unit.
 * cdetr_nms_suppress: ONE launch per forwarded batch, one workgroup per image.  The candidates of image b are the queries with
 *   prob >= threshold in fp32 (a NaN is never one), walked by descending prob, equal probabilities in ascending query order (the order of the
 *   evaluation records of cdetr_emit_detections, not cut at any max_det).  A candidate's box is its evaluation box, the integers
 *   { tdiv2(2 cx - w), tdiv2(2 cy - h), w, h } of the truncated fp32 products with the original width / height, widened to float64.  A
 *   candidate is suppressed when its IoU (coco_ap.box_iou_xywh: float64, the division performed, 0 where the union is not positive) with an
 *   earlier SURVIVING candidate is > iou, strictly; a suppressed candidate suppresses nobody.
 *     prob_out [B][Q]  prob with every suppressed entry replaced by a quiet NaN; every other entry keeps its bits (NaNs, -0 and everything
 *                      below the threshold included).  Every entry is written once and none is read; prob_out must not alias prob.
 *     removed [B]      suppressed candidates per image.
 *   The sorted keys of an image (32 KiB at the limit), the 64 boxes of the chunk being resolved and one flag byte per query live in LDS, under
 *   the 64 KiB static default; each thread keeps the boxes of its own <= 4 candidates in registers.  No atomics.  Limits: Q <= 4096,
 *   B <= 65535, CDETR_ERR_UNSUPPORTED beyond; B, Q >= 1, a finite iou in [0, 1], a threshold that is not NaN and non-NULL pointers,
 *   CDETR_ERR_ARG otherwise.  Nothing is launched on an error.                                                                          */
typedef struct {
    int32_t B, Q;               /* images in this batch, queries per image */
    float threshold;            /* a query is a candidate when prob >= threshold */
    int32_t pad_;
    double iou;                 /* suppressed when the IoU with an earlier survivor is > iou */
    const float* prob;          /* [B][Q] */
    const float* boxes;         /* [B][Q][4] normalised cxcywh */
    const int32_t* orig_hw;     /* [B][2] original (height, width) in pixels */
    float* prob_out;            /* [B][Q] */
    int32_t* removed;           /* [B] */
} cdetr_nms_suppress_desc;
int cdetr_nms_suppress(const cdetr_nms_suppress_desc* d, void* stream);

/* ---- stage-1 pseudo labels emitted on the device (csrc/stage1_labels.hip): what the 1st stage's label writer does per annotated dot on the
 * host between the forward and pseudo_bbox_<split>.json (A1/engine.py:124-187; stage1.write_pseudo_labels' loop), plus the offline
 * evaluator's reading of that file (A1/offline_coco_evaluator.py:134-143: [cx, cy, w, h] -> a detection [cx - w/2, cy - h/2, w, h] of score
 * 1.0) and the IoU of every pseudo box with the ground-truth box its dot is the centre of, EQUAL to the host path (the loop,
 * stage1.score_pseudo_labels, coco_ap.box_iou_xywh); FMA contraction is switched off in this translation unit.
 * cdetr_emit_pseudo_labels: ONE launch per forwarded batch on `stream` (workgroups of 256 rows x B images), appending the batch's images
 *   first .. first + B - 1 to a device-resident STORE that holds a whole split of N images:
 *     img_counts [N]   rows per image (counts[b], or R for a dense batch);
 *     row_off [N + 1] / eval_off [N + 1]: image n owns wire records and paired IoUs row_off[n] .. row_off[n + 1] and evaluation records
 *                      eval_off[n] .. eval_off[n + 1].  The call READS entry `first` (written by the previous call in stream order; entry 0 is
 *                      zeroed by the caller once) and writes entries first + 1 .. first + B as running sums of this batch's own counts.
 *                      Placement is deterministic: no atomic decides where a record lands.
 *     wire [row_cap][8] int32, ROW order: with W = (float)ori_w, H = (float)ori_h and xf = px * W, yf = py * H, wf = pw * W, hf = ph * H
 *                      (one fp32 multiply each): { store image index n, trunc(xf), trunc(yf), trunc(wf), trunc(hf), trunc(wf * hf) (fp32
 *                      product of the unrounded wf, hf), 0, 0 } -- image, bbox and area of a pseudo_bbox annotation.  Truncation toward zero.
 *     pair_iou [row_cap] float64: with gt_xywh, the IoU (pycocotools bbIou, the operations of coco_ap.box_iou_xywh in float64) of the row's
 *                      evaluation box with gt_xywh[b][r]; 0.0 without.
 *     eval_boxes [eval_cap][4], eval_area, eval_score [eval_cap] float64: the first min(counts[b], max_det) rows of each image in row order
 *                      (all scores tie and COCOeval's sort is stable): with cx, cy, w, h the wire integers, box = { cx - w / 2.0,
 *                      cy - h / 2.0, w, h } (NOT truncated again), area = w * h, score = 1.0 -- cdetr_coco_match's dt_boxes / dt_area.
 *   Every range is checked against row_cap / eval_cap (records) before anything is addressed: an image that does not fit writes NOTHING and
 *   ORs a bit into *status (1: wire records, 2: evaluation records, 4: the offsets at `first` do not describe this store, 8: a count outside
 *   0 .. R, taken as 0); offsets stop at the capacity.  counts[b] == 0 writes nothing and leaves the image's offsets equal.  The caller zeroes
 *   *status once and raises when it reads the store back.  Limits: R <= 2^20, B <= 65535, CDETR_ERR_UNSUPPORTED beyond; first + B <= N;
 *   capacities <= 2^30 records; wire 16-byte, points / pred_wh 8-byte aligned.                                                          */
typedef struct {
    int32_t B, R;               /* images in this batch, (padded) rows per image */
    int32_t N, first;           /* images the store holds; store index of this batch's first image */
    int32_t max_det;            /* cut of the evaluation records per image (COCOeval's maxDets[-1], 1100 in the reference) */
    int32_t row_cap, eval_cap;  /* capacities in records */
    int32_t pad_;
    const float* points;        /* [B][R][2] normalised query points (x, y) */
    const float* pred_wh;       /* [B][R][2] predicted normalised (w, h) */
    const int32_t* counts;      /* [B] valid rows of each image; NULL = every row (a dense batch) */
    const int32_t* orig_wh;     /* [B][2] original (width, height) in pixels */
    const double* gt_xywh;      /* [B][R][4] ground-truth boxes in original pixels, same row padding; NULL = no pairing */
    int32_t* img_counts;        /* [N] */
    int32_t* row_off;           /* [N + 1] */
    int32_t* eval_off;          /* [N + 1] */
    int32_t* wire;              /* [row_cap][8] */
    double* pair_iou;           /* [row_cap] */
    double* eval_boxes;         /* [eval_cap][4] xywh */
    double* eval_area;          /* [eval_cap] */
    double* eval_score;         /* [eval_cap] */
    int32_t* status;            /* [1] overflow bits, zeroed by the caller once */
} cdetr_emit_pseudo_labels_desc;
int cdetr_emit_pseudo_labels(const cdetr_emit_pseudo_labels_desc* d, void* stream);

/* ---- tiled inference past the query cap (csrc/tiling.hip; infer.py --tiles RxC): the device steps around the grouped forward of an image's
 * tiles, EQUAL to the host rule of counting_detr_amd/tiling.py; FMA contraction is switched off in this translation unit.
 * cdetr_tile_images: ONE launch per image.  image [3][H][W] fp32 and one record of CDETR_TILE_RECORD_INTS int32 per tile = { x0, y0, width,
 *   height (the crop, in pixels of the image), scale (1 or 2) } -> tiles [T][3][Hm][Wm] fp32 and mask [T][Hm][Wm] bytes (1 = padding); every
 *   element of both is written.  Scale 1 copies the crop.  Scale 2: output sample j of an axis takes the source pixel x0 + j / 2 with weight
 *   0.75 and its left (j even) or right (j odd) neighbour, clamped to the IMAGE, with 0.25; horizontal pass first, the vertical pass over its
 *   result, each pass 0.75f * a + 0.25f * b rounded per operation.  A record is range-checked on the device before it addresses anything
 *   (inside the image, width * scale <= Wm, height * scale <= Hm): a bad one gives an all-padding tile.  Limits: sides <= CDETR_TILE_MAX_SIDE,
 *   T <= CDETR_TILE_MAX_VIRTUAL, CDETR_ERR_UNSUPPORTED beyond.
 * cdetr_exemplar_group_fwd: cdetr_exemplar_fwd with per_image set for tiles that share their exemplars: x [B][h*w][C], rects [B][K][4],
 *   extent [B][2], groups of G consecutive tiles (B % G == 0).  pf [B][C]: every tile of a group gets (sum of x[tile][cell] over the group's
 *   tiles in order and k in order, present rows only, fp32 running sum) * (1 / max(cnt, 1)); idx [B][K]: cell or -1.  Forward only.  G = 1
 *   equals cdetr_exemplar_fwd bit for bit.
 * cdetr_tile_stitch: prob [T][Q], boxes [T][Q][4] cxcywh, points [T][Q][2] of an image's tiles and CDETR_TILE_COEF_FLOATS fp32 per tile =
 *   { ax, ox, ay, oy, lo_x, hi_x, lo_y, hi_y } -> the virtual image of Qv = slots * Q queries (virtual query t * Q + q = query q of tile t):
 *   centres and points v * a + o, sizes v * a (one fp32 multiply, one fp32 add); prob kept iff lo <= centre * (float)W / (float)H < hi on
 *   both axes, an infinite bound being no bound, NaN otherwise; slots T .. slots - 1 are NaN with zero boxes and points.  Every one of the
 *   Qv entries of the three outputs is written once, no atomics; outputs must not alias inputs.  Limit: slots * Q <= CDETR_TILE_MAX_VIRTUAL
 *   (what cdetr_emit_detections and cdetr_nms_suppress take), CDETR_ERR_UNSUPPORTED beyond.                                            */
#define CDETR_TILE_RECORD_INTS 5
#define CDETR_TILE_COEF_FLOATS 8
#define CDETR_TILE_MAX_SIDE 16384
#define CDETR_TILE_MAX_VIRTUAL 4096
int cdetr_tile_images(const float* image, int32_t H, int32_t W, const int32_t* records, int32_t T, int32_t Hm, int32_t Wm, float* tiles,
                      uint8_t* mask, void* stream);
int cdetr_exemplar_group_fwd(const float* x, const float* rects, const float* extent, int32_t B, int32_t G, int32_t h, int32_t w, int32_t C,
                             int32_t K, int32_t* idx, float* pf, void* stream);
int cdetr_tile_stitch(const float* prob, const float* boxes, const float* points, const float* coef, int32_t T, int32_t Q, int32_t slots,
                      int32_t H, int32_t W, float* prob_out, float* boxes_out, float* points_out, void* stream);

const char* cdetr_last_error(void);
int cdetr_abi_version(void);
/* Stream plumbing of the trainer (no reference counterpart: the reference runs one stream and drains it every step, A2/engine.py:33-57).
 * cdetr_delay: one idle wavefront for `us` microseconds -- holds `stream` back without occupying the chip (stream-concurrency probe).
 * cdetr_flag_signal / cdetr_flag_wait: ordering between two streams from INSIDE captured graphs, where no event can be recorded: the signal
 *   (one thread) adds 1 to *flag; the wait (one thread, at the head of the other stream's work) sleeps until *flag has passed *seen -- its own
 *   count of consumed signals, updated by the kernel -- or `timeout_us` has gone by (a missing signal costs a delay, never a hang).
 *   Every signal needs exactly one wait: a wait advances *seen by one (to the flag's value when it was satisfied, by one when it timed out
 *   and the signal arrives later), so a signal nobody waited for leaves the flag one ahead and every later wait passes at once.  A replay
 *   whose signal has no waiter CONSUMES it with timeout_us = 0 (advances *seen by one, whichever side of the signal it lands on).
 *   The flags are a SCHEDULING hint only: whatever must hold for correctness is ordered by events / stream order as well.
 *   engine.Trainer releases the next batch's frozen stage (A2/models/backbone.py:93-95) the moment the Hungarian solve of the current step
 *   (A2/models/matcher.py:243-247) is about to start: the solve needs one whole compute unit's LDS for its cost matrix.                   */
int cdetr_delay(int32_t us, void* stream);
int cdetr_flag_signal(int32_t* flag, void* stream);
int cdetr_flag_wait(const int32_t* flag, int32_t* seen, int32_t timeout_us, int32_t post_us, void* stream);   /* post_us: idle on after the signal */

/* ---- glue (csrc/glue.hip): the small steps between the GEMMs, one launch each -------------------------------------------------
 * cdetr_mask_prep: padding mask [B][H][W] (bytes, non-zero = padding) -> m [B][h][w] (nearest-neighbour down-sampling,
 *   A2/models/backbone.py:143), mask_row [B][w] = m[:, 0, :], mask_col [B][h] = m[:, :, 0] (the RCDA key masks,
 *   row_column_decoupled_attention.py:238-249), pos_row [B][w] / pos_col [B][h] = mask2pos (A2/models/transformer.py:497-503),
 *   extent [B][2] = un-padded (rows, columns) of each image in feature cells.
 * cdetr_stem_pack: images NCHW [B][3][H][W] -> xp [B][Ha][Wa][4] NHWC, image at (pad_y, pad_x), zeros elsewhere, 4th channel 0
 *   (input of the row-packed 7x7 stem, A2/models/resnet.py:178-180).
 * cdetr_exemplar_fwd: pf[b][c] = mean over the present exemplars k of x[b][cell(b,k)][c] with x [B][h*w][C] NHWC, rects [B][K][4]
 *   normalised xyxy (x2 < 0: absent), cell = centre of the box in feature cells, truncated (A2/models/backbone.py:122-131);
 *   per_image: image b uses rects[b] and extent[b]; else rects[0] scaled by (h, w) for every image (the reference's rule).
 *   Writes idx [B][K] (cell or -1) and inv_cnt [B] for the backward.   cdetr_exemplar_bwd: dx[b][cell][c] += dpf[b][c] * inv_cnt[b].
 * cdetr_aggr_weight_fwd: Weff[b] = W[:, :C] + W[:, C:] * pf[b] ([B][d][C]) and its transpose WeffT [B][C][d]; W is [d][2C]
 *   (A2/models/backbone.py:132-136 + anchor_detr.py:119 with the concatenation folded into the weight).
 * cdetr_aggr_weight_bwd: from dWeff [B][d][C]: gW[:, :C] += sum_b dWeff[b]; gW[:, C:] += sum_b dWeff[b] * pf[b] (gW may be NULL);
 *   dpf[b][c] += sum_o dWeff[b][o][c] * W[o][C + c]  (dpf must be zeroed by the caller).  B <= 16.
 * cdetr_box_head_fwd: boxes[m] = sigmoid(tmp[m] + [inverse_sigmoid(ref[m % R]), 0, 0]); tmp / boxes [M][4], ref [R][2], M % R == 0
 *   (A2/models/transformer.py:193-203, A2/util/misc.py:475-479).  cdetr_box_head_bwd: d_tmp = d_boxes * s (1 - s) and, when d_ref is
 *   not NULL, d_ref[m % R] (+)= d_tmp[:2] * d inverse_sigmoid (torch's clamp-backward rule; plain store when M == R, else atomic
 *   accumulation into a caller-zeroed buffer).                                                                                  */
int cdetr_mask_prep(const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w, uint8_t* m, uint8_t* mask_row,
                    uint8_t* mask_col, float* pos_row, float* pos_col, float* extent, void* stream);
int cdetr_stem_pack(const float* images, float* xp, int32_t B, int32_t H, int32_t W, int32_t Ha, int32_t Wa, int32_t pad_y, int32_t pad_x,
                    void* stream);
int cdetr_exemplar_fwd(const float* x, const float* rects, const float* extent, int32_t per_image, int32_t B, int32_t h, int32_t w,
                       int32_t C, int32_t K, int32_t* idx, float* inv_cnt, float* pf, void* stream);
int cdetr_exemplar_bwd(const float* dpf, const int32_t* idx, const float* inv_cnt, float* dx, int32_t B, int32_t P, int32_t C, int32_t K,
                       void* stream);
int cdetr_aggr_weight_fwd(const float* W, const float* pf, float* Weff, float* WeffT, int32_t B, int32_t d, int32_t C, void* stream);
int cdetr_aggr_weight_bwd(const float* dWeff, const float* pf, const float* W, float* gW, float* dpf, int32_t B, int32_t d, int32_t C,
                          void* stream);
int cdetr_box_head_fwd(const float* tmp, const float* ref, float* boxes, int32_t M, int32_t R, void* stream);
int cdetr_box_head_bwd(const float* d_boxes, const float* boxes, const float* ref, float* d_tmp, float* d_ref, int32_t M, int32_t R,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
