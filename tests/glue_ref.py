"""Checker of the transformer glue and normalisation kernels (csrc/elementwise.hip: LayerNorm, the positional adds, the key means, the
broadcast-back, the gradient merges, the ReLU mask, the sine embedding; csrc/igemm.hip: the column sum and the stem max-pool): every
operation restated in fp64 torch on the CPU, with the arguments of its `ops` wrapper and no kernel involved.  Inputs may be fp32 or
fp64 tensors on any device; results are fp64 on the CPU.  Scalars that cross the C ABI as `float` (scales) are taken at their fp32
value, which is what the kernel is given.  tests/test_glue_ref_cpu.py checks these restatements against torch's own operators and
autograd; tests/test_glue_kernels_gpu.py holds the kernels to them.  Not product code: nothing under counting_detr_amd imports it."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)

# The project's LayerNorm bar, `close(..., rtol=1e-5)` with its default atol_scale = 2e-5: max error <= (1e-5 + 2e-5) * max|reference|
LN_BAR = 1e-5 + 2e-5
# Far-mean data: the bar is the larger of LN_BAR and this factor times the error of the fp32 two-pass yardstick on the same inputs (a
# different but equally valid fp32 summation order may be a few times worse than the yardstick's; the one-pass form is ~150x worse)
FAR_MEAN_FACTOR = 4.0


def d(t):
    """fp64 CPU copy (None stays None)."""
    return None if t is None else t.detach().to("cpu", torch.float64)


def f32(s):
    """A Python scalar at the fp32 value the C ABI passes, as a Python float."""
    return torch.tensor(float(s), dtype=torch.float32).double().item()


def bf16_rne(t):
    """bf16 of an fp32 tensor, round to nearest even: what every bf16 twin and hi plane must hold."""
    return t.to(torch.bfloat16)


def split_planes(t):
    """(hi, lo) planes of an fp32 tensor, exactly as ops.split_planes: hi = bf16(t), lo = bf16(t - hi)."""
    hi = bf16_rne(t)
    return hi, bf16_rne(t - hi.float())


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def layer_norm_fwd(x, gamma, beta, eps):
    """-> y, mean, rstd over the last dim of x [rows, C] (biased variance, as nn.LayerNorm)."""
    x, gamma, beta = d(x), d(gamma), d(beta)
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = ((xc * xc).mean(-1) + eps) ** -0.5
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def layer_norm_bwd(dy, x, gamma, eps, add=None):
    """-> dx (+ add), dgamma, dbeta in closed form: dx = rstd (dy g - mean_c(dy g) - xhat mean_c(dy g xhat))."""
    dy, x, gamma = d(dy), d(x), d(gamma)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = ((xc * xc).mean(-1, keepdim=True) + eps) ** -0.5
    xhat = xc * rstd
    dg = dy * gamma
    dx = rstd * (dg - dg.mean(-1, keepdim=True) - xhat * (dg * xhat).mean(-1, keepdim=True))
    if add is not None:
        dx = dx + d(add)
    return dx, (dy * xhat).sum(0), dy.sum(0)


def layer_norm_f32_two_pass(x, gamma, beta, eps, dy, add=None, dgamma0=0.0, dbeta0=0.0):
    """The same forward and backward in plain fp32 tensor ops -- mean first, then the centred second moment -> dict of y, mean, rstd,
    dx, dgamma, dbeta (dgamma0 / dbeta0: what the accumulators held before).  The yardstick of what fp32 can do on hard data, NOT a
    reference."""
    x, gamma, beta, dy = (t.detach().to("cpu", torch.float32) for t in (x, gamma, beta, dy))
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = ((xc * xc).mean(-1, keepdim=True) + eps).rsqrt()
    xhat = xc * rstd
    y = xhat * gamma + beta
    dg = dy * gamma
    dx = rstd * (dg - dg.mean(-1, keepdim=True) - xhat * (dg * xhat).mean(-1, keepdim=True))
    if add is not None:
        dx = dx + add.detach().to("cpu", torch.float32)
    return dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dgamma=(dy * xhat).sum(0) + dgamma0, dbeta=dy.sum(0) + dbeta0)


def layer_norm_f32_one_pass(x, gamma, beta, eps):
    """y with the variance formed as E[x^2] - E[x]^2 in fp32: the form the far-mean bar must reject (tests/test_glue_ref_cpu.py)."""
    x, gamma, beta = (t.detach().to("cpu", torch.float32) for t in (x, gamma, beta))
    mean = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mean * mean
    return (x - mean) * (var + eps).rsqrt() * gamma + beta


def rel_err(actual, ref):
    """max |actual - ref| relative to max |ref| (the measure of the project's `close`)."""
    a, r = d(actual), d(ref)
    return ((a - r).abs().max() / (r.abs().max() + 1e-30)).item()


def far_mean_bar(yardstick_err):
    return max(LN_BAR, FAR_MEAN_FACTOR * yardstick_err)


def far_mean_input(rows, C, generator):
    return 100.0 + 0.5 * torch.randn(rows, C, generator=generator)


# ----------------------------------------------------------------------------------------------------- map-shaped glue
def posadd2(X, Prow, Pcol):
    """Qr[n,y,x,:] = X + Prow[n,x,:], Qc[n,y,x,:] = X + Pcol[n,y,:] for X [N,H,W,C], Prow [N,W,C], Pcol [N,H,C]."""
    X, Prow, Pcol = d(X), d(Prow), d(Pcol)
    return X + Prow[:, None, :, :], X + Pcol[:, :, None, :]


def hw_reduce(Xr, Xc, Ar, Ac, sr, sc):
    """Or[n,x,:] = sr sum_y Xr[n,y,x,:] (+ Ar[n,x,:]), Oc[n,y,:] = sc sum_x Xc[n,y,x,:] (+ Ac[n,y,:])."""
    Or = f32(sr) * d(Xr).sum(1)
    Oc = f32(sc) * d(Xc).sum(2)
    if Ar is not None:
        Or = Or + d(Ar)
    if Ac is not None:
        Oc = Oc + d(Ac)
    return Or, Oc


def bcast_add2_sum(T, T2, T3, Br, Bc, sr, sc):
    """T (+ T2) (+ T3) + sr Br[n,x,:] + sc Bc[n,y,:]."""
    out = d(T)
    if T2 is not None:
        out = out + d(T2)
    if T3 is not None:
        out = out + d(T3)
    return out + f32(sr) * d(Br)[:, None, :, :] + f32(sc) * d(Bc)[:, :, None, :]


# ------------------------------------------------------------------------------------------------------------ flat glue
def add2(T, A, B=None):
    """-> (T + A, T + B or None)."""
    return d(T) + d(A), (None if B is None else d(T) + d(B))


def grad_merge(base, g1, g2=None, acc1=None, acc2=None):
    """-> out = base + g1 (+ g2) and the updated accumulators acc1 + g1, acc2 + g2 (None where absent)."""
    out = d(base) + d(g1)
    if g2 is not None:
        out = out + d(g2)
    return out, (None if acc1 is None else d(acc1) + d(g1)), (None if acc2 is None else d(acc2) + d(g2))


def relu_mask(y, dy, scale):
    """dz = (y > 0) ? dy * scale : 0; a NaN, a zero of either sign or a negative y gives 0."""
    y, dy = d(y), d(dy)
    return torch.where(y > 0, dy * f32(scale), torch.zeros_like(dy))


def colsum(X, out):
    """out[n] + sum_m X[m][n]."""
    return d(out) + d(X).sum(0)


def maxpool3x3s2(x_nhwc):
    """3x3 window, stride 2, one pixel of -inf padding, on an NHWC map -> [N, (H-1)//2+1, (W-1)//2+1, C]."""
    x = d(x_nhwc)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=-math.inf)
    out = torch.full((N, Ho, Wo, C), -math.inf, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out = torch.maximum(out, xp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :])
    return out


# ------------------------------------------------------------------------------------------------------- sine embedding
def _sine_angle(pos, nfeat, T):
    i = torch.arange(nfeat, dtype=torch.float64)
    inv = (2 * math.pi) / float(T) ** (2 * torch.div(i, 2, rounding_mode="floor") / nfeat)       # d angle / d pos per feature
    return pos.to(torch.float64)[..., None] * inv, inv, (torch.arange(nfeat) % 2 == 1)


def sine_embed(pos, nfeat, T=10000.0):
    """out[..., i] = sin(a_i) for even i, cos(a_i) for odd i, a_i = 2 pi pos / T^(2 floor(i/2) / nfeat).  Differentiable in pos."""
    a, _, odd = _sine_angle(pos, nfeat, T)
    return torch.where(odd, a.cos(), a.sin())


def sine_embed_bwd(pos, dout, nfeat, T=10000.0):
    """dpos = sum_i dout[..., i] * d out_i / d pos, in closed form."""
    a, inv, odd = _sine_angle(d(pos), nfeat, T)
    return (d(dout) * torch.where(odd, -a.sin(), a.cos()) * inv).sum(-1)
