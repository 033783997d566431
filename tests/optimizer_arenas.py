"""Shared by the optimizer-kernel tests (test_sgd_kernel_gpu.py, test_adamw_kernel_gpu.py, test_trainer_arena_gpu.py): flat arenas on the
device with the kernels' calling sequence, torch.optim.AdamW after clip_grad_norm_ restated in fp64 (the reference) and in float32 NumPy
(the yardstick the tolerances are measured with), and well-posed Adam states.  Nothing here is written from the kernel: the formulas are
torch's (torch/optim/adamw.py, _single_tensor_adamw; torch/nn/utils/clip_grad.py)."""
import numpy as np
import torch

DEV = "cuda"
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8          # torch.optim.AdamW's defaults, as Python doubles (what torch computes with)
ULP4 = 4.0 * 2.0 ** -23                       # floor of every bar: 4 fp32 ulp of the tensor's scale


def g(seed):
    return torch.Generator().manual_seed(seed)


class Arenas:
    """p, g and the optimizer state (buf for SGD; m, v as well with adam=True) (+ the optional lr table) on the device, the state block
    [step, lr scale, norm, skipped] and the sumsq workspace."""

    def __init__(self, n, seed=0, lr_table=None, lr0=0.0, lr1=0.0, split=0, adam=False):
        self.n = n
        self.p = torch.randn(n, generator=g(seed)).to(DEV)
        self.g = (torch.randn(n, generator=g(seed + 1)) * 0.05).to(DEV)
        self.buf = torch.zeros(n, device=DEV)
        if adam:
            self.m = torch.zeros(n, device=DEV)
            self.v = torch.zeros(n, device=DEV)
        self.lr = None if lr_table is None else lr_table.to(DEV)
        self.lr0, self.lr1, self.split = lr0, lr1, split
        self.state = torch.tensor([0.0, 1.0, 0.0, 0.0], device=DEV)
        self.sumsq = torch.zeros(1, device=DEV)
        self.ws = torch.zeros(2048, device=DEV)

    def base_lr(self):
        if self.lr is not None:
            return self.lr.double().cpu()
        i = torch.arange(self.n)
        return torch.where(i < self.split, torch.tensor(self.lr0, dtype=torch.float64), torch.tensor(self.lr1, dtype=torch.float64))

    def load(self, **tensors):
        """Copy CPU tensors into the named arenas (p, g, m, v, buf)."""
        for k, t in tensors.items():
            getattr(self, k).copy_(t.to(torch.float32).to(DEV))

    def _sumsq(self, L, st):
        from counting_detr_amd import _ffi
        _ffi.check(L.cdetr_sumsq(self.g.data_ptr(), self.n, self.sumsq.data_ptr(), self.ws.data_ptr(), st), "cdetr_sumsq")

    def step(self, max_norm, momentum, wd, grad_div=1.0):
        from counting_detr_amd import _ffi
        L, st = _ffi.lib(), _ffi.stream_ptr()
        self._sumsq(L, st)
        _ffi.check(L.cdetr_sgd_step(self.p.data_ptr(), self.g.data_ptr(), self.buf.data_ptr(), None if self.lr is None else self.lr.data_ptr(),
                                    self.lr0, self.lr1, self.split, self.n, self.sumsq.data_ptr(), self.state.data_ptr(), max_norm, momentum,
                                    wd, grad_div, st), "cdetr_sgd_step")
        torch.cuda.synchronize()

    def step_adamw(self, entry, max_norm, wd, grad_div=1.0, beta1=BETA1, beta2=BETA2, eps=EPS):
        """entry "step": cdetr_adamw_step (needs the table); "step2": cdetr_adamw_step2 (table, or lr0 / lr1 / lr_split without one)."""
        from counting_detr_amd import _ffi
        L, st = _ffi.lib(), _ffi.stream_ptr()
        self._sumsq(L, st)
        tab = None if self.lr is None else self.lr.data_ptr()
        if entry == "step":
            _ffi.check(L.cdetr_adamw_step(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), tab, self.n,
                                          self.sumsq.data_ptr(), self.state.data_ptr(), max_norm, beta1, beta2, eps, wd, grad_div, st),
                       "cdetr_adamw_step")
        else:
            _ffi.check(L.cdetr_adamw_step2(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), tab, self.lr0, self.lr1,
                                           self.split, self.n, self.sumsq.data_ptr(), self.state.data_ptr(), max_norm, beta1, beta2, eps, wd,
                                           grad_div, st), "cdetr_adamw_step2")
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the reference, fp64
def clip_coef64(gq, max_norm):
    """clip_grad_norm_'s coefficient for the (already averaged) gradient gq, and its norm."""
    norm = float(gq.norm())
    return (min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0), norm


def adamw_ref64(p, gr, m, v, lr, s, t, max_norm, wd, grad_div=1.0):
    """clip_grad_norm_(max_norm) + torch.optim.AdamW on fp64 tensors: g' = g grad_div; coef = min(max_norm / (||g'|| + 1e-6), 1);
    p <- p (1 - lr s wd); m <- b1 m + (1 - b1) g' coef; v <- b2 v + (1 - b2) (g' coef)^2;
    p <- p - (lr s / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).  lr: per-element base lr (fp64 tensor), s: the StepLR factor,
    t: the 1-based count of this step.  Returns p, m, v, the norm."""
    gq = gr * grad_div
    coef, norm = clip_coef64(gq, max_norm)
    gc = gq * coef
    l = lr * s
    p = p * (1.0 - l * wd)
    m = BETA1 * m + (1.0 - BETA1) * gc
    v = BETA2 * v + (1.0 - BETA2) * gc * gc
    bc1, bc2 = 1.0 - BETA1 ** t, 1.0 - BETA2 ** t
    p = p - (l / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + EPS))
    return p, m, v, norm


# ------------------------------------------------------------------------------------------------ the yardstick, float32
def adamw_ref32(p, gr, m, v, lr, s, t, max_norm, wd, grad_div=1.0):
    """The same formula in float32 NumPy, in torch's operation order (mul_ / lerp_ / mul_.addcmul_ / sqrt / div / add_ / addcdiv_), every
    intermediate -- the scalars too -- rounded to float32.  beta1, beta2 are float32 values and 1 - beta is formed from them, as any fp32
    implementation that receives the betas as floats must: the float nearest 0.999 is 0.99900001287, so 1 - beta2 is 1.3e-5 (relative)
    off 0.001 and v carries that offset.  Inputs: float32 NumPy arrays (lr: per-element base lr); returns p, m, v, the norm."""
    f = np.float32
    one = f(1.0)
    gq = gr * f(grad_div)
    norm = f(np.sqrt(np.sum(gq * gq, dtype=np.float32)))
    coef = one
    if max_norm > 0:
        coef = f(min(f(f(max_norm) / f(norm + f(1e-6))), one))
    gc = gq * coef
    l = lr * f(s)
    p = p * (one - l * f(wd))
    b1, b2 = f(BETA1), f(BETA2)
    m = m + (gc - m) * f(one - b1)                                   # lerp_(grad, 1 - beta1)
    v = v * b2 + f(one - b2) * gc * gc                               # mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1 = f(one - f(np.power(b1, f(t))))
    bc2 = f(one - f(np.power(b2, f(t))))
    denom = np.sqrt(v) / f(np.sqrt(bc2)) + f(EPS)
    p = p - (l / bc1) * (m / denom)
    for a in (p, m, v):
        assert a.dtype == np.float32
    return p, m, v, float(norm)


def relmax(actual, ref):
    """max |error| over the max |reference| of the tensor (the convention of close() in tests/test_hip_kernels.py)."""
    a, r = np.asarray(actual, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


def bar(yardstick_err):
    """4 x the float32 restatement's own error against fp64 (a few operations ordered differently, powf, 1/sqrtf: a few ulp more, not a
    wrong formula), with a floor of 4 fp32 ulp for a quantity the restatement happens to get exactly."""
    return max(4.0 * yardstick_err, ULP4)


# ------------------------------------------------------------------------------------------------ well-posed inputs
def eps_slices(n, seed):
    """Seeded index sets: elements whose gradient is exactly 0, and elements whose (clipped) gradient has magnitude 1e-9 ... 1e-6, so that
    sqrt(v) / sqrt(bc2) is comparable to eps = 1e-8 and the place eps is added matters."""
    perm = torch.randperm(n, generator=g(seed + 7919))
    k = max(1, n // 16)
    return perm[:k], perm[k:2 * k]


def make_grad(n, seed, scale, max_norm, grad_div, zero_idx, tiny_idx):
    """0.05-ish Gaussian gradient (float32) with the two eps slices; the tiny slice is divided by coef grad_div of the bulk (its own
    contribution to the norm is < 1e-5 of it), so the magnitudes 1e-9 ... 1e-6 are those the moments see."""
    gen = g(seed)
    gr = torch.randn(n, generator=gen) * scale
    gr[zero_idx] = 0.0
    gr[tiny_idx] = 0.0
    coef, _ = clip_coef64(gr.double() * grad_div, max_norm)
    k = tiny_idx.numel()
    mag = 10.0 ** (torch.rand(k, generator=gen, dtype=torch.float64) * 3.0 - 9.0)
    sign = torch.where(torch.rand(k, generator=gen) < 0.5, -1.0, 1.0).double()
    gr[tiny_idx] = (sign * mag / (coef * grad_div)).float()
    return gr


def adam_state(n, seed, t0, lr, s, max_norm, wd, grad_div, zero_idx, tiny_idx, p_scale=0.1, g_scale=0.05, warm=5):
    """A starting state (p, m, v as float32 CPU tensors) that an Adam trajectory produces after t0 steps: the fp64 reference run for
    k = min(t0, warm) steps on fresh gradients from zero moments, then m and v scaled by (1 - beta^t0) / (1 - beta^k), so that the bias
    corrections of step t0 + 1 meet moments of the size they have at that count (k = t0: nothing is scaled).  The step m_hat / sqrt(v_hat)
    is then that of a k-step trajectory: <= sqrt(k) by Cauchy-Schwarz, a few lr at most.  (Independent draws of m and v give steps of
    1000 lr that no trajectory produces.)"""
    p = (torch.randn(n, generator=g(seed)) * p_scale).double()
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    k = min(int(t0), warm)
    for i in range(k):
        gr = make_grad(n, seed + 100 + i, g_scale, max_norm, grad_div, zero_idx, tiny_idx).double()
        p, m, v, _ = adamw_ref64(p, gr, m, v, lr, s, i + 1, max_norm, wd, grad_div)
    if k:
        m = m * ((1.0 - BETA1 ** t0) / (1.0 - BETA1 ** k))
        v = v * ((1.0 - BETA2 ** t0) / (1.0 - BETA2 ** k))
    return p.float(), m.float(), v.float()
