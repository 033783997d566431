"""The transformer glue and normalisation kernels (csrc/elementwise.hip, and the column sum and max-pool of csrc/igemm.hip) against the
plain fp64 restatements of tests/glue_ref.py -- never against another kernel path -- at the sizes where their launch rules change:
one row, fewer rows than a wave batch, the switch of rows per workgroup, every capped grid above its cap, every `nv` of the
LayerNorm chains, empty reduction slices, scalar tails.  Needs an MI355X.

Bars (derived from the arithmetic, not from what the kernels give):
  exact   one correctly rounded fp32 operation per element: torch.equal to the fp64 reference rounded to fp32
  twins   every bf16 twin / plane: torch.equal to bf16_rne of the fp32 output of the same launch
  sum     n fp32 terms summed in an order the kernel chooses: n * 2^-24 * sum|term_i| per element (any order's worst case) plus one
          rounding of the result; nothing relative to the tensor's maximum
  LN      friendly data: the project's `close(rtol=1e-5)`; far-mean data: the larger of that and 4x the error of the fp32 two-pass
          yardstick on the same inputs
  sine    forward 2e-5 absolute, backward `close(rtol=1e-4)` (the bars of test_sine_embed_matches_reference_formula)"""
import itertools

import pytest
import torch
import torch.nn.functional as F

import glue_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def g(seed):
    return torch.Generator().manual_seed(seed)


def randn(seed, *shape):
    return torch.randn(*shape, generator=g(seed))


def dev(t):
    return None if t is None else t.to(DEV)


def close(actual, ref64, rtol=2e-4, atol_scale=2e-5, msg=""):
    """The `close` of tests/test_hip_kernels.py without its backward-arithmetic switch: max error relative to the reference's magnitude."""
    a = actual.detach().double().cpu()
    r = ref64.detach().double().cpu()
    assert a.shape == r.shape, (a.shape, r.shape)
    scale = r.abs().max().item() + 1e-30
    err = (a - r).abs().max().item()
    assert torch.isfinite(a).all(), msg + " non-finite output"
    assert err <= rtol * scale + atol_scale * scale, f"{msg} max err {err:.3e} vs scale {scale:.3e}"


def exact(actual, ref64, msg):
    a, r = actual.detach().cpu(), ref64.to(torch.float32)
    assert a.dtype == torch.float32 and a.shape == r.shape, (msg, a.dtype, a.shape, r.shape)
    if not torch.equal(a, r):
        bad = (a != r).flatten().nonzero().flatten()
        i = bad[0].item()
        raise AssertionError(f"{msg}: {bad.numel()} of {a.numel()} elements differ, first at flat index {i}: {a.flatten()[i].item()!r} vs "
                             f"{r.flatten()[i].item()!r}")


def twin_of(t16, t32, msg):
    a, r = t16.detach().cpu(), ref.bf16_rne(t32.detach().cpu())
    assert a.dtype == torch.bfloat16 and a.shape == r.shape, (msg, a.dtype, a.shape, r.shape)
    assert torch.equal(a.view(torch.int16), r.view(torch.int16)), f"{msg}: the bf16 twin is not the round-to-nearest-even of the fp32 output"


def sum_bound(actual, ref64, abs64, n, msg):
    """|actual - ref| <= n 2^-24 sum|term| + 2^-24 |ref| per element; abs64 = the same reference evaluated on the absolute values."""
    a = actual.detach().double().cpu()
    assert a.shape == ref64.shape, (msg, a.shape, ref64.shape)
    err = (a - ref64).abs()
    bound = n * ref.U * abs64 + ref.U * ref64.abs()
    over = err > bound
    if over.any():
        i = (err - bound).flatten().argmax().item()
        raise AssertionError(f"{msg}: {int(over.sum())} elements beyond the {n}-term bound, worst at flat index {i}: err "
                             f"{err.flatten()[i].item():.3e} vs bound {bound.flatten()[i].item():.3e}")


# ================================================================================================================ LayerNorm
LN_FRIENDLY = [(r, C) for r in (1, 3, 5, 2049) for C in (256, 512, 768, 1024)] + [(8197, 256), (16389, 256)]


def _ln_inputs(rows, C, far=False):
    x = ref.far_mean_input(rows, C, g(1)) if far else randn(1, rows, C) * 2 + 0.5
    return dict(x=x, w=1 + 0.1 * randn(2, C), b=0.1 * randn(3, C), dy=randn(4, rows, C), add=randn(5, rows, C), a1=randn(6, rows, C),
                a2=randn(7, rows, C))


@pytest.mark.parametrize("rows,C", LN_FRIENDLY)
def test_layer_norm_against_fp64(rows, C):
    """ln_fwd_kernel / ln_bwd_kernel on x = 2 randn + 0.5, every entry point, against the fp64 closed forms.
    rows 1, 3: one wave of one workgroup, the other three idle (`row < rows` of the first iteration); 5: a second workgroup with one row, and in
    the C = 256 backward a 4-row batch whose rows 1..3 are clamped and masked (`if (row >= rows) break`); 2049: ln_bwd_blocks switches from 4 to
    32 rows per workgroup, so the C = 256 batches stride by 65 workgroups x 4 and the last one is partly masked; 8197: the forward's cap of
    2048 workgroups binds (its grid-stride loop runs a second time, for 5 rows); 16389: the backward's cap of 512 workgroups binds (`row0 +=
    stride * LN_RB` runs a third time, for 5 rows).  C = 256 takes the `nv == 1` bodies, 512 / 768 / 1024 the `if (i < nv)` chains with
    nv = 2, 3 (the odd one), 4.  dgamma / dbeta are atomically ACCUMULATED: they start at 1.0.  C = 256 also writes the bf16 twin dx16,
    which must be the RNE of dx on every row, tail rows included."""
    from counting_detr_amd import ops
    t = _ln_inputs(rows, C)
    x, w, b, dy, add, a1, a2 = (dev(t[k]) for k in ("x", "w", "b", "dy", "add", "a1", "a2"))
    y64, mean64, rstd64 = ref.layer_norm_fwd(t["x"], t["w"], t["b"], 1e-5)
    y, mean, rstd = ops.ln_fwd_raw(x, w, b, 1e-5)
    close(y, y64, rtol=1e-5, msg="y")
    # the mean is a sum of C fp32 terms in the wave's order, then one division
    x64 = t["x"].double()
    sum_bound(mean, mean64, x64.abs().mean(-1), C, "saved mean")
    assert ((rstd.double().cpu() - rstd64).abs() <= 1e-6 * rstd64).all(), "saved rstd"
    # the fused consumers: same y / mean / rstd bit for bit, o = y + addend in one rounding
    for addends in ((a1, None), (a1, a2)):
        yb, mb, rb, o1, o2 = ops.ln_fwd_add_raw(x, w, b, 1e-5, *addends)
        assert torch.equal(yb, y) and torch.equal(mb, mean) and torch.equal(rb, rstd), "layernorm_fwd_add changes y / mean / rstd"
        exact(o1, yb.double().cpu() + t["a1"].double(), "o1 = y + a1")
        if addends[1] is None:
            assert o2 is None
        else:
            exact(o2, yb.double().cpu() + t["a2"].double(), "o2 = y + a2")
    # backward, fed the statistics the forward saved (as the product does)
    for with_add in (False, True):
        dx64, dg64, db64 = ref.layer_norm_bwd(t["dy"], t["x"], t["w"], 1e-5, add=t["add"] if with_add else None)
        for twin in ((False, True) if C == 256 else (False,)):
            gw, gb = torch.ones(C, device=DEV), torch.ones(C, device=DEV)
            res = ops.ln_bwd_raw(dy, x, mean, rstd, w, gw, gb, add=add if with_add else None, twin=twin)
            dx = res[0] if twin else res
            tag = f"add={with_add} twin={twin}"
            close(dx, dx64, rtol=1e-5, msg="dx " + tag)
            close(gw, 1.0 + dg64, rtol=1e-5, msg="dgamma " + tag)
            close(gb, 1.0 + db64, rtol=1e-5, msg="dbeta " + tag)
            if twin:
                twin_of(res[1], dx, "dx16 " + tag)


@pytest.mark.parametrize("rows,C", [(513, 256), (8197, 256), (513, 768), (513, 1024)])
def test_layer_norm_far_mean(rows, C):
    """x = 100 + 0.5 randn (|mean| / std = 200): a variance formed as E[x^2] - E[x]^2 loses ~5e-3 of y here, the centred second moment of
    ln_fwd_kernel (`a = v.x - mu` before squaring) does not.  The bar per tensor is max(project's bar, 4 x the fp32 two-pass yardstick's
    error); tests/test_glue_ref_cpu.py shows the one-pass form misses it by > 100x.  8197 rows run the capped grid's strided rows on the
    same data; 768 / 1024 the `nv` = 3 / 4 chains.  Measured on an MI355X when the test was written (yardstick / kernel, relative to
    max|reference|; the test prints them):
      513 x 256:   y 8.4e-6 / 4.5e-6   dx 2.4e-6 / 1.2e-6   dgamma 9.0e-6 / 4.8e-6   dbeta 1.6e-7 / 4.3e-7
      8197 x 256:  y 8.1e-6 / 4.8e-6   dx 2.1e-6 / 1.6e-6   dgamma 1.2e-5 / 7.8e-6   dbeta 2.0e-7 / 6.1e-7
      513 x 768:   y 8.5e-6 / 5.9e-6   dx 1.5e-6 / 9.7e-7   dgamma 1.4e-5 / 1.1e-5   dbeta 1.3e-7 / 2.6e-7
      513 x 1024:  y 7.8e-6 / 5.4e-6   dx 9.1e-7 / 7.6e-7   dgamma 7.7e-6 / 7.0e-6   dbeta 1.8e-7 / 3.2e-7"""
    from counting_detr_amd import ops
    t = _ln_inputs(rows, C, far=True)
    x, w, b, dy, add = (dev(t[k]) for k in ("x", "w", "b", "dy", "add"))
    y64, mean64, rstd64 = ref.layer_norm_fwd(t["x"], t["w"], t["b"], 1e-5)
    dx64, dg64, db64 = ref.layer_norm_bwd(t["dy"], t["x"], t["w"], 1e-5, add=t["add"])
    want = dict(y=y64, dx=dx64, dgamma=1.0 + dg64, dbeta=1.0 + db64)
    yard = ref.layer_norm_f32_two_pass(t["x"], t["w"], t["b"], 1e-5, t["dy"], add=t["add"], dgamma0=1.0, dbeta0=1.0)
    y, mean, rstd = ops.ln_fwd_raw(x, w, b, 1e-5)
    gw, gb = torch.ones(C, device=DEV), torch.ones(C, device=DEV)
    dx = ops.ln_bwd_raw(dy, x, mean, rstd, w, gw, gb, add=add)
    got = dict(y=y, dx=dx, dgamma=gw, dbeta=gb)
    assert all(torch.isfinite(v).all() for v in got.values())
    figures, failed = [], []
    for name in ("y", "dx", "dgamma", "dbeta"):
        ye, ke = ref.rel_err(yard[name], want[name]), ref.rel_err(got[name], want[name])
        bar = ref.far_mean_bar(ye)
        figures.append(f"{name}: yardstick {ye:.3e} kernel {ke:.3e} bar {bar:.3e}")
        if not ke <= bar:
            failed.append(name)
    print(f"far-mean rows={rows} C={C}: " + "; ".join(figures))
    assert not failed, f"{failed} beyond the far-mean bar -- " + "; ".join(figures)
    sum_bound(mean, mean64, t["x"].double().abs().mean(-1), C, "saved mean")
    assert ((rstd.double().cpu() - rstd64).abs() <= 1e-6 * rstd64).all(), "saved rstd"


@pytest.mark.parametrize("C", [256, 512, 768, 1024])
def test_layer_norm_constant_rows_are_exact(C):
    """Rows whose elements all equal 0.75: the wave sum C * 0.75 and its division by C are exact, so mean == 0.75, every x - mean == 0,
    y == beta bit for bit and rstd == eps^-1/2 (to rsqrtf's rounding).  A mean taken over the wrong element count (`nv` off by one) or a
    lane that skipped its float4 fails it outright."""
    from counting_detr_amd import ops
    rows = 7
    w, b = 1 + 0.1 * randn(2, C), 0.1 * randn(3, C)
    y, mean, rstd = ops.ln_fwd_raw(torch.full((rows, C), 0.75, device=DEV), dev(w), dev(b), 1e-5)
    assert torch.equal(mean.cpu(), torch.full((rows,), 0.75))
    assert torch.equal(y.cpu(), b.expand(rows, C))
    want = (1e-5) ** -0.5
    assert ((rstd.double().cpu() - want).abs() <= 1e-6 * want).all()


# ========================================================================================================= map-shaped glue
MAP_SHAPES = [(1, 1, 1, 256), (2, 1, 7, 256), (2, 7, 1, 256), (3, 3, 2, 256), (3, 5, 9, 64), (2, 6, 5, 512), (3, 17, 23, 256), (1, 96, 96, 256)]


@pytest.mark.parametrize("N,H,W,C", MAP_SHAPES)
def test_map_glue_against_fp64(N, H, W, C):
    """posadd2, hw_reduce, posadd2_hw_reduce, bcast_add2 and bcast_add2_sum on one map against their fp64 forms.
    (1,1,1,256): one pixel, one float4 per lane; (2,1,7), (2,7,1), (3,3,2) at C = 256: the reduced axis is shorter than the 4 interleaved
    slices of hw_reduce_body's `for (k = sl; k < cnt; k += 4)`, so slices stay empty and still enter `part[sl][c4]`; (3,5,9,64): the
    generic per-channel path; (2,6,5,512): its `cc += 256` loop runs twice; (3,17,23,256): N > 1 and H != W, where `xw = t % W; yh = t % H;
    n = t / H` in the wrong order reads another image's or another row's embedding; (1,96,96,256): 9216 rows x 64 float4 are 2304 workgroups,
    above grid_for's cap of 2048, so posadd2_body / bcast_add2_kernel run their grid-stride loop a second time.  Scales that are not 1/H, 1/W
    (0.3, 1.7) catch a swap of scale_r and scale_c; two different maps without addends and scales 1.0 are the backward's call."""
    from counting_detr_amd import ops
    X, X2, T2, T3 = (randn(s, N, H, W, C) for s in (1, 2, 3, 4))
    Pr, Pc = randn(5, N, W, C), randn(6, N, H, C)
    dX, dX2, dT2, dT3, dPr, dPc = (dev(v) for v in (X, X2, T2, T3, Pr, Pc))
    aX, aX2, aT2, aT3, aPr, aPc = (v.abs() for v in (X, X2, T2, T3, Pr, Pc))

    Qr64, Qc64 = ref.posadd2(X, Pr, Pc)
    Qr, Qc = ops.posadd2(dX, dPr, dPc)
    exact(Qr, Qr64, "posadd2 Qr")
    exact(Qc, Qc64, "posadd2 Qc")

    def reduce_case(Xr, Xc, Ar, Ac, sr, sc, tag):
        Or, Oc = ops.hw_reduce(dev(Xr), dev(Xc), dev(Ar), dev(Ac), sr, sc)
        Or64, Oc64 = ref.hw_reduce(Xr, Xc, Ar, Ac, sr, sc)
        Ora, Oca = ref.hw_reduce(Xr.abs(), Xc.abs(), None if Ar is None else Ar.abs(), None if Ac is None else Ac.abs(), abs(sr), abs(sc))
        extra = 0 if Ar is None else 1
        sum_bound(Or, Or64, Ora, H + extra, f"hw_reduce {tag} Or")
        sum_bound(Oc, Oc64, Oca, W + extra, f"hw_reduce {tag} Oc")
        return Or, Oc
    reduce_case(X, X, Pr, Pc, 1.0 / H, 1.0 / W, "forward")
    reduce_case(X, X2, None, None, 1.0, 1.0, "backward (two maps, no addends)")
    reduce_case(X2, X, Pr, Pc, 0.3, 1.7, "scales 0.3 / 1.7")

    Qr2, Qc2, Kr, Kc = ops.posadd2_hw_reduce(dX, dPr, dPc)
    exact(Qr2, Qr64, "posadd2_hw_reduce Qr")
    exact(Qc2, Qc64, "posadd2_hw_reduce Qc")
    Kr64, Kc64 = ref.hw_reduce(X, X, Pr, Pc, 1.0 / H, 1.0 / W)
    Kra, Kca = ref.hw_reduce(aX, aX, aPr, aPc, 1.0 / H, 1.0 / W)
    sum_bound(Kr, Kr64, Kra, H + 1, "posadd2_hw_reduce Kr")
    sum_bound(Kc, Kc64, Kca, W + 1, "posadd2_hw_reduce Kc")

    for sr, sc in ((1.0, 1.0), (0.3, 1.7)):
        out = ops.bcast_add2(dX, dPr, dPc, sr, sc)
        sum_bound(out, ref.bcast_add2_sum(X, None, None, Pr, Pc, sr, sc), ref.bcast_add2_sum(aX, None, None, aPr, aPc, sr, sc), 3,
                  f"bcast_add2 sr={sr} sc={sc}")
        for n, (u2, u3, d2, d3, b2, b3) in ((3, (None, None, None, None, None, None)), (4, (T2, None, dT2, None, aT2, None)),
                                            (5, (T2, T3, dT2, dT3, aT2, aT3))):
            out = ops.bcast_add2_sum(dX, d2, d3, dPr, dPc, sr, sc)
            sum_bound(out, ref.bcast_add2_sum(X, u2, u3, Pr, Pc, sr, sc), ref.bcast_add2_sum(aX, b2, b3, aPr, aPc, sr, sc), n,
                      f"bcast_add2_sum {n} terms sr={sr} sc={sc}")


# =============================================================================================================== flat glue
FLAT_N = [4, 1028, 4 * 524288 + 1024]


@pytest.mark.parametrize("n", FLAT_N)
def test_add2_and_grad_merge_against_fp64(n):
    """add2_kernel and grad_merge_kernel (float4 per lane).  n = 4: one float4, 255 idle lanes; 1028: a second workgroup with one lane;
    4 * 524288 + 1024: 2049 workgroups' worth, above grid_for's cap of 2048 x 256 float4, so `i += gridDim.x * 256` runs again for the last
    256 float4.  add2 is one rounded add per output (exact), with and without the B / O2 pair.  grad_merge runs every legal combination
    of g2 / acc1 / acc2 (acc2 needs g2): `out` with two terms is exact, with three it has the 3-term sum bound; each accumulator takes
    one rounded add in place (exact), starts non-zero, and an absent one must not be touched through the other's pointer."""
    from counting_detr_amd import ops
    T, A, B, base, g1, g2, c1, c2 = (randn(s, n) for s in range(1, 9))
    dT, dA, dB, dbase, dg1, dg2 = (dev(v) for v in (T, A, B, base, g1, g2))
    o1, o2 = ops.add2(dT, dA)
    assert o2 is None
    exact(o1, ref.add2(T, A)[0], "add2 O1 (no B)")
    o1, o2 = ops.add2(dT, dA, dB)
    r1, r2 = ref.add2(T, A, B)
    exact(o1, r1, "add2 O1")
    exact(o2, r2, "add2 O2")
    for has_g2, has_a1, has_a2 in itertools.product((False, True), repeat=3):
        if has_a2 and not has_g2:
            continue
        tag = f"grad_merge g2={has_g2} acc1={has_a1} acc2={has_a2}"
        a1, a2 = (dev(c1) if has_a1 else None), (dev(c2) if has_a2 else None)
        out = ops.grad_merge(dbase, dg1, dg2 if has_g2 else None, a1, a2)
        out64, n1, n2 = ref.grad_merge(base, g1, g2 if has_g2 else None, c1 if has_a1 else None, c2 if has_a2 else None)
        if has_g2:
            sum_bound(out, out64, base.double().abs() + g1.double().abs() + g2.double().abs(), 3, tag + " out")
        else:
            exact(out, out64, tag + " out")
        if has_a1:
            exact(a1, n1, tag + " acc1")
        if has_a2:
            exact(a2, n2, tag + " acc2")


# ================================================================================================================ ReLU mask
RELU_SPECIALS = [0.0, -0.0, float("nan"), -2.0, -1e-30]


def _relu_y(n, rot):
    """randn with zeros of both signs, a NaN and negatives at known places: the first five elements, five in the middle and the last five
    (the scalar tail).  -> y, the indices that must give 0."""
    y = randn(1, n)
    if rot is None:
        return y, (y <= 0).nonzero().flatten()
    idx = sorted(set(range(min(n, 5))) | set(range(max(n - 5, 0), n)) | (set(range(n // 2, n // 2 + 5)) if n > 20 else set()))
    for i in idx:
        y[i] = RELU_SPECIALS[(i + rot) % 5]
    return y, torch.tensor(idx)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 4 * 524288 + 7])
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0], ids=["1", "half", "third"])
def test_relu_mask_against_fp64(n, scale):
    """relu_mask_kernel through cdetr_relu_mask and cdetr_relu_mask2 (bf16 twin).  n = 1, 3: `n4 == 0`, only block 0's scalar tail runs;
    4: the float4 body alone; 5 and 1027: the tail after the body (`i = (n4 << 2) + threadIdx.x`); 4 * 524288 + 7: 2049 workgroups' worth of
    float4, above grid_for's cap, plus a 3-element tail.  `a.x > 0.f` must be false for +0.0, -0.0, NaN and negatives: those positions
    give exactly 0 whatever dy holds.  Elsewhere dz is ONE rounded product: bit-exact for every scale (1 and 0.5 are exact products, 1/3 is
    the fp64 product of dy and the fp32 scale rounded once).  The twin is the RNE of dz in the body (packed conversion) and in the tail
    (`(__bf16)v`) alike."""
    from counting_detr_amd import ops
    dy = randn(2, n) * 3
    for rot in (list(range(5)) if n <= 5 else [0]) + [None]:
        y, zeros = _relu_y(n, rot)
        dz64 = ref.relu_mask(y, dy, scale)
        assert (dz64[zeros] == 0).all()
        dz = ops.relu_mask(dev(y), dev(dy), scale)
        dz2, dz16 = ops.relu_mask(dev(y), dev(dy), scale, twin=True)
        for name, t in (("relu_mask", dz), ("relu_mask2", dz2)):
            exact(t, dz64, f"{name} rot={rot}")
            assert (t.cpu()[zeros] == 0).all(), f"{name} rot={rot}: y <= 0 / NaN must give 0"
        twin_of(dz16, dz2, f"relu_mask2 dz16 rot={rot}")


# =============================================================================================================== column sum
@pytest.mark.parametrize("pad", [0, 3], ids=["ldx=N", "ldx=N+3"])
def test_colsum_against_fp64(pad):
    """colsum_kernel: out[n] += sum_m X[m][n], rows in slices of 64 (one workgroup row each, atomically added), eight rows per batch of loads.
    M = 1, 7: the remainder loop alone; 8: one batch, no remainder; 9, 63: batches + remainder; 64: one full slice; 65, 129: a second /
    third slice holding one row (`r1 = min(M, r0 + 64)`).  N = 1, 255: `n >= N` masks lanes; 256: one full workgroup; 257: a second
    workgroup column with one lane.  ldx = N + 3: X2d is a column slice of a wider tensor, rows are `ldx` apart, not N.  `out` starts
    non-zero: the kernel accumulates.  M + 1 terms in an order the kernel chooses: the sum bound."""
    from counting_detr_amd import ops
    for M, N in itertools.product((1, 7, 8, 9, 63, 64, 65, 129), (1, 255, 256, 257)):
        wide = randn(M * 1000 + N, M, N + pad)
        out0 = randn(N, N)
        dwide = dev(wide)
        X, dX = (wide[:, 2:N + 2], dwide[:, 2:N + 2]) if pad else (wide, dwide)
        assert dX.stride(0) == N + pad
        out = dev(out0)
        ops.colsum_(dX, out)
        sum_bound(out, ref.colsum(X, out0), ref.colsum(X.abs(), out0.abs()), M + 1, f"colsum M={M} N={N} ldx={N + pad}")


# ========================================================================================================== sine embedding
T_SINE = 10000.0


def _sine_fwd(pos_ptr, pstride, out_ptr, ldo, rows, nfeat):
    from counting_detr_amd import _ffi
    _ffi.check(_ffi.lib().cdetr_sine_embed(pos_ptr, pstride, out_ptr, ldo, rows, nfeat, T_SINE, _ffi.stream_ptr()), "cdetr_sine_embed")


def _sine_bwd(pos_ptr, pstride, dout_ptr, ldo, dpos_ptr, dstride, rows, nfeat, accumulate):
    from counting_detr_amd import _ffi
    _ffi.check(_ffi.lib().cdetr_sine_embed_bwd(pos_ptr, pstride, dout_ptr, ldo, dpos_ptr, dstride, rows, nfeat, T_SINE, accumulate,
                                               _ffi.stream_ptr()), "cdetr_sine_embed_bwd")


@pytest.mark.parametrize("nfeat", [2, 64, 128, 256])
@pytest.mark.parametrize("rows", [1, 5, 2100])
def test_sine_embed_against_fp64(rows, nfeat):
    """sine_embed_kernel / sine_embed_bwd_kernel through the C entry points (the wrapper hides pstride, ldo, dstride and accumulate).
    nfeat = 2: one frequency pair, 62 idle lanes in the backward's `for (i = lane; i < nfeat; i += 64)`; 64: one pass; 128, 256: two / four.
    rows = 1, 5: partial workgroups (`r >= rows` returns in the backward); 2100 x 256 features are 2100 workgroups' worth, above the forward's
    cap of 2048, so `idx += gridDim.x * 256` runs again.  Positions lie in [0, 1] and include 0.0 and 1.0.  pstride = 2 reads each
    coordinate of a [rows, 2] tensor in place; ldo = 2 nfeat writes into the second half of a wider buffer whose first half must stay as it
    was; the backward with accumulate = 0 must overwrite a NaN-filled slot, with accumulate = 1 add to what the slot holds, and dstride = 2
    must leave the other coordinate's slot alone."""
    pos = torch.rand(rows, 2, generator=g(1))
    pos[0, 0], pos[-1, 1], pos[-1, 0], pos[0, 1] = 0.0, 1.0, (0.0 if rows == 1 else 1.0), (1.0 if rows == 1 else 0.0)
    dout = randn(2, rows, 2 * nfeat)
    dpos0 = randn(3, rows, 2)
    pos_d, dout_d = dev(pos), dev(dout)
    # ---- forward: contiguous one-coordinate form
    p0 = dev(pos[:, 0].contiguous())
    out = torch.empty(rows, nfeat, device=DEV)
    _sine_fwd(p0.data_ptr(), 1, out.data_ptr(), nfeat, rows, nfeat)
    e64 = [ref.sine_embed(pos[:, c], nfeat, T_SINE) for c in (0, 1)]
    assert (out.double().cpu() - e64[0]).abs().max().item() <= 2e-5, "sine_embed pstride=1"
    # ---- forward: both coordinates in place (pstride = 2), coordinate 1 into the second half of a wider buffer (ldo = 2 nfeat)
    wide = torch.full((rows, 2 * nfeat), 7.0, device=DEV)
    _sine_fwd(pos_d.data_ptr() + 4, 2, wide.data_ptr() + 4 * nfeat, 2 * nfeat, rows, nfeat)
    assert torch.equal(wide[:, :nfeat].cpu(), torch.full((rows, nfeat), 7.0)), "sine_embed with ldo > nfeat wrote outside its half"
    assert (wide[:, nfeat:].double().cpu() - e64[1]).abs().max().item() <= 2e-5, "sine_embed pstride=2 ldo=2 nfeat (coordinate 1)"
    _sine_fwd(pos_d.data_ptr(), 2, wide.data_ptr(), 2 * nfeat, rows, nfeat)
    assert (wide[:, :nfeat].double().cpu() - e64[0]).abs().max().item() <= 2e-5, "sine_embed pstride=2 (coordinate 0)"
    assert (wide[:, nfeat:].double().cpu() - e64[1]).abs().max().item() <= 2e-5, "sine_embed: the second half changed"
    # ---- backward: dout's halves belong to coordinates 0 / 1 (ldo = 2 nfeat), gradients land in the two slots of a [rows, 2] tensor
    d64 = [ref.sine_embed_bwd(pos[:, c], dout[:, c * nfeat:(c + 1) * nfeat], nfeat, T_SINE) for c in (0, 1)]
    dp = torch.full((rows, 2), float("nan"), device=DEV)
    _sine_bwd(pos_d.data_ptr(), 2, dout_d.data_ptr(), 2 * nfeat, dp.data_ptr(), 2, rows, nfeat, 0)
    assert torch.isnan(dp[:, 1]).all(), "sine_embed_bwd dstride=2 touched the other coordinate's slot"
    close(dp[:, 0], d64[0], rtol=1e-4, msg="dpos coordinate 0, accumulate=0")
    _sine_bwd(pos_d.data_ptr() + 4, 2, dout_d.data_ptr() + 4 * nfeat, 2 * nfeat, dp.data_ptr() + 4, 2, rows, nfeat, 0)
    close(dp[:, 1], d64[1], rtol=1e-4, msg="dpos coordinate 1, accumulate=0")
    close(dp[:, 0], d64[0], rtol=1e-4, msg="dpos coordinate 0 after coordinate 1 was written")
    # accumulate = 1 into known values: slot + gradient, the other slot bit for bit what it was
    dp = dev(dpos0)
    _sine_bwd(pos_d.data_ptr() + 4, 2, dout_d.data_ptr() + 4 * nfeat, 2 * nfeat, dp.data_ptr() + 4, 2, rows, nfeat, 1)
    assert torch.equal(dp[:, 0].cpu(), dpos0[:, 0]), "sine_embed_bwd accumulate=1 dstride=2 touched the other coordinate's slot"
    close(dp[:, 1], dpos0[:, 1].double() + d64[1], rtol=1e-4, msg="dpos coordinate 1, accumulate=1")
    # contiguous form (pstride = dstride = 1, ldo = nfeat), accumulate = 1
    dc = dev(dout[:, :nfeat].contiguous())
    dp1 = dev(dpos0[:, 0].contiguous())
    _sine_bwd(p0.data_ptr(), 1, dc.data_ptr(), nfeat, dp1.data_ptr(), 1, rows, nfeat, 1)
    close(dp1, dpos0[:, 0].double() + d64[0], rtol=1e-4, msg="dpos contiguous, accumulate=1")


# ================================================================================================================= max-pool
def _pool_check(x, tag):
    from counting_detr_amd import ops
    N, H, W, C = x.shape
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1) if x.numel() > 1 << 20 else ref.maxpool3x3s2(x)
    dx = dev(x)
    y = ops.maxpool3x3s2(dx)
    exact(y, want.double(), f"maxpool {tag}")
    ys, hi, lo = ops.maxpool3x3s2(dx, split=True)
    assert torch.equal(ys, y), f"maxpool split=True {tag}: y differs from the plain form"
    yc = ys.cpu()
    whi, wlo = ref.split_planes(yc)
    assert torch.equal(hi.cpu().view(torch.int16), whi.view(torch.int16)), f"maxpool {tag}: hi plane is not bf16_rne(y)"
    assert torch.equal(lo.cpu().view(torch.int16), wlo.view(torch.int16)), f"maxpool {tag}: lo plane is not bf16_rne(y - hi)"


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (1, 5), (6, 4), (37, 41), (5, 8)])
def test_maxpool_against_reference(H, W):
    """maxpool_kernel, plain and split=True.  (1,1): every tap but the centre is padding (`iy < 0 || iy >= H` on both sides at once);
    (2,2), (6,4): even sizes, the last window ends inside the map; (1,5), (5,8): odd x even, the last window's right / bottom tap is
    padding; (37,41): several workgroups and `ox = t % Wo; oy = t % Ho` with Ho != Wo.  C = 4 is one float4 per pixel, 64 sixteen; N = 3
    checks the image stride.  Inputs: randn, and -|randn| - 1, where a zero pad in place of -inf would win every border window.  The
    maximum of fp32 values is exact; the planes are bf16_rne(y) and bf16_rne(y - hi)."""
    for C, N, negative in itertools.product((4, 64), (1, 3), (False, True)):
        x = randn(H * 100 + W + C + N, N, H, W, C)
        _pool_check(-x.abs() - 1 if negative else x, f"N={N} H={H} W={W} C={C} negative={negative}")


def test_maxpool_past_the_grid_cap():
    """(1, 736, 736, 64) pools to 368 x 368 x 16 float4 = 2.17 M outputs = 8464 workgroups' worth, above maxpool's cap of 8192: the
    grid-stride loop `idx += gridDim.x * 256` runs a second time for the last 272 workgroups' worth.  The reference is one F.max_pool2d."""
    _pool_check(randn(1, 1, 736, 736, 64), "736 x 736 x 64")
