"""Case tables, fp64 references and arithmetic floors for the attention kernels at the edges a trained model reaches: near-one-hot
softmax rows, logits above 88 (where exp overflows without the max subtraction), running maxima that jump by more than fp32 exp can
represent, and key-padding masks that fill whole 32-key tiles, cross key 64, start at key 0 or sit on the second image.  No GPU needed;
shared by tests/test_attn_edges_cpu.py, tests/test_rcda_edges_gpu.py and tests/test_mha_edges_gpu.py.

  * RcdaCase / rcda_inputs / rcda_masks: row-column decoupled attention (csrc/rcda.hip).  k and v are multiplied by 1e3 at masked keys:
    finite, so 0 x poison is 0 in the reference too, but a key the kernel fails to mask wrecks the result instead of nudging it.
  * AttnCase / attn_inputs: plain softmax attention (csrc/mha.hip), dense and with per-image lengths.
  * rcda_eval / attn_eval: the closed forms with their hand-written backward passes, in fp64 (the reference) or in the kernel's own
    arithmetic `code` (the emulation):
        0  fp32 tensors throughout;
        1  logits from the three split-bf16 products hi.hi + hi.lo + lo.hi (hi, lo = bf16 roundings), rounded to fp32; the rest in fp64;
        3  code 1 for the forward; each operand of every backward contraction (dO.V^T, dS.K, dS^T.Q, A^T.dO) rounded once to bf16.
  * arithmetic_floor(case, code): max|emulated - fp64| / max|fp64| per output tensor.  bar(existing, floor) = max(existing, 4 x floor): the
    emulation models operand rounding only (not the fp32 accumulation order, not __expf), hence the factor; a bar never comes from a
    kernel's output.
  * RCDA_MUTANTS: wrong mask handlings of the fp64 RCDA reference, to prove that a mask case can tell them from the right one."""
import functools
import math
from dataclasses import dataclass

import torch

NH, E, D = 8, 256, 32
SCALE = D ** -0.5
POISON = 1e3
F64 = None                    # the `code` of the fp64 reference


def g(seed):
    return torch.Generator().manual_seed(seed)


def bf16(t):
    """Round to bf16, keep the dtype."""
    return t.float().bfloat16().to(t.dtype)


def heads(t):
    """[N, L, E] -> [N, nh, L, D]"""
    return t.reshape(t.shape[0], -1, NH, D).permute(0, 2, 1, 3)


def unheads(t):
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], -1, E)


def head_direction():
    """One unit vector per head, the same in every head: the shared direction of the offset cases."""
    return torch.full((E,), 1.0 / math.sqrt(D))


def logits(q, k, code):
    """scale * q k^T per head; q [.., Lq, D], k [.., Lk, D] in fp64 (fp32 for code 0)."""
    if code in (1, 3):
        qh, kh = bf16(q), bf16(k)
        ql, kl = bf16(q - qh), bf16(k - kh)
        kt, klt = kh.transpose(-1, -2), kl.transpose(-1, -2)
        return (qh @ kt + qh @ klt + ql @ kt).float().double() * SCALE
    return (q @ k.transpose(-1, -2)) * SCALE


def rel_err(a, r, floor=1e-30):
    """max|a - r| / max|r|: the metric of every `close` helper of this suite."""
    return (a.double() - r.double()).abs().max().item() / max(r.double().abs().max().item(), floor)


def bar(existing, floor):
    return max(existing, 4.0 * floor)


# ----------------------------------------------------------------------------------------------------- RCDA
def rcda_core_ref(qr, qc, kr, kc, v, mr, mc, nh):
    """fp64 restatement of A2/models/row_column_decoupled_attention.py:215-309 on projected inputs."""
    N, L, E = qr.shape
    H, W = v.shape[1:3]
    d = E // nh
    hs = lambda t: t.reshape(N, -1, nh, d).permute(0, 2, 1, 3)   # noqa: E731
    s_row = (hs(qr) * d ** -0.5) @ hs(kr).transpose(-1, -2)
    s_col = (hs(qc) * d ** -0.5) @ hs(kc).transpose(-1, -2)
    if mr is not None:
        s_row = s_row.masked_fill(mr.bool()[:, None, None, :], float("-inf"))
        s_col = s_col.masked_fill(mc.bool()[:, None, None, :], float("-inf"))
    a_row, a_col = s_row.softmax(-1), s_col.softmax(-1)
    vv = v.reshape(N, H, W, nh, d).permute(0, 3, 1, 2, 4)
    o = torch.einsum("bnqh,bnqw,bnhwc->bnqc", a_col, a_row, vv)
    return o.permute(0, 2, 1, 3).reshape(N, L, E)


@dataclass(frozen=True)
class RcdaCase:
    H: int
    W: int
    L: int
    pattern: str = "pad"          # pad | both | one | holes | bytes
    logit: str = "unit"           # unit | peaked | offset
    keep: tuple = None            # (h, w) valid prefix of image 1 (None: PAD_KEEP[(H, W)])
    N: int = 2

    @property
    def id(self):
        keep = "" if self.keep is None else f"{self.keep[0]}.{self.keep[1]}"
        return f"{self.H}x{self.W}-L{self.L}-{self.pattern}{keep}-{self.logit}"


# valid (h, w) prefix of image 1: inside the first 32-key tile on one axis and one key into the second on the other; past key 64 on H; a
# whole masked tile behind key 96 / only 5 keys of 20; everything from key 96 / 64 on; the last 3 keys of a 100-key axis
PAD_KEEP = {(50, 50): (9, 33), (50, 84): (9, 33), (84, 50): (65, 33), (100, 20): (97, 5), (128, 96): (96, 64), (24, 100): (9, 97),
            (7, 5): (3, 2)}
HOLES = (0, 3, 4, 31, 32, 63, 64, 67, 95)
PEAKED_GAIN = 8.0
RCDA_OFFSET = 100.0


def _rcda_cases():
    every = ("pad", "both", "one", "holes", "bytes")
    out = []
    for (H, W, L), patterns in (((50, 50, 300), ("pad", "one")), ((50, 84, 77), every), ((84, 50, 70), every), ((100, 20, 60), ("pad", "one")),
                                ((128, 96, 40), every), ((24, 100, 33), ("pad", "one")), ((7, 5, 77), ("pad", "one")), ((7, 5, 1), ("pad", "one")),
                                ((50, 50, 2100), ("pad", "one"))):
        out += [RcdaCase(H, W, L, p) for p in patterns]
    out.append(RcdaCase(100, 20, 60, "pad", keep=(5, 19)))
    for H, W, L in ((50, 50, 300), (50, 84, 77), (100, 20, 60), (24, 100, 33)):
        out += [RcdaCase(H, W, L, "pad", "peaked"), RcdaCase(H, W, L, "pad", "offset")]
    return out


RCDA_CASES = _rcda_cases()


def rcda_masks(case):
    """(mask_row [N, W], mask_col [N, H]) uint8, nonzero = masked."""
    N, H, W = case.N, case.H, case.W
    mr, mc = torch.zeros(N, W, dtype=torch.uint8), torch.zeros(N, H, dtype=torch.uint8)
    h, w = case.keep or PAD_KEEP[(H, W)]
    if case.pattern in ("pad", "both", "bytes"):
        mr[1, w:], mc[1, h:] = (255, 2) if case.pattern == "bytes" else (1, 1)
        if case.pattern == "both":
            mr[0, W - 1], mc[0, H - 1] = 1, 1
    elif case.pattern == "one":
        mr[1], mc[1] = 1, 1
        mr[1, (2 * W) // 3], mc[1, H // 2] = 0, 0
    elif case.pattern == "holes":
        for k in HOLES:
            if k < W:
                mr[0, k] = 1
            if k < H:
                mc[0, k] = 1
        mr[1, :W // 2], mc[1, :H // 2] = 1, 1
    else:
        raise ValueError(case.pattern)
    return mr, mc


@functools.lru_cache(maxsize=4)
def rcda_inputs(case):
    """dict of fp32 CPU tensors qr, qc [N,L,E], kr [N,W,E], kc [N,H,E], v [N,H,W,E], go [N,L,E], and uint8 mr [N,W], mc [N,H]."""
    N, L, H, W = case.N, case.L, case.H, case.W
    qr, qc = torch.randn(N, L, E, generator=g(1)), torch.randn(N, L, E, generator=g(2))
    kr, kc = torch.randn(N, W, E, generator=g(3)), torch.randn(N, H, E, generator=g(4))
    v = torch.randn(N, H, W, E, generator=g(5))
    go = torch.randn(N, L, E, generator=g(6))
    if case.logit == "peaked":
        qr, qc = qr * PEAKED_GAIN, qc * PEAKED_GAIN
    elif case.logit == "offset":          # (a u) . (a u) / sqrt(D) = RCDA_OFFSET on every logit
        shift = head_direction() * math.sqrt(RCDA_OFFSET * math.sqrt(D))
        qr, qc, kr, kc = qr + shift, qc + shift, kr + shift, kc + shift
    mr, mc = rcda_masks(case)
    kr[mr.bool()] *= POISON
    kc[mc.bool()] *= POISON
    v = v * torch.where(mc.bool()[:, :, None] | mr.bool()[:, None, :], POISON, 1.0)[..., None]
    return dict(qr=qr, qc=qc, kr=kr, kc=kc, v=v, go=go, mr=mr, mc=mc)


RCDA_OUT = ("out", "dq_row", "dq_col", "dk_row", "dk_col", "dv")


def rcda_eval(inp, code=F64, masks=None, backward=True):
    """The closed form of rcda_core_ref with its backward written out, in fp64 or in arithmetic `code`.  -> dict of out, a_row [N,nh,L,W],
    a_col [N,nh,L,H], s_row, s_col (masked logits) and, with `backward`, dq_row, dq_col, dk_row, dk_col, dv.  `masks`: (mr, mc) in place
    of the inputs' own (the mutants)."""
    dt = torch.float32 if code == 0 else torch.float64
    rnd = bf16 if code == 3 else (lambda t: t)
    mr, mc = masks if masks is not None else (inp["mr"], inp["mc"])
    qr, qc, kr, kc, go = (heads(inp[k].to(dt)) for k in ("qr", "qc", "kr", "kc", "go"))
    N, H, W = inp["v"].shape[:3]
    L = qr.shape[2]
    vv = inp["v"].to(dt).reshape(N, H, W, NH, D).permute(0, 3, 1, 2, 4)            # [N, nh, H, W, D]
    s_row = logits(qr, kr, code).to(dt).masked_fill(mr.bool()[:, None, None, :], -math.inf)
    s_col = logits(qc, kc, code).to(dt).masked_fill(mc.bool()[:, None, None, :], -math.inf)
    a_row, a_col = s_row.softmax(-1), s_col.softmax(-1)
    res = dict(a_row=a_row, a_col=a_col, s_row=s_row, s_col=s_col)
    out = torch.empty(N, NH, L, D, dtype=dt)
    grads = {k: torch.zeros_like(t) for k, t in (("dq_row", qr), ("dq_col", qc), ("dk_row", kr), ("dk_col", kc), ("dv", vv))}
    chunk = max(1, (1 << 23) // (NH * H * W))                                    # queries per pass: the [nh, q, H, W] intermediate stays at 64 MB
    for n in range(N):
        for q0 in range(0, L, chunk):
            q = slice(q0, min(L, q0 + chunk))
            ar, ac = a_row[n, :, q], a_col[n, :, q]
            out[n, :, q] = torch.einsum("nqh,nqhc->nqc", ac, torch.einsum("nqw,nhwc->nqhc", ar, vv[n]))
            if not backward:
                continue
            do = go[n, :, q]
            G = torch.einsum("nqc,nhwc->nqhw", rnd(do), rnd(vv[n]))              # dO . V
            d_ar, d_ac = torch.einsum("nqhw,nqh->nqw", G, ac), torch.einsum("nqhw,nqw->nqh", G, ar)
            ds_r = ar * (d_ar - (ar * d_ar).sum(-1, keepdim=True))
            ds_c = ac * (d_ac - (ac * d_ac).sum(-1, keepdim=True))
            grads["dq_row"][n, :, q] = rnd(ds_r) @ rnd(kr[n]) * SCALE
            grads["dq_col"][n, :, q] = rnd(ds_c) @ rnd(kc[n]) * SCALE
            grads["dk_row"][n] += rnd(ds_r).transpose(-1, -2) @ rnd(qr[n, :, q]) * SCALE
            grads["dk_col"][n] += rnd(ds_c).transpose(-1, -2) @ rnd(qc[n, :, q]) * SCALE
            grads["dv"][n] += torch.einsum("nqh,nqwc->nhwc", rnd(ac), rnd(ar)[..., None] * rnd(do)[:, :, None, :])
    res["out"] = unheads(out)
    if backward:
        for k in ("dq_row", "dq_col", "dk_row", "dk_col"):
            res[k] = unheads(grads[k])
        res["dv"] = grads["dv"].permute(0, 2, 3, 1, 4).reshape(N, H, W, E)
    return res


@functools.lru_cache(maxsize=2)
def rcda_reference(case):
    return rcda_eval(rcda_inputs(case), F64)


def _floors(ref, emu, names):
    return {k: rel_err(emu[k], ref[k]) for k in names}


@functools.lru_cache(maxsize=None)
def _rcda_floor(case, code):
    inp, ref = rcda_inputs(case), rcda_reference(case)
    return _floors(ref, rcda_eval(inp, code), RCDA_OUT)


def rcda_existing_bars(code):
    """The bars of tests/test_hip_kernels.py::test_rcda_core as one number per tensor (its `close` adds rtol and atol_scale, both scaled
    by the reference's largest magnitude): tol(precision) for the output, rtol 5e-4 for the gradients, BF16_BWD_BAR for code 3's."""
    from test_hip_kernels import BF16_BWD_BAR, tol
    t = tol(0 if code == 0 else 1)
    grad = max(5e-4, BF16_BWD_BAR) if code == 3 else 5e-4
    return {k: (t["rtol"] if k == "out" else grad) + t["atol_scale"] for k in RCDA_OUT}


def rcda_bars(case, code):
    """{tensor: (floor, bar)}: bar = max(existing bar, 4 x floor); code 3's output is code 1's (the forward is the same launch)."""
    fl, ex = _rcda_floor(case, code), rcda_existing_bars(code)
    return {k: (fl[k], bar(ex[k], fl[k])) for k in RCDA_OUT}


def _shift(m):
    return torch.cat([m[:, :1], m[:, :-1]], 1)


def _drop_from(key):
    def f(m):
        m = m.clone()
        m[:, key:] = 0
        return m
    return f


def _swap4(m):
    """Keys 8b + j and 8b + (j ^ 4) exchanged: the two lane halves of the matrix-core score phase own offsets 0-3 and 4-7 of every 8 keys
    (the `chunk >> 4g` shift).  Keys whose partner lies past the end stay."""
    n = m.shape[1]
    idx = torch.arange(n) ^ 4
    idx = torch.where(idx < n, idx, torch.arange(n))
    return m[:, idx]


# name -> (mask transform, applicable(number of keys on that axis))
RCDA_MUTANTS = {
    "shifted-by-one": (_shift, lambda n: n > 1),
    "image-0-everywhere": (lambda m: m[:1].expand_as(m).clone(), lambda n: True),
    "bits-from-64-dropped": (_drop_from(64), lambda n: n > 64),
    "bits-from-32-dropped": (_drop_from(32), lambda n: n > 32),
    "lane-halves-swapped": (_swap4, lambda n: n > 4),
}


def rcda_mutants(case):
    """{name: fp64 forward output under the mutated masks} for every mutant that applies to the case's map and changes its masks while
    keeping a valid key on every (image, axis)."""
    inp = rcda_inputs(case)
    out = {}
    for name, (f, ok) in RCDA_MUTANTS.items():
        mr = f(inp["mr"]) if ok(case.W) else inp["mr"]
        mc = f(inp["mc"]) if ok(case.H) else inp["mc"]
        if torch.equal(mr.bool(), inp["mr"].bool()) and torch.equal(mc.bool(), inp["mc"].bool()):
            continue
        if bool(mr.bool().all(1).any()) or bool(mc.bool().all(1).any()):
            continue
        out[name] = rcda_eval(inp, F64, masks=(mr, mc), backward=False)["out"]
    return out


# ----------------------------------------------------------------------------------------------------- plain attention
@dataclass(frozen=True)
class AttnCase:
    Lq: int
    Lk: int
    layout: str                   # separate | packed | lens
    pattern: str                  # peaked | ramp-up | ramp-down | late-half | early-half
    lens: tuple = None
    N: int = 2

    @property
    def id(self):
        tail = "" if self.lens is None else "-" + ".".join(str(x) for x in self.lens)
        return f"{self.Lq}x{self.Lk}-{self.layout}{tail}-{self.pattern}"


ATTN_PATTERNS = ("peaked", "ramp-up", "ramp-down", "late-half", "early-half")
ATTN_OFFSET = 120.0
# The caps of tests/test_attn_edges_cpu.py (4 x floor <= 1e-3 / 5e-2) decide these three, on the CPU, before any kernel runs:
#   * the queries carry ATTN_Q_SHARE times the geometric-mean share of an offset and the keys 1 / ATTN_Q_SHARE of it: dq = dS K with the
#     rows of dS summing to zero, so a large shared component of K only feeds bf16 noise into dq (code-3 floors 1.0-2.1e-2 at equal
#     shares, at most 1.14e-2 at 3; at 4 the code-1 floor of dv passes 2.5e-4);
#   * a 120-logit ramp over 33 keys (3.75 per key) saturates every row and leaves gradients of the size of their bf16 noise (floors
#     2.4e-2 / 4.6e-2): those two ramps end at +60 / +30;
#   * 300 keys at gain 8 give a median row maximum of 0.79: gain 10 from 256 keys on (0.87).
ATTN_Q_SHARE = 3.0
ATTN_OFFSET_LOWERED = {(33, "ramp-up"): 60.0, (33, "ramp-down"): 30.0}
# L = 80: the two-wave kernel (fewer than 128 keys); 160 (five 32-key tiles: uneven halves) and 300: the key-split kernel
ATTN_DENSE = [(80, 80, "separate"), (160, 160, "separate"), (300, 300, "separate"), (31, 80, "separate"), (33, 33, "packed"), (300, 300, "packed")]
ATTN_CASES = [AttnCase(lq, lk, lay, p) for lq, lk, lay in ATTN_DENSE for p in ATTN_PATTERNS]
ATTN_LENS_CASES = [AttnCase(L, L, "lens", p, tuple(lens), N) for N, L, lens in ((3, 130, (64, 65, 130)), (2, 300, (300, 3)))
                   for p in ("peaked", "ramp-up")]


def attn_offset(pattern, Lk):
    return ATTN_OFFSET_LOWERED.get((Lk, pattern), ATTN_OFFSET)


def attn_gain(Lk):
    return PEAKED_GAIN if Lk < 256 else 10.0


def key_offsets(pattern, Lk):
    """The logit offset of every key, [Lk] fp64."""
    j, top = torch.arange(Lk, dtype=torch.float64), attn_offset(pattern, Lk)
    if pattern == "ramp-up":
        return top * j / max(Lk - 1, 1)
    if pattern == "ramp-down":
        return top * (1 - j / max(Lk - 1, 1))
    if pattern == "late-half":
        return top * (j >= Lk // 2)
    if pattern == "early-half":
        return top * (j < Lk // 2)
    raise ValueError(pattern)


@functools.lru_cache(maxsize=4)
def attn_inputs(case):
    """dict of fp32 CPU tensors q [N,Lq,E], k, v [N,Lk,E], go [N,Lq,E] (packed / lens: the test joins q | k).  The offset patterns put
    a_q u on every query and c_j u on key j, u the shared unit direction per head, with the random parts projected off u: the logit of
    (i, j) is the random one plus exactly key_offsets(pattern, Lk)[j] (before the fp32 rounding of the operands)."""
    N, Lq, Lk = case.N, case.Lq, case.Lk
    q, k = torch.randn(N, Lq, E, generator=g(11)), torch.randn(N, Lk, E, generator=g(12))
    v, go = torch.randn(N, Lk, E, generator=g(13)), torch.randn(N, Lq, E, generator=g(14))
    if case.pattern == "peaked":
        q = q * attn_gain(Lk)
    else:
        u = head_direction().double()

        def proj(t):
            th, uh = t.double().reshape(*t.shape[:2], NH, D), u.reshape(NH, D)
            return (th - (th * uh).sum(-1, keepdim=True) * uh).reshape(t.shape)
        a = ATTN_Q_SHARE * math.sqrt(attn_offset(case.pattern, Lk) * math.sqrt(D))
        q = (proj(q) + a * u).float()
        k = (proj(k) + (key_offsets(case.pattern, Lk) * math.sqrt(D) / a)[None, :, None] * u).float()
    return dict(q=q, k=k, v=v, go=go)


ATTN_OUT = ("o", "lse", "dq", "dk", "dv")


def attn_eval(inp, code=F64, lens=None):
    """softmax(q k^T / sqrt(32)) v per head with the backward of the flash kernels (dS = P (dP - rowsum(dO o))), in fp64 or in arithmetic
    `code` -> dict o, lse [N,nh,Lq], p [N,nh,Lq,Lk], dq, dk, dv.  lens (self-attention only): image n's first lens[n] rows attend to each
    other, everything beyond is zero and never read."""
    dt = torch.float32 if code == 0 else torch.float64
    rnd = bf16 if code == 3 else (lambda t: t)
    N, Lq, Lk = inp["q"].shape[0], inp["q"].shape[1], inp["k"].shape[1]
    res = dict(o=torch.zeros(N, Lq, E, dtype=dt), lse=torch.zeros(N, NH, Lq, dtype=dt), p=torch.zeros(N, NH, Lq, Lk, dtype=dt),
               dq=torch.zeros(N, Lq, E, dtype=dt), dk=torch.zeros(N, Lk, E, dtype=dt), dv=torch.zeros(N, Lk, E, dtype=dt))
    for n in range(N):
        lq, lk = (Lq, Lk) if lens is None else (int(lens[n]), int(lens[n]))
        if lq == 0:
            continue
        q, do = (heads(inp[x][n:n + 1, :lq].to(dt)) for x in ("q", "go"))
        k, v = (heads(inp[x][n:n + 1, :lk].to(dt)) for x in ("k", "v"))
        s = logits(q, k, code).to(dt)
        lse = s.logsumexp(-1)
        p = (s - lse[..., None]).exp()
        o = p @ v
        d_p = rnd(do) @ rnd(v).transpose(-1, -2)
        d_s = p * (d_p - (do * o).sum(-1, keepdim=True))
        res["o"][n, :lq], res["lse"][n, :, :lq], res["p"][n, :, :lq, :lk] = unheads(o)[0], lse[0], p[0]
        res["dq"][n, :lq] = unheads(rnd(d_s) @ rnd(k) * SCALE)[0]
        res["dk"][n, :lk] = unheads(rnd(d_s).transpose(-1, -2) @ rnd(q) * SCALE)[0]
        res["dv"][n, :lk] = unheads(rnd(p).transpose(-1, -2) @ rnd(do))[0]
    return res


@functools.lru_cache(maxsize=2)
def attn_reference(case):
    return attn_eval(attn_inputs(case), F64, case.lens)


@functools.lru_cache(maxsize=None)
def _attn_floor(case, code):
    return _floors(attn_reference(case), attn_eval(attn_inputs(case), code, case.lens), ATTN_OUT)


LSE_BAR = 1e-5


def attn_bars(case, code):
    """{tensor: (floor, bar)} from the BARS table of tests/test_attn_kernels_gpu.py; lse: 1e-5 relative, with the floor rule for code 0."""
    from test_attn_kernels_gpu import BARS
    fl = _attn_floor(case, code)
    bo, bg = BARS[code]
    out = {k: (fl[k], bar(bo if k == "o" else bg, fl[k])) for k in ("o", "dq", "dk", "dv")}
    out["lse"] = (fl["lse"], bar(LSE_BAR, fl["lse"]) if code == 0 else LSE_BAR)
    return out


def arithmetic_floor(case, code):
    """{tensor: max|emulated - fp64| / max|fp64|} of an RcdaCase or an AttnCase in arithmetic `code` (0, 1 or 3)."""
    return dict(_rcda_floor(case, code) if isinstance(case, RcdaCase) else _attn_floor(case, code))
