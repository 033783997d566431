"""cdetr_attn_fwd / cdetr_attn_bwd (through ops.attn_core) against fp64 torch attention, for query / key lengths from 1 to 4200, packed
(q | k halves of one [N,L,2E] tensor) and separate strided operands, in the three arithmetic codes -- and bitwise against cdetr_mha_* at
the decoder self-attention's sizes.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NH, E = 8, 256
SHAPES = [(1, 33), (31, 80), (300, 864), (900, 2500), (2500, 2500), (4200, 4200)]


def g(seed):
    return torch.Generator().manual_seed(seed)


def close(actual, ref, rtol, msg, floor=1e-30):
    """Error relative to the reference's largest magnitude (the style of tests/test_hip_kernels.py's `close`); `floor`: the scale when the
    exact result vanishes (one key: dq = dk = 0 exactly, the kernels leave the rounding of dO.v - dO.o)."""
    a, r = actual.detach().double(), ref.detach().double().to(actual.device)
    assert a.shape == r.shape, (a.shape, r.shape)
    assert torch.isfinite(a).all(), msg + " non-finite"
    scale = max(r.abs().max().item(), floor)
    err = (a - r).abs().max().item()
    assert err <= rtol * scale, f"{msg}: max err {err:.3e} vs scale {scale:.3e}"


def reference(q, k, v, go):
    """fp64 softmax(q k^T / sqrt(32)) v per head, with its gradients."""
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    N, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    hs = lambda t, L: t.reshape(N, L, NH, 32).permute(0, 2, 1, 3)      # noqa: E731
    a = ((hs(q64, Lq) * 32 ** -0.5) @ hs(k64, Lk).transpose(-1, -2)).softmax(-1)
    o = (a @ hs(v64, Lk)).permute(0, 2, 1, 3).reshape(N, Lq, E)
    o.backward(go.double())
    return o.detach(), q64.grad, k64.grad, v64.grad


def run(precision, bwd, Lq, Lk, packed, N=2, seed=0):
    """(o, dq, dk, dv) of ops.attn_core in the given arithmetic, and the fp64 reference's."""
    from counting_detr_amd import ops
    if packed:
        qk = torch.randn(N, Lq, 2 * E, generator=g(seed)).to(DEV).requires_grad_(True)
        q, k = qk[..., :E], qk[..., E:]
    else:                   # separate operands, each a column slice of a wider tensor: row strides E + 64, image strides L * (E + 64)
        qw = torch.randn(N, Lq, E + 64, generator=g(seed)).to(DEV).requires_grad_(True)
        kw = torch.randn(N, Lk, E + 64, generator=g(seed + 1)).to(DEV).requires_grad_(True)
        q, k = qw[..., 32:32 + E], kw[..., 32:32 + E]
    v = torch.randn(N, Lk, E, generator=g(seed + 2)).to(DEV).requires_grad_(True)
    go = torch.randn(N, Lq, E, generator=g(seed + 3)).to(DEV)
    old = (ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16)
    ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = precision, 3, bwd == 3
    try:
        o = ops.attn_core(qk, None, v, NH) if packed else ops.attn_core(q, k, v, NH)
        o.backward(go)
    finally:
        ops.PRECISION, ops.PRECISION_BWD, ops.MHA_BWD_BF16 = old
    if packed:
        dq, dk = qk.grad[..., :E], qk.grad[..., E:]
    else:
        dq, dk = qw.grad[..., 32:32 + E], kw.grad[..., 32:32 + E]
        assert float(qw.grad[..., :32].abs().max()) == 0.0 and float(kw.grad[..., 32 + E:].abs().max()) == 0.0
    return (o, dq, dk, v.grad), reference(q, k, v, go)


# (forward precision, backward precision code): 0 = fp32 VALU; 1 = split-bf16 x3; 3 = split-bf16 scores + plain-bf16 gradient contractions
MODES = [(0, 0), (1, 1), (1, 3)]
BARS = {0: (2e-5, 1e-4), 1: (2e-5, 1e-4), 3: (2e-5, 1.5e-2)}      # (output, gradients): tests/test_hip_kernels.py::test_mha_core's bars


# the packed q | k layout is a self-attention: only the square shapes
LAYOUTS = [(lq, lk, False) for lq, lk in SHAPES] + [(lq, lk, True) for lq, lk in SHAPES if lq == lk]


@pytest.mark.parametrize("mode", MODES, ids=["fp32", "bf16x3", "bf16-bwd"])
@pytest.mark.parametrize("Lq,Lk,packed", LAYOUTS, ids=[f"{lq}x{lk}-{'packed' if p else 'separate'}" for lq, lk, p in LAYOUTS])
def test_attn_core_vs_fp64(Lq, Lk, packed, mode):
    ours, ref = run(mode[0], mode[1], Lq, Lk, packed)
    bo, bg = BARS[mode[1]]
    close(ours[0], ref[0], bo, "o")
    for name, a, r in zip(("dq", "dk", "dv"), ours[1:], ref[1:]):
        close(a, r, bg, name)


def test_packed_self_attention_lengths_without_a_square_case():
    """Rows past L inside the last 32- and 64-row tiles: self-attention at lengths that are not tile multiples, packed layout."""
    for L in (1, 31, 33, 80):
        ours, ref = run(1, 1, L, L, True, N=2, seed=L)
        close(ours[0], ref[0], 2e-5, f"o L={L}")
        for name, a, r in zip(("dq", "dk", "dv"), ours[1:], ref[1:]):
            close(a, r, 1e-4, f"{name} L={L}", floor=1.0)          # unit-variance operands: gradients of O(1)


@pytest.mark.parametrize("L", [300, 900])
@pytest.mark.parametrize("precision,bwd", [(0, 0), (1, 1), (1, 3)], ids=["fp32", "bf16x3", "bf16-bwd"])
def test_attn_equals_mha_bitwise(L, precision, bwd):
    """cdetr_attn_* on q = qk[..., :E], k = qk[..., E:] is cdetr_mha_* bit for bit (same kernels, same arithmetic)."""
    from counting_detr_amd import _ffi, ops
    N = 2
    qk = torch.randn(N, L, 2 * E, generator=g(7)).to(DEV)
    v = torch.randn(N, L, E, generator=g(8)).to(DEV)
    go = torch.randn(N, L, E, generator=g(9)).to(DEV)
    old = ops.PRECISION
    ops.PRECISION = precision
    try:
        o_m, lse_m = ops.mha_fwd_raw(qk, v, NH)
    finally:
        ops.PRECISION = old
    L_ = _ffi.lib()
    d_qk, d_v, work = torch.empty_like(qk), torch.empty_like(v), torch.empty(N, NH, L, device=DEV)
    _ffi.check(L_.cdetr_mha_bwd(qk.data_ptr(), v.data_ptr(), o_m.data_ptr(), go.data_ptr(), lse_m.data_ptr(), d_qk.data_ptr(),
                                d_v.data_ptr(), work.data_ptr(), N, L, NH, 32 ** -0.5, bwd, _ffi.stream_ptr()), "cdetr_mha_bwd")
    # the same problem through cdetr_attn_* with q and k as strided views
    import ctypes
    d = ops._attn_desc(qk.data_ptr(), 2 * E, qk.data_ptr() + 4 * E, 2 * E, v.data_ptr(), E, N, L, L, NH, precision)
    o_a, lse_a = torch.empty_like(o_m), torch.empty_like(lse_m)
    d.o, d.lse = o_a.data_ptr(), lse_a.data_ptr()
    _ffi.check(L_.cdetr_attn_fwd(ctypes.byref(d), _ffi.stream_ptr()), "cdetr_attn_fwd")
    dq, dk, dv2, work2 = torch.empty(N, L, E, device=DEV), torch.empty(N, L, E, device=DEV), torch.empty_like(v), torch.empty_like(work)
    d = ops._attn_desc(qk.data_ptr(), 2 * E, qk.data_ptr() + 4 * E, 2 * E, v.data_ptr(), E, N, L, L, NH, bwd)
    d.o, d.lse, d.d_o, d.d_q, d.d_k, d.d_v, d.work = o_m.data_ptr(), lse_m.data_ptr(), go.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv2.data_ptr(), work2.data_ptr()
    d.ld_dq, d.ld_dk, d.ld_dv = E, E, E
    _ffi.check(L_.cdetr_attn_bwd(ctypes.byref(d), _ffi.stream_ptr()), "cdetr_attn_bwd")
    torch.cuda.synchronize()
    assert torch.equal(o_a, o_m) and torch.equal(lse_a, lse_m)
    assert torch.equal(dq, d_qk[..., :E]) and torch.equal(dk, d_qk[..., E:]) and torch.equal(dv2, d_v)


@pytest.mark.parametrize("Lq,Lk", [(300, 864), (2500, 2500)])
def test_repeated_launches_are_bit_identical(Lq, Lk):
    a, _ = run(1, 3, Lq, Lk, False, seed=3)
    b, _ = run(1, 3, Lq, Lk, False, seed=3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_bwd_one_launch_equals_two_launches(monkeypatch):
    """The backward's one-launch grid (as wide as the longer side, surplus workgroups exit) computes what two exactly sized launches do:
    the A/B switch CDETR_ATTN_BWD_TWO_LAUNCHES is read once per process, so the comparison runs in a child."""
    import subprocess
    import sys
    code = ("import sys, torch; sys.path.insert(0, 'tests'); import test_attn_kernels_gpu as T\n"
            "out = [t.cpu() for t in T.run(1, 3, 900, 2500, False, seed=5)[0]]\n"
            "torch.save(out, sys.argv[1])\n")
    import os
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    with tempfile.TemporaryDirectory() as td:
        for two in ("0", "1"):
            path = os.path.join(td, f"o{two}.pt")
            env = dict(os.environ, CDETR_ATTN_BWD_TWO_LAUNCHES=two)
            subprocess.run([sys.executable, "-c", code, path], cwd=root, env=env, check=True, timeout=300)
            res.append(torch.load(path))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert np.isfinite(res[0][0].detach().numpy()).all()
