"""Kernel times of cdetr_attn_fwd / cdetr_attn_bwd at the nn.MultiheadAttention variant's sizes (N=2, nh=8) -> one JSON line.

    CDETR_ATTN_BWD_TWO_LAUNCHES=0|1 python tools/attn_ab.py

The switch is read once per process (csrc/mha.hip): run once per setting to compare the backward's one launch against two.  Times are medians over 50 launches between events, after 5 warm-up launches.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(300, 864), (300, 2500), (900, 2500), (2500, 2500), (4200, 4200)]


def med_ms(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    from counting_detr_amd import ops
    N, nh, E = 2, 8, 256
    g = torch.Generator().manual_seed(0)
    res = {"bwd_two_launches": os.environ.get("CDETR_ATTN_BWD_TWO_LAUNCHES", "0")}
    for Lq, Lk in SHAPES:
        q = torch.randn(N, Lq, E, generator=g).cuda().requires_grad_(True)
        k = torch.randn(N, Lk, E, generator=g).cuda().requires_grad_(True)
        v = torch.randn(N, Lk, E, generator=g).cuda().requires_grad_(True)
        go = torch.randn(N, Lq, E, generator=g).cuda()
        fl = 4 * N * nh * Lq * Lk * 32
        t_f = med_ms(lambda: ops.attn_core(q, k, v, nh))
        o = ops.attn_core(q, k, v, nh)
        t_b = med_ms(lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True))
        res[f"{Lq}x{Lk}"] = {"fwd_ms": round(t_f, 4), "bwd_ms": round(t_b, 4), "fwd_tflops": round(fl / t_f / 1e9, 1),
                             "bwd_tflops": round(2.5 * fl / t_b / 1e9, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
