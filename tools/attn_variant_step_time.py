"""Step time of attention_type RCDA vs nn.MultiheadAttention on one MI355X -> one JSON line (profiles/attn_variant_step_time.json).

    python tools/attn_variant_step_time.py [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/attn_variant_step_time.json] [--no-profile]

B=2 800x800 synthetic batch (bench.py's: oracle.step.synthetic_batch seed 0), seeded weights, Q=300 learned anchors.  For each attention
type: the graph-cached training step (Trainer.step) and the graph-replayed inference forward (InferenceEngine); the two types alternate
in one process, `--rounds` times, and the median per round is reported.  Then, unless --no-profile, each type runs again in its OWN child
under `rocprofv3 --kernel-trace --stats` (four stream-ordered training steps, nothing timed): the share of kernel time in the attention kernels (cdetr_mha_* /
cdetr_attn_*: mha.hip), their algorithmic throughput (4 N nh Lq Lk 32 FLOP per forward, 2.5x that per backward: the recomputed scores
and the four gradient products) against the MI355X bf16 MFMA peak (2.5 PF dense), and every kernel
whose name says torch batched GEMM or softmax (there must be none on the nn.MultiheadAttention path).  The kernel-stats CSVs are copied
next to --out.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TYPES = ("RCDA", "nn.MultiheadAttention")
B, H, W, TS = 2, 800, 800, (37, 120)
BF16_PEAK_TF = 2500.0


def _setup(attention_type):
    import torch
    import counting_detr_amd
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import InferenceEngine, Trainer
    from oracle.step import synthetic_batch
    from oracle.weights import model_schema, seeded_state_dict
    from tools.gen_golden_attn_mha import attn_mha_schema
    args = default_args(device="cuda:0")
    args.attention_type = attention_type
    model, crit, _ = counting_detr_amd.build_model(args)
    model.load_state_dict(seeded_state_dict(model_schema() if attention_type == "RCDA" else attn_mha_schema()), strict=True)
    model.to(args.device).train()
    tr = Trainer(model, crit, args, device=args.device)
    images, rects, targets = synthetic_batch(B=B, H=H, W=W, Ts=TS)
    batch = (images.cuda(), rects.cuda(), [{k: v.cuda() for k, v in t.items()} for t in targets])
    # inference on a copy of the model: the engine owns eval mode and its weight images
    imodel, _, _ = counting_detr_amd.build_model(args)
    imodel.load_state_dict(model.state_dict(), strict=True)
    eng = InferenceEngine(imodel.to(args.device))
    torch.cuda.synchronize()
    return tr, eng, batch


def _time(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def measure(steps, warmup, rounds):
    setups = {t: _setup(t) for t in TYPES}
    res = {t: {"train_ms": [], "infer_ms": []} for t in TYPES}
    for _ in range(rounds):
        for t in TYPES:
            tr, eng, (images, rects, targets) = setups[t]
            res[t]["train_ms"].append(_time(lambda: tr.step(images, rects, targets), steps, warmup) * 1e3)
            res[t]["infer_ms"].append(_time(lambda: eng(images, rects), steps, warmup) * 1e3)
    out = {}
    for t in TYPES:
        tr = setups[t][0]
        out[t] = {k: round(statistics.median(v), 3) for k, v in res[t].items()}
        out[t].update({k + "_rounds": [round(x, 3) for x in v] for k, v in res[t].items()})
        out[t]["train_img_s"] = round(B / out[t]["train_ms"] * 1e3, 1)
        out[t]["nonfinite_steps"] = tr.nonfinite_steps()
    return out


def attention_flops(attention_type, enc=6, dec=6, nh=8, Q=300):
    """Algorithmic FLOP of one forward's attention cores (4 N nh Lq Lk 32 each)."""
    hw = (H // 16) * (W // 16)
    f = lambda lq, lk: 4 * B * nh * lq * lk * 32          # noqa: E731
    total = dec * f(Q, Q)                                   # decoder self-attention (both types)
    if attention_type != "RCDA":
        total += enc * f(hw, hw) + dec * f(Q, hw)
    return total


def profile_leg(attention_type, steps):
    import torch
    tr, _, (images, rects, targets) = _setup(attention_type)
    for _ in range(1 + steps):             # stream-ordered steps: exactly one forward and one backward each (kernel_summary divides by 1 + steps)
        tr.train_step(images, rects, targets)
    torch.cuda.synchronize()


def kernel_summary(csv_path, attention_type, steps):
    rows = list(csv.DictReader(open(csv_path)))
    rows = [r for r in rows if "flag_wait_kernel" not in r["Name"] and "delay_kernel" not in r["Name"]]      # sleeping, not working
    ns = lambda r: float(r["TotalDurationNs"])          # noqa: E731
    tot = sum(ns(r) for r in rows)
    fwd = [r for r in rows if re.search(r"flash::fwd|mha_fwd_kernel", r["Name"])]
    bwd = [r for r in rows if re.search(r"flash::bwd|mha_bwd_(q|kv)_kernel", r["Name"])]
    torch_attn = [r["Name"][:100] for r in rows if re.search(r"softmax|bmm|Cijk_|gemm", r["Name"], re.I) and "anonymous namespace" not in r["Name"]]
    calls = 1 + steps                                   # training steps profile_leg ran
    f_fwd = attention_flops(attention_type) * calls
    t_fwd, t_bwd = sum(ns(r) for r in fwd), sum(ns(r) for r in bwd)
    tf = lambda fl, t: round(fl / t / 1e3, 1) if t else None      # noqa: E731   FLOP / ns / 1e3 = TF/s
    top = sorted(rows, key=lambda r: -ns(r))[:10]
    return {"kernel_ms_total": round(tot / 1e6, 3), "attention_share": round((t_fwd + t_bwd) / tot, 4) if tot else None,
            "attn_fwd_ms_per_step": round(t_fwd / 1e6 / calls, 3), "attn_bwd_ms_per_step": round(t_bwd / 1e6 / calls, 3),
            "attn_fwd_tflops": tf(f_fwd, t_fwd), "attn_bwd_tflops": tf(2.5 * f_fwd, t_bwd), "bf16_peak_tflops": BF16_PEAK_TF,
            "torch_gemm_or_softmax_kernels": torch_attn,
            "top": [{"name": r["Name"][:90], "ms": round(ns(r) / 1e6, 3), "calls": int(r["Calls"])} for r in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--leg", default="time", choices=["time", "profile"])
    ap.add_argument("--attention_type", default="nn.MultiheadAttention", choices=TYPES)
    a = ap.parse_args()
    if a.leg == "profile":
        profile_leg(a.attention_type, 3)
        return
    line = {"what": f"B={B} {H}x{W} training step (Trainer.step, graph-cached) and inference (InferenceEngine), seeded weights, Q=300",
            "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "types": measure(a.steps, a.warmup, a.rounds)}
    if not a.no_profile:
        line["profile"] = {}
        for t in TYPES:
            work = tempfile.mkdtemp(prefix="attn_prof_")
            cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "-o", "attn", "--",
                   sys.executable, os.path.abspath(__file__), "--leg", "profile", "--attention_type", t]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            found = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
            if p.returncode == 0 and found:
                line["profile"][t] = kernel_summary(found[0], t, 3)
                if a.out:
                    tag = "rcda" if t == "RCDA" else "mha"
                    shutil.copy(found[0], os.path.splitext(a.out)[0] + f"_{tag}_kernel_stats.csv")
            else:
                line["profile"][t] = {"error": f"rocprofv3 exit {p.returncode}", "tail": (p.stdout + p.stderr)[-800:]}
            shutil.rmtree(work, ignore_errors=True)
            if p.returncode != 0:
                break                      # a failed profiled child ends the profiling legs
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
