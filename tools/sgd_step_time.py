"""Training step and optimizer-update time of AdamW vs --sgd on one MI355X -> one JSON line (profiles/sgd_step_time.json).

    python tools/sgd_step_time.py [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/sgd_step_time.json] [--no-profile]

bench.py's configuration: B=2 800x800 synthetic batch (oracle.step.synthetic_batch seed 0), Q=300 learned anchors, T=(37,120), seeded
weights, the graph-cached step (Trainer.step: captured once, then the chain replayed).  The two optimizers' trainers live in one process
and alternate, `--rounds` times; the median per round is reported.  Then, unless --no-profile, each optimizer runs again in its OWN
child under `rocprofv3 --kernel-trace --stats` (four stream-ordered steps, nothing timed): the update kernels' time per step
(adamw_kernel / sgd_kernel, adamw_finish_kernel, sumsq) and the update kernel's achieved HBM rate against the 8 TB/s peak, from the bytes
the update must move per trainable parameter: AdamW reads p, g, m, v and writes p, m, v (28 B); SGD reads p, g, buf and writes p, buf
(20 B).  The kernel-stats CSVs are copied next to --out.  Each child runs under its own time limit.
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

OPTS = ("AdamW", "SGD")
B, H, W, TS = 2, 800, 800, (37, 120)
HBM_PEAK_TBS = 8.0
BYTES_PER_PARAM = {"AdamW": 28, "SGD": 20}


def _setup(opt):
    import torch
    import counting_detr_amd
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import Trainer
    from oracle.step import synthetic_batch
    from oracle.weights import model_schema, seeded_state_dict
    args = default_args(device="cuda:0", sgd=(opt == "SGD"))
    model, crit, _ = counting_detr_amd.build_model(args)
    model.load_state_dict(seeded_state_dict(model_schema()), strict=True)
    model.to(args.device).train()
    tr = Trainer(model, crit, args, device=args.device)
    assert tr.optimizer_name == opt
    images, rects, targets = synthetic_batch(B=B, H=H, W=W, Ts=TS)
    batch = (images.cuda(), rects.cuda(), [{k: v.cuda() for k, v in t.items()} for t in targets])
    torch.cuda.synchronize()
    return tr, batch


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
    setups = {o: _setup(o) for o in OPTS}
    res = {o: [] for o in OPTS}
    for _ in range(rounds):
        for o in OPTS:
            tr, (images, rects, targets) = setups[o]
            res[o].append(_time(lambda: tr.step(images, rects, targets), steps, warmup) * 1e3)
    out = {}
    for o in OPTS:
        tr = setups[o][0]
        assert tr.cache_stats["captures"] == 1, tr.cache_stats
        out[o] = {"step_ms": round(statistics.median(res[o]), 3), "step_ms_rounds": [round(x, 3) for x in res[o]],
                  "train_img_s": round(B / statistics.median(res[o]) * 1e3, 1), "nonfinite_steps": tr.nonfinite_steps(),
                  "trainable_params": tr.flat_p.numel()}
    out["sgd_minus_adamw_ms"] = round(out["SGD"]["step_ms"] - out["AdamW"]["step_ms"], 3)
    return out


def profile_leg(opt, steps):
    import torch
    tr, (images, rects, targets) = _setup(opt)
    for _ in range(1 + steps):             # stream-ordered steps: exactly one update each (kernel_summary divides by 1 + steps)
        tr.train_step(images, rects, targets)
    torch.cuda.synchronize()
    print(json.dumps({"trainable_params": tr.flat_p.numel()}))


def kernel_summary(csv_path, opt, steps, n_params):
    rows = list(csv.DictReader(open(csv_path)))
    ns = lambda r: float(r["TotalDurationNs"])          # noqa: E731
    calls = 1 + steps

    def pick(pat):
        sel = [r for r in rows if re.search(pat, r["Name"])]
        return sum(ns(r) for r in sel), sum(int(r["Calls"]) for r in sel)
    upd_ns, upd_calls = pick(r"::(adamw|sgd)_kernel\(")
    fin_ns, _ = pick(r"::adamw_finish_kernel\(")
    sq_ns, _ = pick(r"::sumsq(_final)?_kernel\(")
    assert upd_calls == calls, (upd_calls, calls)
    nbytes = BYTES_PER_PARAM[opt] * n_params
    upd_us = upd_ns / calls / 1e3
    return {"update_kernel_us": round(upd_us, 1), "finish_kernel_us": round(fin_ns / calls / 1e3, 2), "sumsq_us": round(sq_ns / calls / 1e3, 1),
            "update_bytes": nbytes, "update_tb_s": round(nbytes / (upd_us * 1e-6) / 1e12, 2),
            "update_share_of_peak": round(nbytes / (upd_us * 1e-6) / 1e12 / HBM_PEAK_TBS, 3),
            "calls": calls, "kernel_ms_total_per_step": round(sum(ns(r) for r in rows) / calls / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--leg", default="time", choices=["time", "profile"])
    ap.add_argument("--opt", default="SGD", choices=OPTS)
    a = ap.parse_args()
    if a.leg == "profile":
        profile_leg(a.opt, 3)
        return
    line = {"what": "stage-2 training step, AdamW vs --sgd (graph-cached step, chain replayed), seeded weights",
            "config": {"B": B, "H": H, "W": W, "Q": 300, "targets": list(TS)}, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
            "time": measure(a.steps, a.warmup, a.rounds)}
    if not a.no_profile:
        line["profile"] = {}
        for o in OPTS:
            work = tempfile.mkdtemp(prefix="sgd_prof_")
            cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "-o", o.lower(), "--",
                   sys.executable, os.path.abspath(__file__), "--leg", "profile", "--opt", o]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            found = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
            n = [json.loads(x)["trainable_params"] for x in p.stdout.splitlines() if x.startswith("{\"trainable_params\"")]
            if p.returncode == 0 and found and n:
                line["profile"][o] = kernel_summary(found[0], o, 3, n[0])
                if a.out:
                    shutil.copy(found[0], os.path.splitext(a.out)[0] + f"_{o.lower()}_kernel_stats.csv")
            else:
                line["profile"][o] = {"error": f"rocprofv3 exit {p.returncode}", "tail": (p.stdout + p.stderr)[-800:]}
            shutil.rmtree(work, ignore_errors=True)
            if p.returncode != 0:
                break                          # a failed child: start nothing more on the GPU
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
