"""What constrained decoding costs (tcavt_constraint_mask / tcavt_constraint_advance around every token selection), at the full
model size (Llama-3.2-1B shape) on one MI355X, in one process, the arms alternating.
    python tools/bench_generate_constraint.py [--requests 256] [--slots 8 32] [--admit-group 4] [--reps 5] [--out FILE]
Arms: "none" (no constraint: launch for launch the call of the parent commit), "free" (one state that allows everything), "one"
(one state that allows exactly one token), "1pct" (one state that allows every 100th id).
1. The two launches alone (V = 128 256, the slots form the pool's decode loop uses) at B = 8 and 32: windows of 200 mask + advance
   pairs between device events on fresh scores (one copy_ per pair, timed on its own and subtracted); median and range in us.
2. The decode step of generate_batch at B = 8 and 32 (prompt 16 + 240 tokens, greedy, hipGraph replay): wall time of a call with
   161 new tokens minus one with 33, over the 128 steps between them.
3. generate_pool on the request list of tools/bench_generate_pool.py (256 requests, prompt 16 + 240 ragged, budgets uniform 16..128,
   seed 7) at every --slots with admit_group --admit-group, greedy.  Wall time per run, median and range; the "free" arm's tokens
   are compared with the "none" arm's."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tcavt_amd import capi, config, model, ops, synth
from tcavt_amd.constraint import TokenConstraint
from tcavt_amd.weights import make_weights

ap = argparse.ArgumentParser()
ap.add_argument("--requests", type=int, default=256)
ap.add_argument("--text-len", type=int, default=240)
ap.add_argument("--min-new", type=int, default=16)
ap.add_argument("--max-new", type=int, default=128)
ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
ap.add_argument("--admit-group", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--preset", default="llama32_1b")
ap.add_argument("--out", default=None, help="also write the result lines to this file")
args = ap.parse_args()
capi.init(0)
dev = torch.device("cuda:0")
lines = []


def report(**rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def spread(xs, digits=1):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits))


cfg = config.PRESETS[args.preset]()
V = cfg.llama.vocab
ONE_TOKEN = 1234
FORMS = {"free": TokenConstraint.free(V), "one": TokenConstraint.from_allowed_tokens(V, [ONE_TOKEN]),
         "1pct": TokenConstraint.from_allowed_tokens(V, range(0, V, 100))}

# ---- 1. the two launches alone
CALLS = 200
for B in (8, 32):
    gen = torch.Generator().manual_seed(B)
    base = (torch.randn(B, V, generator=gen) * 6.0).to(dev)
    logits = base.clone()
    step, fin = torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    orow = torch.arange(B, dtype=torch.int64, device=dev)
    arms = {"copy only": (lambda: logits.copy_(base), [])}
    for name, C in FORMS.items():
        T = ops.ConstraintTable(C.token_class, C.trans, dev).build()
        tok = ONE_TOKEN if name == "one" else 0
        a = ops.constraint_args(T, logits, step, fin, torch.full((B,), tok, dtype=torch.int64, device=dev),
                                torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                                torch.empty(ops.constraint_workspace_bytes(B), dtype=torch.uint8, device=dev), out_row=orow,
                                flag=torch.zeros(1, dtype=torch.int32, device=dev))

        def pair(a=a, T=T):
            logits.copy_(base)
            ops.constraint_mask(a)
            ops.constraint_advance(a)

        arms[name] = (pair, [])
    for call, _ in arms.values():
        for _ in range(20):
            call()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for call, times in arms.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / CALLS * 1e3)
    copy = statistics.median(arms["copy only"][1])
    report(launches="constraint_mask + constraint_advance", B=B, V=V, form="slots", calls_per_window=CALLS, windows=args.reps,
           copy_only_us=spread(arms["copy only"][1]), **{f"{k}_us": spread(v[1]) for k, v in arms.items() if k != "copy only"},
           **{f"{k}_minus_copy_us": round(statistics.median(v[1]) - copy, 2) for k, v in arms.items() if k != "copy only"})

# ---- the model
with torch.device(dev):
    m = model.MultiModalTrajectoryModel.from_config(cfg)
m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
R, G = args.requests, args.admit_group
b = synth.make_batch(cfg, R, text_len=args.text_len, seed=3, ragged=True, min_text=min(128, args.text_len // 2))
g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
GREEDY = dict(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
ARMS = [("none", {})] + [(k, dict(constraint=C)) for k, C in FORMS.items()]

# ---- 2. the decode step of generate_batch
N_SHORT, N_LONG = 33, 161


def run_batch(B, N, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.mllm.generate_batch(g["vision_emb"][:B], None, max_new_tokens=N, input_ids=g["input_ids"][:B], attention_mask=g["attention_mask"][:B],
                          **GREEDY, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for B in (8, 32):
    for _, kw in ARMS:  # warm-up of every shape and capture path
        run_batch(B, N_SHORT, kw)
    steps = {k: [] for k, _ in ARMS}
    for rep in range(args.reps):
        for k, kw in ARMS:
            steps[k].append((run_batch(B, N_LONG, kw) - run_batch(B, N_SHORT, kw)) / (N_LONG - N_SHORT) * 1e3)
    none = statistics.median(steps["none"])
    report(path="generate_batch decode step", B=B, prompt=f"{cfg.q_num_query_tokens}+{args.text_len}", greedy=True, reps=args.reps,
           steps_between=N_LONG - N_SHORT, **{f"{k}_ms_per_step": spread(v, 4) for k, v in steps.items()},
           **{f"{k}_over_none": round(statistics.median(v) / none, 4) for k, v in steps.items() if k != "none"})

# ---- 3. generate_pool on the request list
budgets = np.random.default_rng(7).integers(args.min_new, args.max_new + 1, size=R).tolist()
useful = int(sum(budgets))


def run_pool(S, kw, n=R):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.mllm.generate_pool(g["vision_emb"][:n], g["input_ids"][:n], g["attention_mask"][:n], max_new_tokens=budgets[:n], slots=S,
                               poll_every=1, admit_group=G, **GREEDY, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


report(workload=f"{R} requests, prompt {cfg.q_num_query_tokens}+{args.text_len} tokens (ragged), budgets uniform {args.min_new}..{args.max_new} "
                f"(seed 7): {useful} useful tokens; greedy, admit_group {G}, poll_every 1, fp16 weights and cache; hipGraph replay", preset=args.preset)
for S in args.slots:
    for _, kw in ARMS:
        run_pool(S, kw, n=min(R, 2 * S))
    times, outs = {k: [] for k, _ in ARMS}, {}
    for rep in range(args.reps):
        for k, kw in ARMS:
            t, out = run_pool(S, kw)
            times[k].append(t)
            outs[k] = out.clone()
    none = statistics.median(times["none"])
    report(path="generate_pool", slots=S, admit_group=G, reps=args.reps, decode_steps=m.mllm.pool_stats["steps"],
           **{f"{k}_wall_s": spread(v, 3) for k, v in times.items()},
           **{f"{k}_over_none": round(statistics.median(v) / none, 4) for k, v in times.items() if k != "none"},
           free_tokens_equal_none=bool(torch.equal(outs["free"], outs["none"])),
           one_says_its_token_only=bool((outs["one"] == ONE_TOKEN).sum().item() == useful))
m.mllm.check_flags()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
