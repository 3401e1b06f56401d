"""What the per-request parameter table costs (tcavt_sample_tokens_per_request against the entries that take the parameters by
value), at the full model size (Llama-3.2-1B shape) on one MI355X, in one process.
    python tools/bench_generate_per_request.py [--requests 256] [--slots 8 32] [--admit-group 4] [--reps 5] [--out FILE]
1. The sampler launch alone (stage 1 + stage 2, V = 128 256, the slots form the pool's decode loop uses) at B = 8 and 32: windows of
   200 calls between device events, the two arms alternating, --reps windows each; median and range in us per call.  Without
   processors nothing has to be reset between calls, so the window holds the two sampler launches and nothing else; with the
   reference's processors the scores are restored before every call (one copy_ and one fill_ launch in both arms).
2. generate_pool on the request list of tools/bench_generate_pool.py (256 requests, prompt 16 + 240 ragged, budgets uniform 16..128,
   seed 7) at every --slots with admit_group --admit-group: the arguments as scalars (the path of a call without the feature)
   against the SAME values given as lists of R, alternating inside a repetition; greedy as in profiles/generate_pool.txt, and
   sampling with the reference's settings.  Wall time per run, median and range; the two arms' tokens are compared."""
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


# ---- 1. the sampler launch alone
V, CALLS = 128256, 200
for B in (8, 32):
    gen = torch.Generator().manual_seed(B)
    base = (torch.randn(B, V, generator=gen) * 6.0).to(dev)
    hist0 = torch.randint(0, V, (B, 320), generator=gen).to(dev)
    for name, (rep_pen, ngram) in (("sampling, no processors", (1.0, 0)), ("sampling + processors", (1.2, 3))):
        sp = capi.SampleParams(0.9, 0.9, rep_pen, 40, ngram, 1, -1, 0, 7)
        table = ops.RequestTable([sp] * B).to(dev)
        arms = {}
        for arm in ("by value", "table"):
            st = dict(logits=base.clone(), hist=hist0.clone(), hl=torch.full((B,), 300, dtype=torch.int32, device=dev),
                      step=torch.zeros(B, dtype=torch.int32, device=dev), mx=torch.full((B,), 1 << 30, dtype=torch.int32, device=dev),
                      orow=torch.arange(B, dtype=torch.int64, device=dev), cur=torch.zeros(B, dtype=torch.int64, device=dev),
                      pos=torch.zeros(B, dtype=torch.int32, device=dev), fin=torch.zeros(B, dtype=torch.int32, device=dev),
                      out=torch.zeros(B, 64, dtype=torch.int64, device=dev), ws=ops.sample_workspace(B, dev))

            def call(st=st, arm=arm):
                if ngram or rep_pen != 1.0:  # (the penalty and the bans are applied in place: fresh scores and history per call)
                    st["logits"].copy_(base)
                    st["hl"].fill_(300)
                if arm == "table":
                    ops.sample_tokens(st["logits"], st["hist"], st["hl"], sp, st["step"], st["cur"], st["pos"], st["fin"], st["out"],
                                      advance_pos=True, workspace=st["ws"], max_new=st["mx"], out_row=st["orow"], per_request=table)
                else:
                    ops.sample_logits_slots(st["logits"], st["hist"], st["hl"], sp, st["step"], st["mx"], st["orow"], st["cur"], st["pos"],
                                            st["fin"], st["out"], advance_pos=True, workspace=st["ws"])

            arms[arm] = (call, [])
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
        a, b = arms["by value"][1], arms["table"][1]
        report(sampler=name, B=B, V=V, form="slots, two-stage", calls_per_window=CALLS, windows=args.reps, by_value_us=spread(a),
               table_us=spread(b), table_minus_by_value_us=round(statistics.median(b) - statistics.median(a), 2),
               includes="the two sampler launches" + (", a copy_ of the scores and a fill_" if ngram or rep_pen != 1.0 else " only"))
        assert int(table.flag.item()) == 0

# ---- 2. generate_pool, scalars against the same values as lists
cfg = config.PRESETS[args.preset]()
with torch.device(dev):
    m = model.MultiModalTrajectoryModel.from_config(cfg)
m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
R, G = args.requests, args.admit_group
b = synth.make_batch(cfg, R, text_len=args.text_len, seed=3, ragged=True, min_text=min(128, args.text_len // 2))
g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
budgets = np.random.default_rng(7).integers(args.min_new, args.max_new + 1, size=R).tolist()
useful = int(sum(budgets))
WORKLOADS = {
    "greedy": dict(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0),
    "sampling": dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.2, no_repeat_ngram_size=3, seed=5),
}


def run_pool(S, kw, n=R):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.mllm.generate_pool(g["vision_emb"][:n], g["input_ids"][:n], g["attention_mask"][:n], max_new_tokens=budgets[:n], slots=S,
                               poll_every=1, admit_group=G, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


report(workload=f"{R} requests, prompt {cfg.q_num_query_tokens}+{args.text_len} tokens (ragged), budgets uniform {args.min_new}..{args.max_new} "
                f"(seed 7): {useful} useful tokens; admit_group {G}, poll_every 1, fp16 weights and cache; hipGraph replay", preset=args.preset)
for wname, kw in WORKLOADS.items():
    for S in args.slots:
        as_lists = lambda n: {k: [v] * n for k, v in kw.items()}  # noqa: E731
        for arm_kw in (kw, as_lists(min(R, 2 * S))):  # warm-up of every shape and capture path the timed windows use
            run_pool(S, arm_kw, n=min(R, 2 * S))
        times = {"scalars": [], "lists": []}
        outs = {}
        for rep in range(args.reps):
            for arm, arm_kw in (("scalars", kw), ("lists", as_lists(R))):
                t, out = run_pool(S, arm_kw)
                times[arm].append(t)
                outs[arm] = out.clone()
        ms, ml = statistics.median(times["scalars"]), statistics.median(times["lists"])
        report(path="generate_pool", workload=wname, slots=S, admit_group=G, reps=args.reps, scalars_wall_s=spread(times["scalars"], 3),
               lists_wall_s=spread(times["lists"], 3), lists_over_scalars=round(ml / ms, 4),
               scalars_useful_tokens_per_s=round(useful / ms, 1), lists_useful_tokens_per_s=round(useful / ml, 1),
               decode_steps=m.mllm.pool_stats["steps"], tokens_equal=bool(torch.equal(outs["scalars"], outs["lists"])))
m.mllm.check_flags()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
