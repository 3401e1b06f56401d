"""A/B of the KV cache type of generate_batch at the full model size: kv_cache="fp16" against "fp8" (KV8), under both decode_weights,
in ONE process with the arms alternating (profiles/decode_kv8.txt).  One MI355X; measurement tool, never on the product path.

    python tools/ab_kv8.py [--batch 8 32] [--text-len 240 1008] [--new 64] [--reps 5] [--out FILE]

ms per decode step = (t(new tokens) - t(1 token)) / (new - 1), host clock around device synchronises, hipGraph replay, reference
sampling settings; median, min and max over the repetitions.  Quality (recorded, asserted nowhere): greedy decoding without logits
processors, the last step's logits of the fp8-cache arm against the fp16-cache arm (relative error over all rows) and the number of
greedy tokens that differ."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tcavt_amd import capi, config, model, synth
from tcavt_amd.weights import make_weights

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[8, 32])
ap.add_argument("--text-len", type=int, nargs="+", default=[240, 1008])
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--preset", default="llama32_1b")
ap.add_argument("--out", default=None)
args = ap.parse_args()
capi.init(0)
dev = torch.device("cuda:0")
cfg = config.PRESETS[args.preset]()
ll = cfg.llama
with torch.device(dev):
    m = model.MultiModalTrajectoryModel.from_config(cfg)
m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


ARMS = [(dw, kv) for dw in ("fp16", "fp8") for kv in ("fp16", "fp8")]
say(f"{args.preset}, synthetic weights, {args.new} new tokens, hipGraph replay, sampling T=0.9 top-k 40 top-p 0.9 rep 1.2 no-repeat-3; "
    f"{args.reps} repetitions per arm, arms alternating inside each repetition")
say("  B  prompt  weights  cache   ms/step median      min      max   cache MB/step   prefill+1 ms")
for B in args.batch:
    for Lt in args.text_len:
        b = synth.make_batch(cfg, B, text_len=Lt, seed=3, ragged=False)  # full-length prompts: every sample reads 16 + Lt + step rows
        g = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k in ("vision_emb", "input_ids", "attention_mask")}

        def run(n, dw, kv, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=n, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                                        decode_weights=dw, kv_cache=kv, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        for dw, kv in ARMS:  # packed weights, workspaces, every kernel form, clocks
            run(4, dw, kv)
            run(args.new, dw, kv)
        res = {a: [] for a in ARMS}
        for _ in range(args.reps):
            for dw, kv in ARMS:
                t1, _ = run(1, dw, kv)
                tn, _ = run(args.new, dw, kv)
                res[(dw, kv)].append(((tn - t1) / (args.new - 1) * 1e3, t1 * 1e3))
        rows = 16 + Lt + args.new / 2
        for dw, kv in ARMS:
            r = sorted(res[(dw, kv)])
            mb = 2 * ll.layers * B * rows * ll.n_kv_heads * (66 if kv == "fp8" else 128) / 1e6
            say(f" {B:2d}  16+{Lt:<4d}  {dw:>6s}  {kv:>5s}        {r[len(r) // 2][0]:8.4f} {r[0][0]:8.4f} {r[-1][0]:8.4f}   {mb:10.1f}   {r[len(r) // 2][1]:10.2f}")
        # quality: greedy, no processors; the last step's logits and the tokens, fp8 cache against fp16 cache
        for dw in ("fp16", "fp8"):
            q = {}
            for kv in ("fp16", "fp8"):
                _, out = run(args.new, dw, kv, do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
                logits = m.mllm._ws.get("gen.logits", (B, ll.vocab), torch.float32, dev).double().clone()
                q[kv] = (out.clone(), logits)
            rel = ((q["fp8"][1] - q["fp16"][1]).norm() / q["fp16"][1].norm()).item()
            diff = int((q["fp8"][0] != q["fp16"][0]).sum())
            same = int((q["fp8"][0] == q["fp16"][0]).all(1).sum())
            say(f"     quality B={B} 16+{Lt} weights={dw}: last step's logits rel_err(fp8 cache vs fp16 cache) {rel:.4e}; greedy tokens that differ "
                f"{diff} of {B * args.new}; samples with identical continuation {same}/{B}")
