"""Prompt-lookup speculative decoding at the full model size (Llama-3.2-1B shape): generate_batch(prompt_lookup_num_tokens=k)
against the call without it, arms alternating in one process.  One MI355X.
    python tools/bench_prompt_lookup.py [--k 3] [--batches 1,4,8] [--new 64] [--text-len 240] [--reps 5] [--ngram 2]

The 16 + text-len prompt, --new tokens, hipGraph replay, synthetic weights.  Three workloads: "random" -- synth.make_batch's prompts,
greedy selection without the repetition processors, whatever acceptance that yields --, "pattern" -- the same selection on prompts
that are a 2- to 5-id pattern repeated over their whole length, so that the sequence ends in an n-gram that occurred before from
the first step on (a prompt that contains the model's own continuation cannot be built for random weights: changing the prompt
changes the continuation) -- and "sampled" -- the random prompts under the reference's defaults (temperature 0.9, top-k 40, top-p
0.9, repetition penalty 1.2, no-repeat-3-gram), which exist to keep the text from repeating.

Per batch size and workload, from --reps alternating pairs (median; min and max next to it): ms per call (prefill + --new tokens,
ending in a device synchronise); ms per decode step = (call - call with one new token) / steps run, for both arms; the ratio of the
two step costs -- the mean number of tokens a step must commit for the feature to break even, which does not depend on the text;
tokens committed per step = (--new - 1) / steps run (the batch leaves when its slowest row is done); drafted and accepted ids;
whether the tokens of the two arms are equal.  The sampled workload also runs the PLAIN call on the prompts tiled to k + 1 times
the rows (row s is the same prompt with the same Philox row) and reports how many of the first S rows keep their tokens: what the row
count alone does to a sampled row, without the feature."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tcavt_amd import capi, config, model, synth
from tcavt_amd.weights import make_weights

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=3)
ap.add_argument("--ngram", type=int, default=2)
ap.add_argument("--batches", default="1,4,8")
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--text-len", type=int, default=240)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--preset", default="llama32_1b")
args = ap.parse_args()
capi.init(0)
dev = torch.device("cuda:0")
cfg = config.PRESETS[args.preset]()
with torch.device(dev):
    m = model.MultiModalTrajectoryModel.from_config(cfg)
m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
N = args.new
stat = lambda v: dict(median=round(sorted(v)[len(v) // 2], 4), min=round(min(v), 4), max=round(max(v), 4))


def prompts(S, workload):
    b = synth.make_batch(cfg, S, text_len=args.text_len, seed=3, ragged=False)
    g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    if workload == "pattern":
        gen = torch.Generator().manual_seed(7)
        rows = []
        for s in range(S):
            pat = torch.randint(1, cfg.llama.vocab, (2 + s % 4,), generator=gen)
            rows.append(pat.repeat(args.text_len)[:args.text_len])
        g["input_ids"] = torch.stack(rows).to(dev)
    return g


def call(g, new, k, sampled):
    sel = dict(do_sample=True, seed=5) if sampled else dict(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, info = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=new, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                                      use_graph=True, return_info=True, prompt_lookup_num_tokens=k, max_matching_ngram_size=args.ngram, **sel)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out, info


for workload in ("random", "pattern", "sampled"):
    for S in (int(s) for s in args.batches.split(",")):
        g = prompts(S, workload)
        arms = {"plain": None, "lookup": args.k}
        sampled = workload == "sampled"
        for k in arms.values():  # packed weights, workspaces, every kernel form, the clocks
            call(g, 4, k, sampled)
            call(g, N, k, sampled)
        ms_call, ms_step, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
        for _ in range(args.reps):
            for a, k in arms.items():
                t1, _, _ = call(g, 1, k, sampled)
                tn, out, info = call(g, N, k, sampled)
                ms_call[a].append(tn)
                ms_step[a].append((tn - t1) / max(info["steps"], 1))
                last[a] = (out, info)
        m.mllm.check_flags()
        info = last["lookup"][1]
        tiled = None
        if sampled:
            g4 = {k_: v.repeat(args.k + 1, *([1] * (v.dim() - 1))).contiguous() for k_, v in g.items()}
            tiled = int((call(g4, N, None, True)[1][:S] == last["plain"][0]).all(1).sum())
        sp, sl = stat(ms_step["plain"]), stat(ms_step["lookup"])
        drafted, accepted = int(info["drafted"].sum()), int(info["accepted"].sum())
        print(json.dumps({
            "workload": f"{workload}, S={S}, prompt {cfg.q_num_query_tokens}+{args.text_len}, {N} new tokens, "
                        f"{'sampling at the reference defaults' if sampled else 'greedy, no repetition processors'}, hipGraph replay, k={args.k}, max_matching_ngram_size={args.ngram}; {args.reps} alternating pairs",
            "rows_per_step": {"plain": S, "lookup": S * (args.k + 1)},
            "ms_per_step": {"plain": sp, "lookup": sl},
            "break_even_tokens_per_step": round(sl["median"] / sp["median"], 3),
            "steps": {"plain": last["plain"][1]["steps"], "lookup": info["steps"]},
            "tokens_per_step": {"plain": 1.0, "lookup": round((N - 1) / max(info["steps"], 1), 3)},
            "drafted": drafted, "accepted": accepted, "acceptance": round(accepted / max(drafted, 1), 3),
            "accepted_per_sequence": info["accepted"].tolist(),
            "ms_per_call": {"plain": stat(ms_call["plain"]), "lookup": stat(ms_call["lookup"])},
            "lookup_over_plain_call": round(stat(ms_call["lookup"])["median"] / stat(ms_call["plain"])["median"], 4),
            "tokens_equal_between_arms": bool(torch.equal(last["plain"][0], last["lookup"][0])),
            "rows_equal_between_arms": int((last["plain"][0] == last["lookup"][0]).all(1).sum()),
            "plain_rows_equal_when_tiled_to_lookup_row_count": tiled}), flush=True)
