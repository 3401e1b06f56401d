"""A request list through the slot pool (LlamaMultiModal.generate_pool) against the same requests as consecutive generate_batch
calls, at the full model size (Llama-3.2-1B shape) on one MI355X, in one process.
    python tools/bench_generate_pool.py [--requests 256] [--text-len 240] [--min-new 16] [--max-new 128] [--slots 8 32]
                                        [--poll 1 8 32] [--admit-group 1 2 4 8] [--reps 2] [--out profiles/generate_pool.txt]
Requests end on per-request token budgets drawn uniformly from [min-new, max-new] with a fixed seed (random weights do not emit
EOS on cue).  The baseline is what a caller has without the pool: batches of B requests, each run for max-new tokens (a static
batch cannot know its rows' budgets: with EOS it runs until max_new_tokens whatever its rows do).  Greedy, fp16 weights and cache.
Reported per configuration: wall time, useful tokens / s = sum of the budgets / wall time, and for the pool the decode steps and
the mean number of live slots per step (tokens chosen in decode steps / steps).
--admit-group: the widths G of the grouped admission (generate_pool(admit_group=G)) to run as further arms, 1 = one request per
prefill; per arm also the group passes and the pad rows they carried, and after each repetition, per G, equal_across_pool_sizes = the
requests whose tokens are identical at every pool size (the contract of a fixed G: all of them).
--stop-fraction F: the token-driven workload instead (stop_workload below) -- sampling, one budget --max-new for every request, a stop
bitmap over a seeded random fraction F of the vocabulary; arms: generate_batch with the rules off, on and unpolled (the baseline), with
poll_every from --batch-poll, and generate_pool per --slots x --admit-group at poll_every = --poll[0]."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tcavt_amd import capi, config, model, synth
from tcavt_amd.weights import make_weights

ap = argparse.ArgumentParser()
ap.add_argument("--requests", type=int, default=256)
ap.add_argument("--text-len", type=int, default=240)
ap.add_argument("--min-new", type=int, default=16)
ap.add_argument("--max-new", type=int, default=128)
ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
ap.add_argument("--poll", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--admit-group", type=int, nargs="+", default=[1])
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--preset", default="llama32_1b")
ap.add_argument("--out", default=None, help="also write the result lines to this file")
ap.add_argument("--stop-fraction", type=float, default=None,
                help="run the token-driven workload instead: sampling on, every request has the budget --max-new and ends on a stop "
                     "bitmap that covers this (seeded random) fraction of the vocabulary")
ap.add_argument("--batch-poll", type=int, nargs="+", default=[1, 8], help="token-driven workload: poll_every arms of generate_batch")
args = ap.parse_args()
capi.init(0)
dev = torch.device("cuda:0")
cfg = config.PRESETS[args.preset]()
with torch.device(dev):
    m = model.MultiModalTrajectoryModel.from_config(cfg)
m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
R = args.requests
b = synth.make_batch(cfg, R, text_len=args.text_len, seed=3, ragged=True, min_text=min(128, args.text_len // 2))
g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
budgets = np.random.default_rng(7).integers(args.min_new, args.max_new + 1, size=R).tolist()
useful = int(sum(budgets))
kw = dict(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)


def run_batches(B, n=R):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = [m.mllm.generate_batch(g["vision_emb"][i:i + B], None, max_new_tokens=args.max_new, input_ids=g["input_ids"][i:i + B],
                                  attention_mask=g["attention_mask"][i:i + B], **kw).clone() for i in range(0, n, B)]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cat(outs)


def run_pool(S, poll, n=R, G=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.mllm.generate_pool(g["vision_emb"][:n], g["input_ids"][:n], g["attention_mask"][:n], max_new_tokens=budgets[:n], slots=S,
                               poll_every=poll, admit_group=G, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


lines = []


def report(**rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def stop_workload():
    """Ends that depend on the tokens: sampling with the reference's settings, one budget (--max-new) for every request, and a stop
    set = a seeded random fraction of the vocabulary, so that random weights give roughly geometric lengths.  Arms, alternating inside
    a repetition: generate_batch with the rules off (the launch sequence of a call without the feature), with the rules on and no
    polling (the baseline: the same number of steps), with poll_every from --batch-poll, and generate_pool per --slots x
    --admit-group at poll_every = --poll[0].  Useful tokens of an arm = the sum of its own n_generated (rules off: the rows cut on
    the host by StopRules.first_end)."""
    from tcavt_amd.stopping import StopRules

    V, N = cfg.llama.vocab, args.max_new
    ids = torch.nonzero(torch.rand(V, generator=torch.Generator().manual_seed(11)) < args.stop_fraction).flatten().tolist()
    rules = StopRules(V, stop_token_ids=ids)
    skw = dict(do_sample=True, seed=5)
    rk = dict(stop_token_ids=ids, return_info=True)

    def batches(B, n=R, poll=None, on=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_gen, steps = [], 0
        for i in range(0, n, B):
            sl = slice(i, i + B)
            res = m.mllm.generate_batch(g["vision_emb"][sl], None, max_new_tokens=N, input_ids=g["input_ids"][sl],
                                        attention_mask=g["attention_mask"][sl], poll_every=poll, **skw, **(rk if on else {}))
            if on:
                n_gen += res[1]["n_generated"].tolist()
                steps += res[1]["steps"]
            else:
                n_gen.append(res.clone())
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if not on:  # (outside the timed window)
            n_gen = [rules.first_end(row, None, budget=N)[0] for o in n_gen for row in o.tolist()]
            steps = -(-n // B) * (N - 1)
        return t, n_gen, steps

    def pool(S, G, n=R):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, st = m.mllm.generate_pool(g["vision_emb"][:n], g["input_ids"][:n], g["attention_mask"][:n], max_new_tokens=N, slots=S,
                                     poll_every=args.poll[0], admit_group=G, **skw, **rk)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, st["n_generated"].tolist(), st["steps"]

    for S in args.slots:  # warm-up of every shape and capture path the timed windows use
        for poll in [None] + args.batch_poll:
            batches(S, n=S, poll=poll)
        batches(S, n=S, on=False)
        for G in args.admit_group:
            if G <= S:
                pool(S, G, n=min(R, 2 * S))
    for rep in range(args.reps):
        for S in args.slots:
            arms = [("generate_batch, rules off", lambda: batches(S, on=False), {}),
                    ("generate_batch", lambda: batches(S), dict(poll_every=None))]
            arms += [("generate_batch", lambda p=p: batches(S, poll=p), dict(poll_every=p)) for p in args.batch_poll]
            arms += [("generate_pool", lambda G=G: pool(S, G), dict(poll_every=args.poll[0], admit_group=G)) for G in args.admit_group if G <= S]
            for path, fn, extra in arms:
                t, n_gen, steps = fn()
                tot = int(sum(n_gen))
                rec = dict(path=path, rows=S, rep=rep, wall_s=round(t, 3), useful_tokens=tot, mean_length=round(tot / R, 1),
                           useful_tokens_per_s=round(tot / t, 1), decode_steps=steps, **extra)
                if rep == 0 and path == "generate_batch" and extra.get("poll_every") is None:
                    hist = np.bincount(np.minimum((np.asarray(n_gen) - 1) // 16, N // 16 - 1), minlength=N // 16).tolist()
                    rec.update(length_histogram_16=hist, ended_by_stop_token=int(sum(x < N for x in n_gen)))
                report(**rec)


if args.stop_fraction is not None:
    report(workload=f"{R} requests, prompt {cfg.q_num_query_tokens}+{args.text_len} tokens (ragged), budget {args.max_new} each; sampling "
                    f"(temperature 0.9, top-k 40, top-p 0.9, penalty 1.2, no-repeat 3-grams, seed 5); stop set = a random "
                    f"{args.stop_fraction} of the vocabulary (seed 11); fp16 weights and cache; hipGraph replay", preset=args.preset)
    stop_workload()
    m.mllm.check_flags()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

report(workload=f"{R} requests, prompt {cfg.q_num_query_tokens}+{args.text_len} tokens (ragged), budgets uniform {args.min_new}..{args.max_new} "
                f"(seed 7): {useful} useful tokens, mean {useful / R:.1f}; greedy, fp16 weights and cache; hipGraph replay",
       preset=args.preset)
ref = {}
for S in args.slots:  # warm-up of every shape the timed windows use: packed weights, workspaces, kernels, graph capture paths
    run_batches(S, n=S)
    for G in args.admit_group:  # (2 S requests: the eager group pass, its capture and a replay)
        if G <= S:
            run_pool(S, args.poll[0], n=min(R, 2 * S), G=G)
for rep in range(args.reps):  # (the configurations alternate inside a repetition: the spread between repetitions is the noise)
    by_group = {}
    for S in args.slots:
        t, out_b = run_batches(S)
        ref[S] = out_b
        report(path="generate_batch", batch=S, rep=rep, wall_s=round(t, 3), useful_tokens_per_s=round(useful / t, 1),
               decode_rows_computed=R * (args.max_new - 1), useful_share=round((useful - R) / (R * (args.max_new - 1)), 3))
        for poll, G in ((p_, g_) for p_ in args.poll for g_ in args.admit_group if g_ <= S):
            t, out_p = run_pool(S, poll, G=G)
            st = m.mllm.pool_stats
            by_group.setdefault((poll, G), []).append(out_p.clone())
            # a request's tokens in the pool are those of its row in a static batch, up to its budget (greedy; both paths compute a
            # row independently of its neighbours, but a B = 1 prefill may round differently from the batched one: reported, not asserted)
            same = sum(bool(torch.equal(out_p[r, :budgets[r]], out_b[r, :budgets[r]])) for r in range(R))
            report(path="generate_pool", slots=S, poll_every=poll, admit_group=G, rep=rep, wall_s=round(t, 3),
                   useful_tokens_per_s=round(useful / t, 1), decode_steps=st["steps"],
                   mean_live_slots_per_step=round((useful - R) / st["steps"], 2), group_passes=len(st["groups"]),
                   pad_rows=sum(G - len(reqs) for reqs, _, _ in st["groups"]),
                   requests_equal_to_static_batch=f"{same}/{R}",
                   finite=bool(((out_p >= 0) & (out_p < cfg.llama.vocab)).all().item()))
    for (poll, G), outs in by_group.items():
        if len(outs) > 1:
            same = sum(all(bool(torch.equal(o[r], outs[0][r])) for o in outs[1:]) for r in range(R))
            report(check="equal_across_pool_sizes", poll_every=poll, admit_group=G, rep=rep, slots=[S for S in args.slots if G <= S],
                   requests=f"{same}/{R}")
m.mllm.check_flags()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
