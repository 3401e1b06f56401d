"""Text-generation throughput at the full model size (Llama-3.2-1B shape): prefill + hipGraph-replayed decode steps
(BASELINE.json configs[4] "hipGraph-captured decode"; reference: scripts/train.py:577-654).  One MI355X.
    python tools/bench_generate.py [--batch 32] [--new 64] [--text-len 240] [--no-graph] [--greedy] [--decode-weights fp8] [--kv-cache fp8]
        [--num-return-sequences 8 [--share-prefix]] [--logprobs] [--top-logprobs 5 20 [--pool-slots 8 32]]"""
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
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--text-len", type=int, default=240)
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--greedy", action="store_true")
ap.add_argument("--preset", default="llama32_1b")
ap.add_argument("--decode-weights", choices=["fp16", "fp8"], default="fp16", help="what the decode step streams (generate_batch)")
ap.add_argument("--kv-cache", choices=["fp16", "fp8"], default="fp16", help="what the KV cache holds (generate_batch): 16-bit rows or KV8")
ap.add_argument("--num-return-sequences", type=int, default=1,
                help="n > 1: A/B of generate_batch(num_return_sequences=n) on --batch prompts against generate_batch on the prompts "
                     "repeated to batch * n rows, arms alternating; and the tcavt_kv_fanout launch on its own")
ap.add_argument("--reps", type=int, default=7, help="timed pairs of the n > 1 A/B")
ap.add_argument("--share-prefix", action="store_true",
                help="with --num-return-sequences n: A/B of arm (a) num_return_sequences=n against arm (c) = (a) + share_prefix=True, "
                     "arms alternating in one process; and one layer's attention launch, both kernels, on the buffers the calls left")
ap.add_argument("--logprobs", action="store_true",
                help="A/B of generate_batch(return_logprobs=True) against the call without it, arms alternating in one process: "
                     "ms per decode step of each arm (the two launches of the bracket and one more read of the logits)")
ap.add_argument("--top-logprobs", type=int, nargs="+", default=None, metavar="K",
                help="A/B of generate_batch(return_logprobs=True, top_logprobs=k) for every k given against return_logprobs=True "
                     "alone, arms alternating in one process: ms per decode step of each arm (the two launches of "
                     "tcavt_logprob_topk and one more read of the logits)")
ap.add_argument("--pool-slots", type=int, nargs="*", default=[],
                help="with --top-logprobs: also one generate_pool run per arm and slot count on a 256-request list (budgets 16 .. 128)")
args = ap.parse_args()
capi.init(0)
dev = torch.device("cuda:0")
cfg = config.PRESETS[args.preset]()
with torch.device(dev):
    m = model.MultiModalTrajectoryModel.from_config(cfg)
m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
b = synth.make_batch(cfg, args.batch, text_len=args.text_len, seed=3, ragged=True, min_text=min(128, args.text_len // 2))
g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
kw = dict(input_ids=g["input_ids"], attention_mask=g["attention_mask"], do_sample=not args.greedy, use_graph=not args.no_graph,
          decode_weights=args.decode_weights, kv_cache=args.kv_cache)


def run(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=n, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def nsamples_ab(n):
    """(a) the prompts once, n continuations each; (b) the prompts repeated n times (repeat_interleave: the same row order).  Each
    timed call is a whole generation -- prefill, fan-out or not, args.new tokens -- ending in a device synchronise."""
    from tcavt_amd import generation, ops

    rep = {k: g[k].repeat_interleave(n, 0).contiguous() for k in ("vision_emb", "input_ids", "attention_mask")}
    kw_b = dict(kw, input_ids=rep["input_ids"], attention_mask=rep["attention_mask"])

    def arm(which, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "a":
            out = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=new, num_return_sequences=n, **kw)
        else:
            out = m.mllm.generate_batch(rep["vision_emb"], None, max_new_tokens=new, **kw_b)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for which in "ab":  # packed weights, workspaces, every kernel form, the clocks
        arm(which, 4)
        arm(which, args.new)
    times = {"a": [], "b": []}
    for _ in range(args.reps):
        for which in "ab":
            t, out = arm(which, args.new)
            times[which].append(t * 1e3)
    m.mllm.check_flags()
    stat = lambda v: dict(median=round(sorted(v)[len(v) // 2], 2), min=round(min(v), 2), max=round(max(v), 2))
    # the fan-out launch on its own, on the buffers the last (a) call left in the workspace
    LW, ws = m.mllm.llama_wrapper, m.mllm._ws
    ll, Nq, Lt, B = LW.shape, cfg.q_num_query_tokens, args.text_len, args.batch
    src = generation.cache_buffers(ws, "gen.src", LW, args.kv_cache, B, Nq + Lt, dev)
    dst = generation.cache_buffers(ws, "gen", LW, args.kv_cache, B * n, Nq + Lt + args.new, dev)
    lsrc = ws.get("gen.src.logits", (B, ll.vocab), torch.float32, dev)
    ldst = ws.get("gen.logits", (B * n, ll.vocab), torch.float32, dev)
    hist = torch.zeros(B * n, Lt + args.new, dtype=torch.int64, device=dev)
    i32 = lambda: torch.zeros(B * n, dtype=torch.int32, device=dev)

    def fan():
        ops.kv_fanout(src, dst, n, Nq + Lt, Nq + Lt, Nq + Lt + args.new, ll.layers, ll.n_kv_heads, g["input_ids"],
                      ws.get("gen.src.kvlen", (B,), torch.int32, dev), Nq, lsrc, ldst, hist, i32(), i32(), i32())

    fan()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fan_ms = []
    for _ in range(20):
        ev[0].record()
        fan()
        ev[1].record()
        ev[1].synchronize()
        fan_ms.append(ev[0].elapsed_time(ev[1]))
    row = (66 if args.kv_cache == "fp8" else 2 * ll.head_dim) * ll.n_kv_heads * 2 * ll.layers  # cache bytes of one position
    rd = B * ((Nq + Lt) * row + 4 * ll.vocab + 8 * Lt)
    moved = rd * (1 + n)  # read once, written n times
    fmed = sorted(fan_ms)[len(fan_ms) // 2]
    print(json.dumps({
        "workload": f"generate_batch: {B} prompts x {n} continuations, prompt {Nq}+{Lt} tokens (ragged), {args.new} new tokens, "
                    f"{'greedy' if args.greedy else 'sampling'}, {'eager' if args.no_graph else 'hipGraph replay'}, "
                    f"decode_weights={args.decode_weights}, kv_cache={args.kv_cache}; {args.reps} alternating pairs",
        "a_num_return_sequences_ms": stat(times["a"]), "b_repeated_prompts_ms": stat(times["b"]),
        "a_over_b_median": round(stat(times["a"])["median"] / stat(times["b"])["median"], 4),
        "fanout_ms": dict(median=round(fmed, 4), min=round(min(fan_ms), 4), max=round(max(fan_ms), 4)),
        "fanout_bytes_read": rd, "fanout_bytes_moved": moved, "fanout_TBps": round(moved / (fmed * 1e-3) / 1e12, 3),
        "fanout_frac_of_6.29TBps_copy": round(moved / (fmed * 1e-3) / 6.29e12, 3),
        "finite": bool(((out >= 0) & (out < ll.vocab)).all().item())}))


def share_prefix_ab(n):
    """(a) num_return_sequences = n: every decode row owns a copy of its prompt's cache; (c) the same call with share_prefix=True.
    Each timed call is a whole generation ending in a device synchronise.  Then one layer's decode attention on its own, device
    events around single launches: tcavt_attn_decode on (a)'s cache, tcavt_attn_decode_shared on (c)'s, at the last step's positions."""
    from tcavt_amd import generation, ops

    def arm(which, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=new, num_return_sequences=n, share_prefix=which == "c", **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for which in "ac":  # packed weights, workspaces, every kernel form, the clocks
        arm(which, 4)
        arm(which, args.new)
    times, outs = {"a": [], "c": []}, {}
    for _ in range(args.reps):
        for which in "ac":
            t, outs[which] = arm(which, args.new)
            times[which].append(t * 1e3)
    m.mllm.check_flags()
    stat = lambda v: dict(median=round(sorted(v)[len(v) // 2], 2), min=round(min(v), 2), max=round(max(v), 2))
    sa, sc = stat(times["a"]), stat(times["c"])
    LW, ws = m.mllm.llama_wrapper, m.mllm._ws
    ll, Nq, Lt, B, N = LW.shape, cfg.q_num_query_tokens, args.text_len, args.batch, args.new
    R, nq, nkv, st = B * n, ll.n_q_heads, ll.n_kv_heads, LW.storage
    w = nkv * ll.head_dim
    kc, vc = generation.cache_buffers(ws, "gen", LW, "fp16", R, Nq + Lt + N, dev)
    pk, pv = generation.cache_buffers(ws, "gen.src", LW, "fp16", B, Nq + Lt, dev)
    sk, sv = generation.cache_buffers(ws, "gen.sfx", LW, "fp16", R, max(N - 1, 1), dev)
    kv_len = ws.get("gen.src.kvlen", (B,), torch.int32, dev)
    pos = (kv_len.repeat_interleave(n) + (N - 2)).to(torch.int32).contiguous()  # the last decode step
    qkv = (torch.randn(R, (nq + 2 * nkv) * ll.head_dim, device=dev) * 0.5).to(st)
    layout = 1 if R <= 32 and (nq * 64) % 256 == 0 else 0
    att = torch.zeros(32 if layout else R, nq * ll.head_dim, dtype=st, device=dev)
    scale = ll.head_dim ** -0.5
    launches = {"unshared": lambda: ops.attn_decode(qkv, kc[0], vc[0], pos, att, R, nq, nkv, Nq + Lt + N, scale, out_layout=layout),
                "shared": lambda: ops.attn_decode_shared(qkv, pk[0], pv[0], kv_len, sk[0], sv[0], pos, att, B, n, nq, nkv, Nq + Lt,
                                                         max(N - 1, 1), scale, out_layout=layout)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    attn = {}
    for name, fn in launches.items():
        for _ in range(5):
            fn()
        ms = []
        for _ in range(50):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        attn[name] = sorted(ms)
    plen = kv_len.cpu().long()
    row = 2 * w * 2  # bytes of one cached position of one layer: keys + values
    by = {"unshared": int((plen.repeat_interleave(n) + N - 1).sum()) * row, "shared": (int(plen.sum()) + R * (N - 1)) * row}
    rep = lambda name: dict(median_us=round(attn[name][25] * 1e3, 2), min_us=round(attn[name][0] * 1e3, 2), max_us=round(attn[name][-1] * 1e3, 2),
                            cache_bytes=by[name], TBps=round(by[name] / (attn[name][25] * 1e-3) / 1e12, 3))
    spread_a = round(sa["max"] - sa["min"], 2)
    print(json.dumps({
        "workload": f"generate_batch: {B} prompts x {n} continuations, prompt {Nq}+{Lt} tokens (ragged), {N} new tokens, "
                    f"{'greedy' if args.greedy else 'sampling'}, {'eager' if args.no_graph else 'hipGraph replay'}, "
                    f"decode_weights={args.decode_weights}; {args.reps} alternating pairs",
        "a_num_return_sequences_ms": sa, "c_share_prefix_ms": sc, "c_over_a_median": round(sc["median"] / sa["median"], 4),
        "c_minus_a_median_ms": round(sc["median"] - sa["median"], 2), "a_spread_ms": spread_a,
        "c_not_slower_than_a_by_more_than_a_spread": bool(sc["median"] - sa["median"] <= spread_a),
        "per_step_gain_ms": round((sa["median"] - sc["median"]) / max(N - 1, 1), 4),
        "attention_one_layer_last_step": {k: rep(k) for k in launches},
        "rows_equal_between_arms": int((outs["a"] == outs["c"]).all(1).sum().item()), "rows": R,
        "finite": bool(((outs["c"] >= 0) & (outs["c"] < ll.vocab)).all().item())}))


def logprobs_ab():
    """Arm "off": the call as it is; arm "on": the same call with return_logprobs=True.  A timed call is a whole generation ending
    in a device synchronise; ms per decode step = (time of args.new tokens - time of 1 token) / (args.new - 1), per pair."""
    def arm(flag, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=new, return_logprobs=flag, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    for flag in (False, True):  # packed weights, workspaces, every kernel form, the clocks
        arm(flag, 4)
        arm(flag, args.new)
    step, first, last = {False: [], True: []}, {False: [], True: []}, {}
    for _ in range(args.reps):
        for flag in (False, True):
            t1, _ = arm(flag, 1)
            tn, last[flag] = arm(flag, args.new)
            step[flag].append((tn - t1) / max(args.new - 1, 1) * 1e3)
            first[flag].append(t1 * 1e3)
    m.mllm.check_flags()
    stat = lambda v: dict(median=round(sorted(v)[len(v) // 2], 4), min=round(min(v), 4), max=round(max(v), 4))
    off, on = stat(step[False]), stat(step[True])
    out, info = last[True]
    ll = cfg.llama
    print(json.dumps({
        "workload": f"generate_batch: B={args.batch}, prompt {cfg.q_num_query_tokens}+{args.text_len} tokens (ragged), {args.new} new tokens, "
                    f"{'greedy' if args.greedy else 'sampling'}, {'eager' if args.no_graph else 'hipGraph replay'}, "
                    f"decode_weights={args.decode_weights}, kv_cache={args.kv_cache}; {args.reps} alternating pairs",
        "off_decode_ms_per_step": off, "on_decode_ms_per_step": on,
        "on_minus_off_us_per_step": round((on["median"] - off["median"]) * 1e3, 2), "off_spread_us": round((off["max"] - off["min"]) * 1e3, 2),
        "on_over_off_median": round(on["median"] / off["median"], 4),
        "off_prefill_plus_first_token_ms": stat(first[False]), "on_prefill_plus_first_token_ms": stat(first[True]),
        "logits_bytes_read_again_per_step": 4 * ll.vocab * args.batch,
        "tokens_equal_between_arms": bool(torch.equal(out, last[False])),
        "n_scored_all_new": bool((info["n_scored"] == args.new).all().item()),
        "mean_logprob_per_token": round(float((info["sum_logprob"] / info["n_scored"]).mean()), 4),
        "finite": bool(torch.isfinite(info["token_logprobs"]).all().item() and ((out >= 0) & (out < ll.vocab)).all().item())}))


def top_logprobs_ab(ks):
    """Arm 0: return_logprobs=True; arm k: the same call with top_logprobs=k.  A timed call is a whole generation ending in a device
    synchronise; ms per decode step = (time of args.new tokens - time of 1 token) / (args.new - 1), per round of all arms."""
    arms = [None] + list(ks)

    def arm(k, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=new, return_logprobs=True, top_logprobs=k, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    for k in arms:  # packed weights, workspaces, every kernel form, the clocks
        arm(k, 4)
        arm(k, args.new)
    step, first, last = {k: [] for k in arms}, {k: [] for k in arms}, {}
    for _ in range(args.reps):
        for k in arms:
            t1, _ = arm(k, 1)
            tn, last[k] = arm(k, args.new)
            step[k].append((tn - t1) / max(args.new - 1, 1) * 1e3)
            first[k].append(t1 * 1e3)
    m.mllm.check_flags()
    stat = lambda v: dict(median=round(sorted(v)[len(v) // 2], 4), min=round(min(v), 4), max=round(max(v), 4))
    base = stat(step[None])
    ll = cfg.llama
    rec = {"workload": f"generate_batch: B={args.batch}, prompt {cfg.q_num_query_tokens}+{args.text_len} tokens (ragged), {args.new} new "
                       f"tokens, {'greedy' if args.greedy else 'sampling'}, {'eager' if args.no_graph else 'hipGraph replay'}, "
                       f"decode_weights={args.decode_weights}, kv_cache={args.kv_cache}; {args.reps} alternating rounds",
           "logprobs_decode_ms_per_step": base, "logprobs_spread_us": round((base["max"] - base["min"]) * 1e3, 2),
           "logprobs_prefill_plus_first_token_ms": stat(first[None]), "logits_bytes_read_again_per_step": 4 * ll.vocab * args.batch}
    out0, info0 = last[None]
    for k in ks:
        on = stat(step[k])
        out, info = last[k]
        ids, lps = info["top_token_ids"], info["top_token_logprobs"]
        rec[f"top{k}"] = {
            "decode_ms_per_step": on, "minus_logprobs_us_per_step": round((on["median"] - base["median"]) * 1e3, 2),
            "over_logprobs_median": round(on["median"] / base["median"], 4), "prefill_plus_first_token_ms": stat(first[k]),
            "tokens_and_logprobs_equal_to_arm_0": bool(torch.equal(out, out0) and torch.equal(info["token_logprobs"], info0["token_logprobs"])),
            "lists_sorted_and_in_range": bool((lps[..., :-1] >= lps[..., 1:]).all().item() and ((ids >= 0) & (ids < ll.vocab)).all().item()),
            "emitted_token_listed_frac": round(float((ids == out.cpu()[..., None]).any(-1).float().mean()), 4)}
    print(json.dumps(rec))
    if args.pool_slots:
        import numpy as np

        R = 256
        b = synth.make_batch(cfg, R, text_len=args.text_len, seed=3, ragged=True, min_text=min(128, args.text_len // 2))
        q = {k_: torch.from_numpy(v).to(dev) for k_, v in b.items()}
        budgets = np.random.default_rng(7).integers(16, 129, size=R).tolist()  # the list of tools/bench_generate_pool.py
        for S in args.pool_slots:
            pool = {}
            for rnd in range(2):  # the first round is the warm-up of every form at this pool size
                for k in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m.mllm.generate_pool(q["vision_emb"], q["input_ids"], q["attention_mask"], max_new_tokens=budgets, slots=S,
                                         do_sample=not args.greedy, return_logprobs=True, top_logprobs=k)
                    torch.cuda.synchronize()
                    pool[k] = round(time.perf_counter() - t0, 4)
            m.mllm.check_flags()
            print(json.dumps({"workload": f"generate_pool: {R} requests, budgets 16..128 ({sum(budgets)} tokens), {S} slots, admit_group=1, "
                                          "poll_every=1; one timed run per arm after one warm-up run",
                              "wall_s": {("logprobs" if k is None else f"top{k}"): v for k, v in pool.items()},
                              "steps": m.mllm.pool_stats["steps"]}))


if args.top_logprobs:
    top_logprobs_ab(args.top_logprobs)
    sys.exit(0)

if args.logprobs:
    logprobs_ab()
    sys.exit(0)

if args.num_return_sequences > 1 or args.share_prefix:
    if args.share_prefix:
        share_prefix_ab(args.num_return_sequences)
    else:
        nsamples_ab(args.num_return_sequences)
    sys.exit(0)

run(4)  # packed weights, workspaces
run(args.new)  # clocks, graph capture path
reps = []
for _ in range(5):  # (a decode step is latency-bound and sensitive to the clock state: median of five)
    t1, _ = run(1)          # prefill + first token
    tn, out = run(args.new)  # prefill + args.new tokens
    reps.append(((tn - t1) / max(args.new - 1, 1), t1))
reps.sort()
per_tok, t1 = reps[len(reps) // 2]
ll = cfg.llama
wbytes = 2 * (ll.layers * (ll.hidden * (ll.n_q_heads + 2 * ll.n_kv_heads) * ll.head_dim + ll.n_q_heads * ll.head_dim * ll.hidden
                           + 3 * ll.hidden * ll.inter) + ll.vocab * ll.hidden)
if args.decode_weights == "fp8":  # one byte per weight + one fp32 scale per row
    wbytes = wbytes // 2 + 4 * (ll.layers * ((ll.n_q_heads + 2 * ll.n_kv_heads) * ll.head_dim + 2 * ll.hidden + 2 * ll.inter) + ll.vocab)
# cache bytes a step reads at the mean prompt length (keys + values of every layer; KV8: 64 codes + 2 scale bytes per row and kv head)
mean_len = cfg.q_num_query_tokens + float(g["attention_mask"].sum(1).float().mean()) + args.new / 2
kvbytes = int(2 * ll.layers * args.batch * mean_len * ll.n_kv_heads * (66 if args.kv_cache == "fp8" else 2 * ll.head_dim))
print(json.dumps({
    "decode_weights": args.decode_weights, "kv_cache": args.kv_cache, "kv_cache_bytes_per_step": kvbytes,
    "workload": f"generate_batch: B={args.batch}, prompt {cfg.q_num_query_tokens}+{args.text_len} tokens (ragged), {args.new} new tokens, "
                f"{'greedy' if args.greedy else 'sampling T=0.9 top-k 40 top-p 0.9 rep 1.2 no-repeat-3'}, "
                f"{'eager launches' if args.no_graph else 'hipGraph replay of the decode step'}",
    "prefill_plus_first_token_ms": round(t1 * 1e3, 2), "decode_ms_per_step": round(per_tok * 1e3, 3),
    "decode_ms_per_step_min_max_of_5": [round(reps[0][0] * 1e3, 3), round(reps[-1][0] * 1e3, 3)],
    "decode_tokens_per_s": round(args.batch / per_tok, 1),
    "weight_bytes_per_step": wbytes, "weight_stream_GBps": round(wbytes / per_tok / 1e9, 1),
    "hbm_frac_of_8TBps": round(wbytes / per_tok / 8e12, 4), "finite": bool(((out >= 0) & (out < ll.vocab)).all().item())}))
