"""Beam search against the parent path it is built on, at the full model size (Llama-3.2-1B shape), one MI355X:
    python tools/bench_beams.py [--batch 4] [--beams 8] [--new 64] [--text-lens 240 1008] [--reps 7] [--out profiles/generate_beams.txt]
Arms, alternating a b a b ... in ONE process after both ran twice as warm-up; a timed call is a whole generation between two device
synchronisations (host clock):
  (a) generate_batch(num_return_sequences=beams, share_prefix=True, do_sample=True)  -- the shared-prompt-cache path
  (b) generate_batch(num_beams=beams, do_sample=False)                               -- the search on the same rows
Then the two new entries on their own (device events around single launches): tcavt_beam_select at batch * beams rows and
tcavt_beam_reorder with every row moved and all new - 1 suffix slots written, with the bytes it moves.  This is a new capability:
there is no pass mark, the numbers are reported as measured."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tcavt_amd import capi, config, model, ops, synth
from tcavt_amd.weights import make_weights

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--beams", type=int, default=8)
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--text-lens", type=int, nargs="+", default=[240, 1008])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--preset", default="llama32_1b")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "generate_beams.txt"))
args = ap.parse_args()
capi.init(0)
dev = torch.device("cuda:0")
cfg = config.PRESETS[args.preset]()
with torch.device(dev):
    m = model.MultiModalTrajectoryModel.from_config(cfg)
m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
B, n, N = args.batch, args.beams, args.new
R, V, ll = B * n, cfg.llama.vocab, cfg.llama
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def stats(ts, scale=1e3, nd=2):
    return dict(median=round(statistics.median(ts) * scale, nd), min=round(min(ts) * scale, nd), max=round(max(ts) * scale, nd))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def event_times(fn, before=lambda: None, reps=50, warm=5):
    """Device time of single launches of fn (seconds); ``before`` runs outside the timed window."""
    ts = []
    for i in range(warm + reps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    return ts


def kernels():
    """The two entries on a state of their own: every beam live at step new / 2 with random scores; the reorder at the last step with
    every row moved (a rotation of the beams) and new - 1 suffix slots written."""
    g = torch.Generator(device=dev).manual_seed(7)
    Lt, s_sel, cap = 16, N // 2, 16 + N
    logits = 3.0 * torch.randn(R, V, generator=g, device=dev)
    history = torch.randint(0, V, (R, cap), generator=g, device=dev, dtype=I64)
    z = lambda *sh, dt=I32: torch.zeros(*sh, dtype=dt, device=dev)  # noqa: E731
    hist_len, pos, step = torch.full((R,), Lt + s_sel, dtype=I32, device=dev), torch.full((R,), 16 + Lt + s_sel - 1, dtype=I32, device=dev), \
        torch.full((B,), s_sel, dtype=I32, device=dev)
    run_score, live = -torch.rand(R, generator=g, device=dev), torch.ones(R, dtype=I32, device=dev)
    fin_tokens, fin_score, fin_flag, fin_len = z(B, n, N, dt=I64), z(B, n, dt=F32), z(B, n), z(B, n)
    unsat, done, cur, finished = torch.ones(B, dtype=I32, device=dev), z(B), z(R, dt=I64), z(R)
    prefix_len, parent, plan = torch.full((B,), 16 + Lt, dtype=I32, device=dev), z(R), z(B, 4)
    len_pow = torch.arange(1, N + 1, device=dev, dtype=F32)
    ws = torch.empty(ops.beam_workspace_bytes(R), dtype=torch.uint8, device=dev)
    sel = ops.beam_args(logits, n, N, history, hist_len, run_score, live, fin_tokens, fin_score, fin_flag, fin_len, unsat, done, cur, pos,
                        finished, step, prefix_len, len_pow, parent, plan, ws, V - 1, 0, 1.2, 3, False)
    score0 = run_score.clone()

    def rearm():
        done.zero_(), fin_flag.zero_(), unsat.fill_(1), live.fill_(1), run_score.copy_(score0)

    t_sel = event_times(lambda: ops.beam_select(sel), rearm)
    sfx = N - 1
    sk = torch.randn(ll.layers, R, sfx, ll.n_kv_heads * 64, generator=g, device=dev).to(torch.float16)
    sv = torch.randn(ll.layers, R, sfx, ll.n_kv_heads * 64, generator=g, device=dev).to(torch.float16)
    reo = ops.beam_reorder_args(n, parent, plan, cur, history, hist_len, pos, step, sk, sv, ll.layers, ll.n_kv_heads)
    rot = (torch.arange(n, device=dev, dtype=I32) + 1) % n
    plan_full = torch.tensor([[N - 1, sfx, 1, Lt]] * B, dtype=I32, device=dev)

    def plant():
        parent.copy_(rot.repeat(B)), plan.copy_(plan_full), hist_len.fill_(Lt + N - 1), pos.fill_(16 + Lt + N - 2)

    t_reo = event_times(lambda: ops.beam_reorder(reo), plant)
    moved = 2 * R * sfx * ll.layers * 2 * ll.n_kv_heads * 128  # read + write: rows x slots x layers x (k, v) x row bytes
    return t_sel, t_reo, moved


lines, raw = [], []
lines += [f"generate_batch(num_beams={n}): beam search on the shared prompt cache, one MI355X",
          "=" * 88,
          f"tools/bench_beams.py --batch {B} --beams {n} --new {N} --text-lens {' '.join(map(str, args.text_lens))} --reps {args.reps}",
          f"Full model size ({args.preset}, synthetic weights and prompts, ragged prompt lengths), hipGraph replay of the decode step, fp16",
          "weights and cache.  Arms alternate a b a b ... in ONE process after both ran twice (4 and the full number of tokens) as warm-up;",
          "a timed call is a whole generation between two device synchronisations, host clock:",
          f"  (a) num_return_sequences={n}, share_prefix=True, do_sample=True (T 0.9, top-k 40, top-p 0.9, penalty 1.2, no-repeat 3-gram):",
          "      the parent path the search is built on -- decode_step_shared + the two-stage sampler per step",
          f"  (b) num_beams={n}, do_sample=False (penalty 1.2, no-repeat 3-gram, no EOS: all {N} tokens): decode_step_shared + tcavt_beam_select",
          "      + tcavt_beam_reorder per step, on the same rows",
          "A new capability: no pass mark, the numbers as measured.", ""]
for Lt in args.text_lens:
    b = synth.make_batch(cfg, B, text_len=Lt, seed=3, ragged=True, min_text=min(128, Lt // 2))
    g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    kw = dict(input_ids=g["input_ids"], attention_mask=g["attention_mask"], use_graph=True)

    def arm(which, new):
        if which == "a":
            return m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=new, num_return_sequences=n, share_prefix=True, do_sample=True, **kw)
        return m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=new, num_beams=n, do_sample=False, **kw)

    for new in (4, N):
        for which in "ab":
            timed(lambda: arm(which, new))
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(timed(lambda: arm("a", N))[0])
        tb.append(timed(lambda: arm("b", N))[0])
    m.mllm.check_flags()
    sa, sb = stats(ta), stats(tb)
    d = sb["median"] - sa["median"]
    rec = {"workload": f"{B} prompts x {n} rows, prompt 16+{Lt} tokens (ragged), {N} new tokens, hipGraph replay; {args.reps} alternating pairs",
           "a_share_prefix_sampling_ms": sa, "b_beam_search_ms": sb, "b_over_a_median": round(sb["median"] / sa["median"], 4),
           "b_minus_a_median_ms": round(d, 2), "per_step_ms": round(d / max(N - 1, 1), 4)}
    raw.append(rec)
    lines += [f"prompt 16 + {Lt} rows",
              f"  (a) median {sa['median']:.2f} ms   min {sa['min']:.2f}   max {sa['max']:.2f}",
              f"  (b) median {sb['median']:.2f} ms   min {sb['min']:.2f}   max {sb['max']:.2f}",
              f"  (b) / (a) = {rec['b_over_a_median']:.3f} : the search is {abs(d):.2f} ms {'SLOWER' if d > 0 else 'faster'} "
              f"({d / sa['median'] * 100:+.1f} %), {d / max(N - 1, 1) * 1e3:+.0f} us per decode step", ""]
t_sel, t_reo, moved = kernels()
ss, sr = stats(t_sel, 1e6, 1), stats(t_reo, 1e6, 1)
tbps = moved / statistics.median(t_reo) / 1e12
raw.append({"kernels": f"R = {R} rows, V = {V}, n = {n}; device events around single launches, 50 after 5 warm-up launches",
            "beam_select_us": ss, "beam_reorder_us": sr, "reorder_bytes_read_plus_written": moved, "reorder_TBps": round(tbps, 3)})
lines += [f"The two entries on their own (R = {R} rows, V = {V}; device events around single launches, 50 after 5 warm-up launches):",
          f"  tcavt_beam_select   median {ss['median']:.1f} us (min {ss['min']:.1f}, max {ss['max']:.1f}): three launches, every beam live, penalty 1.2, 3-gram ban",
          f"  tcavt_beam_reorder  median {sr['median']:.1f} us (min {sr['min']:.1f}, max {sr['max']:.1f}): every row moved, {N - 1} suffix slots, "
          f"{moved / 1e6:.1f} MB read + written: {tbps:.2f} TB/s", "", "Raw output lines"]
lines += [json.dumps(r) for r in raw]
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
