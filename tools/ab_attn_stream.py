"""A/B of the decoder attention beyond 544 rows (B=8, 32 query / 8 key-value heads, fp16, ragged kv_len).

forward   the streaming kernel (tcavt_attn_causal_gqa_stream) at L in {544, 640, 1040} and the resident kernel
          (tcavt_attn_causal_gqa_lse) at L = 544, all alternating in one process.  Yardstick: the resident kernel at 544 scaled
          by the attended (query, key) pairs, L (L + 1) / 2.
backward  tcavt_attn_bwd_stream against the tiled path behind TCAVT_ATTN_BWD_NO_STREAM (attn_bwd_scores + attn_bwd_dkv +
          rope_bwd_pack through an fp32 buffer) at the same lengths (tcavt_attn_bwd_long is what serves 544; the stream entry
          runs the same kernels there).
--step    one stage-1 step (MllmTrainer.step, Llama-3.2-1B shape) at B = 8, Lt = 1024: ms per step and peak memory.

Every call is timed with HIP events; the median of 15 runs after 3 warm-ups, us per call.
Usage: python tools/ab_attn_stream.py [--step] [--out FILE] [L ...]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tcavt_amd import capi, ops
from tcavt_amd.config import LlamaShape
from tcavt_amd.rope import rope_tables

RUNS, WARM = 15, 3
B, nq, nkv, dt = 8, 32, 8, torch.float16
LINES = []


def log(s):
    print(s, flush=True)
    LINES.append(s)


def _interleaved(forms):
    times = {k: [] for k in forms}
    for it in range(WARM + RUNS):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}


def _inputs(L, dev):
    ncols, M = (nq + 2 * nkv) * 64, B * L
    g = torch.Generator(device="cpu").manual_seed(L)
    qkv = torch.zeros(M + 64, ncols, dtype=dt, device=dev)
    qkv[:M] = torch.randn(M, ncols, generator=g).to(dt).to(dev)
    dO = torch.randn(M, nq * 64, generator=g).to(dt).to(dev)
    kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
    kv_len[1::3] = max(1, L - 37)
    kv_len[2::3] = max(1, (2 * L) // 3)
    return qkv, dO, kv_len


def forward(Ls, dev):
    log(f"forward: B={B} nq={nq} nkv={nkv} {str(dt)[6:]}, kv_len ragged (L, L - 37, 2 L / 3); median of {RUNS} after {WARM}, us per call")
    data, forms, outs = {}, {}, {}
    for L in sorted(set(Ls) | {544}):
        qkv, _, kv_len = _inputs(L, dev)
        M = B * L
        out = torch.empty(M, nq * 64, dtype=dt, device=dev)
        lse = torch.empty(B * nq * L, device=dev)
        data[L] = (qkv, kv_len, out, lse)
        forms[f"stream {L}"] = (lambda L=L: ops.attn_causal_gqa_stream(data[L][0][:B * L], data[L][2], data[L][1], B, L, nq, nkv, 0.125,
                                                                       lse=data[L][3]))
    out_r = torch.empty(B * 544, nq * 64, dtype=dt, device=dev)
    forms["resident 544"] = lambda: ops.attn_causal_gqa(data[544][0][:B * 544], out_r, data[544][1], B, 544, nq, nkv, 0.125, lse=data[544][3])
    med = _interleaved(forms)
    base = med["resident 544"]
    log(f"{'form':>14} {'us':>10} {'pairs / pairs(544)':>20} {'time / resident(544)':>22} {'time / yardstick':>18}")
    log(f"{'resident 544':>14} {base:10.1f} {1.0:20.2f} {1.0:22.2f} {1.0:18.2f}")
    for L in sorted(data):
        t = med[f"stream {L}"]
        pairs = L * (L + 1) / (544 * 545)
        log(f"{'stream ' + str(L):>14} {t:10.1f} {pairs:20.2f} {t / base:22.2f} {t / (base * pairs):18.2f}")
    forms["stream 544"]()
    a = data[544][2].float().clone()
    forms["resident 544"]()
    torch.cuda.synchronize()
    log(f"agreement at 544, stream against resident: rel {((a - out_r.float()).norm() / out_r.float().norm()).item():.2e}")


def backward(Ls, dev):
    log(f"backward: same shapes; the chunked two-launch form (tcavt_attn_bwd_stream) against the tiled path, us per call")
    log(f"{'T':>5} {'tiled':>10} {'chunked':>10} {'tiled/chunked':>14}   agreement (rel)")
    for T in Ls:
        ncols, M, Tp = (nq + 2 * nkv) * 64, B * T, (T + 63) // 64 * 64
        qkv, dO, kv_len = _inputs(T, dev)
        cos, sin = (t.to(dev) for t in rope_tables(LlamaShape(), T))
        att = torch.empty(M, nq * 64, dtype=dt, device=dev)
        lse = torch.empty(B * nq * T, device=dev)
        ops.attn_causal_gqa_stream(qkv[:M], att, kv_len, B, T, nq, nkv, 0.125, lse=lse)
        stats = torch.empty(B * nq * T, 4, device=dev)
        g32 = torch.empty(M, ncols, device=dev)
        out = {"tiled": torch.empty(M, ncols, dtype=dt, device=dev), "chunked": torch.empty(M, ncols, dtype=dt, device=dev)}

        def tiled():
            ops.attn_bwd_scores(qkv, dO, None, None, None, kv_len, B, T, Tp, nq, nkv, 0.125, dQ=g32, stats=stats, lse=lse, att=att)
            ops.attn_bwd_dkv(qkv, dO, stats, g32, kv_len, B, T, Tp, nq, nkv, 0.125)
            ops.rope_bwd_pack(g32, out["tiled"], cos, sin, (nq + nkv) * 64, T)

        def chunked():
            ops.attn_bwd_stream(qkv, dO, att, lse, out["chunked"], stats, cos, sin, kv_len, B, T, nq, nkv, 0.125)

        med = _interleaved({"tiled": tiled, "chunked": chunked})
        rel = ((out["chunked"].float() - out["tiled"].float()).norm() / out["tiled"].float().norm()).item()
        log(f"{T:5d} {med['tiled']:10.1f} {med['chunked']:10.1f} {med['tiled'] / med['chunked']:14.2f}   {rel:.2e}")


def step(dev, Bs=8, text_len=1024):
    from tcavt_amd import config, model, synth, training
    from tcavt_amd.weights import make_weights

    cfg = config.llama32_1b()
    m = model.MultiModalTrajectoryModel.from_config(cfg).to(dev)
    m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev))
    m.eval()
    tr = training.MllmTrainer(m)
    b = synth.make_batch(cfg, Bs, text_len=text_len, seed=100, ragged=True, min_text=512)
    g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    args = (g["vision_emb"], g["input_ids"], g["attention_mask"], g["labels"])
    torch.cuda.reset_peak_memory_stats()
    losses = [float(tr.step(*args)) for _ in range(WARM)]
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.step(*args)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    tr.check_flags()
    L = cfg.q_num_query_tokens + text_len
    log(f"stage-1 step: MllmTrainer.step, Llama-3.2-1B shape, B {Bs}, Lt {text_len} (L {L}, M {Bs * L}), {int(tr.last.n_tokens)} labelled rows")
    log(f"step  median {statistics.median(ms):8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, n {len(ms)});  peak allocated "
        f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    log(f"loss over the warm-up steps on one batch: {', '.join(f'{v:.4f}' for v in losses)}; optimizer (applied, skipped) = {tr.optimizer_counters()}")


def main():
    argv = sys.argv[1:]
    do_step = "--step" in argv
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    Ls = [int(a) for i, a in enumerate(argv) if a.isdigit() and (i == 0 or argv[i - 1] != "--out")] or [544, 640, 1040]
    capi.init(0)
    dev = torch.device("cuda:0")
    log(f"tools/ab_attn_stream.py: {torch.cuda.get_device_name(0)}")
    forward(Ls, dev)
    backward(Ls, dev)
    if do_step:
        step(dev)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
