"""LM loss on labels: the fused kernels (ops.lm_loss_forward / lm_loss_backward) against the composed path a user would have
to write without them, at the bench shape (B 32, L 256, H 2048, V 128256), in ONE process, alternating the two paths.

Composed path: ops.gemm_bf16 into fp32 logits [B * L, V], torch's cross-entropy and its autograd, a cast of the logits'
gradient to bf16 (the scaled gradient leaves fp16's normal range), ops.gemm_bf16 with the transposed table.

Two label sets: tcavt_amd.synth's (full rows: 7680 labelled rows of 8192) and one with 1/8 of the rows labelled.
Per set: time of each path (HIP events after a warm-up; median and spread over the repetitions), peak allocated memory of
each path, model FLOP/s of the fused forward and backward over their own time (2 N V H and 4 N V H for N labelled rows).
--trainer adds the MllmTrainer step at the Llama-3.2-1B shape.
--eval runs the evaluation leg INSTEAD: ops.lm_eval (loss + arg-max + per-sample sums) and ops.lm_loss_forward alternate with
the composed evaluation (ops.gemm_bf16 -> fp32 logits -> torch.argmax + cross-entropy); time and peak memory of each.  Usage:
    python tools/bench_lm_loss.py [--reps 10] [--warmup 3] [--trainer] [--out profiles/lm_loss.txt]
    python tools/bench_lm_loss.py --eval [--out profiles/lm_eval.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, BF16 = torch.float32, torch.bfloat16


def row_targets(labels, Nq):
    """[B * L] target of every row (-100: unlabelled): row (b, p) predicts fused_labels[b, p + 1]."""
    B, Lt = labels.shape
    fused = torch.cat([torch.full((B, Nq), -100, dtype=labels.dtype, device=labels.device), labels], 1)
    tgt = torch.full_like(fused, -100)
    tgt[:, :-1] = fused[:, 1:]
    return tgt.reshape(-1)


def composed_forward_backward(h16, table, table_t_bf16, targets):
    """-> (loss fp32 scalar, g_final bf16 [rows, H]) through the stored fp32 logits"""
    from tcavt_amd import ops

    logits = ops.gemm_bf16(h16, table, out_dtype=F32).requires_grad_(True)
    with torch.enable_grad():
        loss = torch.nn.functional.cross_entropy(logits, targets, ignore_index=-100)
    loss.backward()
    d16 = logits.grad.to(BF16)
    return loss.detach(), ops.gemm_bf16(d16, table_t_bf16)


class Fused:
    def __init__(self, h16, table, labels, Nq, B, L):
        from tcavt_amd import ops

        dev = h16.device
        V, H = table.shape
        self.a = (h16, table, labels, Nq, B, L)
        self.table_t = ops.lm_table_t(table)
        self.ws = torch.empty(ops.lm_loss_workspace_bytes(B * L, V, H), dtype=torch.uint8, device=dev)
        self.loss, self.count = torch.empty(1, dtype=F32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        self.lse = torch.empty(B * L, dtype=F32, device=dev)
        self.g = torch.empty(B * L, H, dtype=BF16, device=dev)

    def forward(self):
        from tcavt_amd import ops

        h16, table, labels, Nq, B, L = self.a
        return ops.lm_loss_forward(h16, table, labels, Nq, B, L, loss=self.loss, count=self.count, lse=self.lse, workspace=self.ws)

    def backward(self):
        from tcavt_amd import ops

        h16, table, labels, Nq, B, L = self.a
        return ops.lm_loss_backward(h16, table, self.table_t, labels, Nq, B, L, lse=self.lse, count=self.count, g_out=self.g,
                                    workspace=self.ws)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return e0, e1, out


def _stats(ms):
    return f"median {statistics.median(ms):8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, n {len(ms)})"


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def run_label_set(name, h16, table, table_t_bf16, labels, Nq, B, L, reps, warmup, log):
    V, H = table.shape
    fused = Fused(h16, table, labels, Nq, B, L)
    targets = row_targets(labels, Nq)
    N = int((targets != -100).sum())
    for _ in range(warmup):
        fused.forward(), fused.backward()
        composed_forward_backward(h16, table, table_t_bf16, targets)
    torch.cuda.synchronize()
    ev = {"fused fwd": [], "fused bwd": [], "composed": []}
    for _ in range(reps):  # alternate the paths inside one process
        ev["fused fwd"].append(_timed(fused.forward)[:2])
        ev["fused bwd"].append(_timed(fused.backward)[:2])
        ev["composed"].append(_timed(lambda: composed_forward_backward(h16, table, table_t_bf16, targets))[:2])
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    both = [a + b for a, b in zip(ms["fused fwd"], ms["fused bwd"])]
    loss_c, g_c = composed_forward_backward(h16, table, table_t_bf16, targets)
    fused.forward(), fused.backward()
    torch.cuda.synchronize()
    rel_loss = abs(float(fused.loss) - float(loss_c)) / abs(float(loss_c))
    rel_g = float((fused.g.double() - g_c.double()).norm() / g_c.double().norm())
    fused_ws = fused.ws.numel() + fused.g.numel() * 2 + fused.lse.numel() * 4
    peak_c = _peak(lambda: composed_forward_backward(h16, table, table_t_bf16, targets))
    peak_f = _peak(lambda: (fused.forward(), fused.backward()))
    log(f"--- labels: {name}: {N} labelled rows of {B * L} (B {B}, L {L}, H {H}, V {V}, operands {str(h16.dtype)[6:]})")
    log(f"fused forward            {_stats(ms['fused fwd'])}   {2.0 * N * V * H / statistics.median(ms['fused fwd']) / 1e9:7.1f} model TFLOP/s")
    log(f"fused backward           {_stats(ms['fused bwd'])}   {4.0 * N * V * H / statistics.median(ms['fused bwd']) / 1e9:7.1f} model TFLOP/s")
    log(f"fused forward + backward {_stats(both)}")
    log(f"composed (fp32 logits)   {_stats(ms['composed'])}")
    log(f"fused / composed time    {statistics.median(both) / statistics.median(ms['composed']):.3f}")
    log(f"memory: fused path holds {fused_ws / 2 ** 20:.1f} MiB (workspace {fused.ws.numel() / 2 ** 20:.1f} + g_final + lse; its calls allocate "
        f"{peak_f / 2 ** 20:.1f} MiB more); composed path peaks at {peak_c / 2 ** 20:.1f} MiB; table transpose (either path) "
        f"{fused.table_t.numel() * 2 / 2 ** 20:.1f} MiB")
    log(f"agreement: loss fused {float(fused.loss):.6f} vs composed {float(loss_c):.6f} (rel {rel_loss:.2e}); g_final rel {rel_g:.2e}")
    return {"N": N, "ms": ms}


def composed_eval(h16, table, targets):
    """-> (loss, pred [rows], correct) through the stored fp32 logits"""
    from tcavt_amd import ops

    logits = ops.gemm_bf16(h16, table, out_dtype=F32)
    pred = logits.argmax(dim=1)
    loss = torch.nn.functional.cross_entropy(logits, targets, ignore_index=-100)
    return loss, pred, ((pred == targets) & (targets != -100)).sum()


def run_eval(name, h16, table, labels, Nq, B, L, reps, warmup, log):
    from tcavt_amd import ops

    dev = h16.device
    V, H = table.shape
    fused = Fused(h16, table, labels, Nq, B, L)
    targets = row_targets(labels, Nq)
    N = int((targets != -100).sum())
    ws = torch.empty(ops.lm_eval_workspace_bytes(B * L, V, H), dtype=torch.uint8, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    loss, count, correct, pred, lse = torch.empty(1, dtype=F32, device=dev), i32(1), i32(1), i32(B * L), torch.empty(B * L, dtype=F32, device=dev)
    row_loss, nll, stok, scor = torch.empty(B * L, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev), i32(B), i32(B)

    def ev():
        return ops.lm_eval(h16, table, labels, Nq, B, L, loss=loss, count=count, lse=lse, pred=pred, workspace=ws, row_loss=row_loss,
                           correct=correct, sample_tokens=stok, sample_correct=scor, sample_nll=nll)

    for _ in range(warmup):
        ev(), fused.forward(), composed_eval(h16, table, targets)
    torch.cuda.synchronize()
    evs = {"eval": [], "forward": [], "composed": []}
    for _ in range(reps):  # alternate the paths inside one process
        evs["eval"].append(_timed(ev)[:2])
        evs["forward"].append(_timed(fused.forward)[:2])
        evs["composed"].append(_timed(lambda: composed_eval(h16, table, targets))[:2])
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in evs.items()}
    loss_c, pred_c, cor_c = composed_eval(h16, table, targets)
    ev(), fused.forward()
    torch.cuda.synchronize()
    lab = targets != -100
    agree = int((pred.long()[lab] == pred_c[lab]).sum())
    peak_c = _peak(lambda: composed_eval(h16, table, targets))
    peak_e = _peak(ev)
    med = {k: statistics.median(v) for k, v in ms.items()}
    log(f"--- eval, labels: {name}: {N} labelled rows of {B * L} (B {B}, L {L}, H {H}, V {V}, operands {str(h16.dtype)[6:]})")
    log(f"tcavt_lm_eval            {_stats(ms['eval'])}   {2.0 * N * V * H / med['eval'] / 1e9:7.1f} model TFLOP/s")
    log(f"tcavt_lm_loss_forward    {_stats(ms['forward'])}   {2.0 * N * V * H / med['forward'] / 1e9:7.1f} model TFLOP/s")
    log(f"composed (fp32 logits)   {_stats(ms['composed'])}")
    log(f"eval / forward time      {med['eval'] / med['forward']:.3f}     eval / composed time {med['eval'] / med['composed']:.3f}")
    log(f"memory: eval workspace {ws.numel() / 2 ** 20:.1f} MiB (loss workspace {fused.ws.numel() / 2 ** 20:.1f} MiB; the call allocates "
        f"{peak_e / 2 ** 20:.1f} MiB more); composed path peaks at {peak_c / 2 ** 20:.1f} MiB")
    log(f"agreement: loss bits equal to the forward's: {bool(torch.equal(loss, fused.loss))}; loss vs composed rel "
        f"{abs(float(loss) - float(loss_c)) / abs(float(loss_c)):.2e}; arg-max equal on {agree} of {N} rows; correct {int(correct)} vs {int(cor_c)}")


def run_trainer(reps, warmup, log, B=32, text_len=240):
    from tcavt_amd import config, model, synth, training
    from tcavt_amd.weights import make_weights

    dev = torch.device("cuda")
    cfg = config.llama32_1b()
    m = model.MultiModalTrajectoryModel.from_config(cfg).to(dev)
    m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev))
    m.eval()
    tr = training.MllmTrainer(m)
    b = synth.make_batch(cfg, B, text_len=text_len, seed=100, ragged=True, min_text=128)
    g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    args = (g["vision_emb"], g["input_ids"], g["attention_mask"], g["labels"])
    losses = [float(tr.step(*args)) for _ in range(warmup)]
    torch.cuda.synchronize()
    ev = [_timed(lambda: tr.step(*args))[:2] for _ in range(reps)]
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b_) for a, b_ in ev]
    tr.check_flags()
    L = cfg.q_num_query_tokens + text_len
    log(f"--- MllmTrainer.step at the Llama-3.2-1B shape, B {B}, L {L}, {int(tr.last.n_tokens)} labelled rows, eval arithmetic")
    log(f"step                     {_stats(ms)}   (trajectory-loss LoRA step of the same shape: 36.9 ms, DESIGN.md section 8)")
    log(f"loss over the warm-up steps on one batch: {', '.join(f'{v:.4f}' for v in losses)}; optimizer (applied, skipped) = {tr.optimizer_counters()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--eval", action="store_true", help="the evaluation leg: lm_eval against lm_loss_forward and the composed arg-max")
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tcavt_amd import capi, config, synth

    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    capi.init(0)
    dev = torch.device("cuda")
    dt = getattr(torch, a.dtype)
    cfg = config.llama32_1b()
    B, Lt, Nq, H, V = 32, 240, cfg.q_num_query_tokens, cfg.llama.hidden, cfg.llama.vocab
    L = Nq + Lt
    g = torch.Generator(device=dev).manual_seed(0)
    table = (torch.randn(V, H, generator=g, device=dev) * 0.02).to(dt)
    h16 = torch.randn(B * L, H, generator=g, device=dev).to(dt)
    table_t_bf16 = table.t().contiguous().to(BF16)
    labels = torch.from_numpy(synth.make_batch(cfg, B, text_len=Lt, seed=100, ragged=False)["labels"]).to(dev)  # every text row labelled
    log(f"tools/bench_lm_loss.py{' --eval' if a.eval else ''} --reps {a.reps} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}")
    if a.eval:
        run_eval("synth", h16, table, labels, Nq, B, L, a.reps, a.warmup, log)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    run_label_set("synth", h16, table, table_t_bf16, labels, Nq, B, L, a.reps, a.warmup, log)
    sparse = labels.clone()
    keep = torch.zeros_like(sparse, dtype=torch.bool)
    keep[:, ::8] = True
    sparse[~keep] = -100
    run_label_set("1/8 of the rows", h16, table, table_t_bf16, sparse, Nq, B, L, a.reps, a.warmup, log)
    del table, h16, table_t_bf16
    torch.cuda.empty_cache()
    if a.trainer:
        run_trainer(a.reps, a.warmup, log)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
