"""The reference's own training loop against training.Trainer, in one process, at bench.py's default configuration
(B = 32 samples, L = 16 query tokens + 240 text tokens, Llama-3.2-1B preset, train mode with dropout, fp16 storage).

    literal:  optimizer.zero_grad(); loss, _ = model(...); loss.backward(); optimizer.step(); loss.item()
              (scripts/train.py:1168-1183, torch.optim.AdamW(trainable, lr 5e-4, weight_decay 1e-4), MLLM frozen)
    trainer:  Trainer.step(...) (fused AdamW, the MLLM pass pipelined under the previous step, next batch's Q-Former
              prefetched), as bench.py times it

Both loops see the same batches (four synthetic batches in rotation).  Runs alternate literal / trainer, each with its own
warm-up; a run's figure is host wall time over `--steps` steps between two device synchronisations.  Prints every run and
the median and spread (min .. max) of the runs of each loop.

--lora-trainable: the LoRA-only set (adapters of q_proj / v_proj train too); the literal loop then clips the gradient norm to
1.0 as modify_train.py:1192 does, and Trainer runs with max_grad_norm = 1.0 as bench.py --lora-trainable does.
--only literal|trainer: one loop only (a profiler run of its own)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=4, help="runs per loop (alternating)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--text-len", type=int, default=240)
    ap.add_argument("--preset", default="llama32_1b")
    ap.add_argument("--lora-trainable", action="store_true")
    ap.add_argument("--only", choices=["literal", "trainer"], default=None)
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("--steps: at least 20 timed steps per run")

    import torch

    from tcavt_amd import capi, config, model, synth, training
    from tcavt_amd.weights import make_weights

    torch.cuda.set_device(0)
    capi.init(0)
    dev = torch.device("cuda:0")
    cfg = config.PRESETS[args.preset](seq_len=18, out_len=30, use_lora=True)
    B = args.batch
    batches = []
    for j in range(4):
        b = synth.make_batch(cfg, B, text_len=args.text_len, seed=100 + j, ragged=True,
                             min_text=128 if args.text_len > 128 else max(1, args.text_len // 2))
        batches.append({k: torch.from_numpy(v).to(dev) for k, v in b.items()})

    def build():
        with torch.device(dev):
            m = model.MultiModalTrajectoryModel.from_config(cfg)
        W = make_weights(cfg, seed=1, backend="torch", device=dev)
        m.load_weights(W)
        del W
        m.set_storage(torch.float16)
        return m.train()

    def call_args(g):
        return (g["traj_emb"], g["vision_emb"], None, g["lane_polygon"], g["lane_polygon_len"])

    def kw(g):
        return dict(y=g["target_traj"], norm_stat=g["norm_stat"], input_ids=g["input_ids"],
                    attention_mask=g["attention_mask"], labels=g["labels"])

    loops = {}
    if args.only in (None, "literal"):
        ml = build()
        for p in ml.mllm.parameters():  # train.py:1141-1142
            p.requires_grad_(False)
        if args.lora_trainable:
            for n, p in ml.mllm.named_parameters():
                if ".lora_" in n:
                    p.requires_grad_(True)
        trainable = [p for p in ml.parameters() if p.requires_grad]
        optimizer = torch.optim.AdamW(trainable, lr=5e-4, weight_decay=1e-4)
        state = {"i": 0, "loss": None}

        def literal():
            g = batches[state["i"] % len(batches)]
            state["i"] += 1
            optimizer.zero_grad()
            loss, _ = ml(*call_args(g), **kw(g))
            loss.backward()
            if args.lora_trainable:
                torch.nn.utils.clip_grad_norm_(trainable, 1.0)
            optimizer.step()
            state["loss"] = loss.item()

        loops["literal"] = literal
    if args.only in (None, "trainer"):
        mt = build()
        tr = training.Trainer(mt, lr=5e-4, weight_decay=1e-4, lora_trainable=args.lora_trainable,
                              max_grad_norm=1.0 if args.lora_trainable else None)
        tstate = {"i": 0}

        def trainer():
            g = batches[tstate["i"] % len(batches)]
            nxt = batches[(tstate["i"] + 1) % len(batches)]
            tstate["i"] += 1
            tr.step(g["traj_emb"], g["vision_emb"], g["lane_polygon"], g["lane_polygon_len"], g["target_traj"],
                    g["norm_stat"], g["input_ids"], g["attention_mask"], g["labels"], next_vision_embs=nxt["vision_emb"],
                    inputs_ready=True if mt.pipeline_decoder else None)

        loops["trainer"] = trainer

    def run(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    res = {k: [] for k in loops}
    for r in range(args.runs):
        for k, fn in loops.items():
            ms = run(fn)
            res[k].append(ms)
            print(f"run {r} {k:8s} {ms:8.3f} ms/step", flush=True)
    form = "S1 (LoRA adapters train; grad-norm clip 1.0)" if args.lora_trainable else "S0 (train.py: MLLM frozen)"
    print(f"# {args.preset} B={B} L={cfg.q_num_query_tokens + args.text_len} train mode, {form}; "
          f"{args.runs} runs x ({args.warmup} warm-up + {args.steps} timed steps) per loop, alternating")
    for k, v in res.items():
        print(f"{k:8s} median {statistics.median(v):8.3f} ms/step  spread {min(v):.3f} .. {max(v):.3f}  runs "
              + " ".join(f"{x:.3f}" for x in v))
    if len(res) == 2:
        a, b = statistics.median(res["literal"]), statistics.median(res["trainer"])
        print(f"literal / trainer = {a / b:.3f}  (+{a - b:.3f} ms/step)")


if __name__ == "__main__":
    main()
