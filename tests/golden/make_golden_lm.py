"""Generate tests/golden/tiny_lm_loss.npz: the LM loss the REFERENCE's own modules compute and discard (build container only).

Run:  python tests/golden/make_golden_lm.py        (needs /root/reference; not needed on the GPU box)

`outputs.loss` of LlamaWithCrossAttnPEFT.forward(..., labels=fused_labels) (scripts/train.py:445-453, 536-552) is captured by
a forward hook on model.mllm.llama_wrapper while the reference's LlamaMultiModal.forward runs on the batch of each model case
of make_golden.py -- nothing of the reference is restated here; the model, the LoRA shim and the cases are make_golden's.
Cases: the three of make_golden.CASES, plus "<case 1>_answers": case 1 with the first ceil(len / 2) labels of every row set to
-100 (len = the row's valid text length), so that only "answer" tokens count.

Per case the file holds (arrays only):  <case>.loss float64, <case>.n (labelled rows), <case>.labels, and for the LoRA cases
the gradient of that loss with respect to every adapter matrix (eval mode: dropout off), <case>.grad.<state-dict key> sampled
and capped per tensor as make_golden._sample does, with <case>.gnorm.<key> the float64 norm of the whole tensor.
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

ANSWERS_OF = 0  # index into make_golden.CASES of the case the "answers only" variant is made from


def answers_only(labels, attention_mask):
    lab = labels.copy()
    for b in range(lab.shape[0]):
        n = int(attention_mask[b].sum())
        lab[b, : -(-n // 2)] = -100
    return lab


def run_lm_case(ref, out, name, preset, T, To, lora, B, text_len, ragged, empty_every, seed, labels_fn=None, tag=None):
    cfg = mg.tconfig.PRESETS[preset](seq_len=T, out_len=To, use_lora=lora)
    weights = mg.make_weights(cfg, seed)
    model = mg.build_reference_model(ref, cfg, weights)
    batch = mg.synth.make_batch(cfg, B, text_len=text_len, seed=seed, ragged=ragged, min_text=4, empty_polygon_every=empty_every)
    labels = batch["labels"] if labels_fn is None else labels_fn(batch["labels"], batch["attention_mask"])
    t = {k: torch.from_numpy(v) for k, v in batch.items()}
    seen = []
    hook = model.mllm.llama_wrapper.register_forward_hook(lambda mod, args, output: seen.append(output.loss))
    adapters = {}
    if lora:
        for i, layer in enumerate(model.mllm.llama_wrapper.llama_model.model.layers):
            for proj in ("q_proj", "v_proj"):
                m = getattr(layer.self_attn, proj)
                key = f"{mg.LLAMA_PREFIX}layers.{i}.self_attn.{proj}."
                adapters[key + "lora_A.weight"], adapters[key + "lora_B.weight"] = m.A, m.B
    for p in model.parameters():
        p.requires_grad_(False)
    for p in adapters.values():
        p.requires_grad_(True)
    model.eval()
    try:
        with torch.set_grad_enabled(lora):
            model.mllm(t["vision_emb"], None, input_ids=t["input_ids"], attention_mask=t["attention_mask"],
                       labels=torch.from_numpy(labels))
    finally:
        hook.remove()
    assert len(seen) == 1 and seen[0] is not None
    loss = seen[0]
    n = int((labels != -100).sum())  # every label position p + 1 >= Nq has a predicting row p
    key = tag or name
    out[key + ".loss"] = np.array(loss.item(), np.float64)
    out[key + ".n"] = np.array(n, np.int64)
    out[key + ".labels"] = labels
    norms = []
    if lora:
        grads = torch.autograd.grad(loss, list(adapters.values()))
        for k, g in zip(adapters, grads):
            out[f"{key}.grad.{k}"] = mg._sample(g)
            out[f"{key}.gnorm.{k}"] = np.array(g.double().norm().item())
            norms.append(g.double().norm().item() ** 2)
    print(f"[golden] lm loss {key}: loss={loss.item():.6f} labelled rows {n} of {labels.size}"
          + (f", adapter gradient norm {sum(norms) ** 0.5:.4f}" if lora else ""))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    with redirect_stdout(io.StringIO()):
        ref = mg._import(os.path.join(mg.REF, "ablation_study_without_lora.py"), "ref_nolora")
    out = {}
    for case in mg.CASES:
        run_lm_case(ref, out, *case)
    run_lm_case(ref, out, *mg.CASES[ANSWERS_OF], labels_fn=answers_only, tag=mg.CASES[ANSWERS_OF][0] + "_answers")
    out["cases"] = np.array([c[0] for c in mg.CASES] + [mg.CASES[ANSWERS_OF][0] + "_answers"])
    np.savez_compressed(os.path.join(HERE, "tiny_lm_loss.npz"), **out)


if __name__ == "__main__":
    main()
