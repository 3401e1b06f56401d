"""Makes tests/golden/tiny_beam.npz: HF's own beam search results on a tiny model, and the logits rows a search needs to repeat them.

    python tests/golden/make_golden_beam.py          (needs torch and transformers 5.x; the test that reads the file needs neither)

A seeded, randomly initialised ``transformers.LlamaForCausalLM`` in float64 (V = 48) runs ``generate(num_beams=n, do_sample=False,
...)`` for the cases below.  Per case the file holds HF's ``sequences`` (the generated part) and ``sequences_scores``, and the raw
logits row after every generated prefix that tests/beam_ref.py's search visits (recorded from the same model), so that
tests/test_beam_reference_cpu.py replays the search from the file alone."""
import os
import sys

import numpy as np
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import beam_ref  # noqa: E402

V, PAD = 48, 0


class _Float64Torch:
    """``torch`` as transformers.generation.utils sees it while the fixture is made: HF's beam search casts the logits to
    torch.float32 and keeps its scores in torch.float whatever the model's dtype; with both names answering torch.float64 the same
    code runs in float64, which is what a float64 reference can be compared with at 1e-9."""

    def __getattr__(self, name):
        return torch.float64 if name in ("float32", "float") else getattr(torch, name)


# (n, N, length_penalty, early_stopping, repetition_penalty, no_repeat_ngram_size, eos, prompt seed); eos = -1: the token in the
# middle of the best hypothesis of the same search without an EOS, so that hypotheses of different lengths compete
CASES = [(2, 6, 1.0, False, 1.0, 0, -1, 0), (2, 8, 0.5, True, 1.2, 2, -1, 1), (2, 10, 2.0, False, 1.2, 3, -1, 2),
         (3, 6, 1.0, True, 1.2, 3, 5, 3), (3, 8, 2.0, False, 1.0, 2, 17, 4), (3, 10, 0.5, False, 1.2, 0, -1, 5),
         (4, 6, 0.5, False, 1.2, 2, -1, 6), (4, 8, 1.0, True, 1.0, 3, 30, 7), (4, 10, 1.0, False, 1.2, 3, -1, 8),
         (4, 10, 2.0, True, 1.2, 0, -1, 9), (3, 10, 1.0, False, 1.0, 0, 5, 10), (2, 10, 1.0, True, 1.2, 3, 30, 11)]


def main(out_path):
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(vocab_size=V, hidden_size=16, intermediate_size=32, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=2, max_position_embeddings=64)
    model = transformers.LlamaForCausalLM(cfg).to(torch.float64).eval()
    with torch.no_grad():
        for p in model.parameters():  # a sharper distribution than the default initialisation's: beams then differ and EOS occurs
            p.mul_(4.0)
    transformers.generation.utils.torch = _Float64Torch()
    data, reached, used = {}, 0, []
    for c, (n, N, lp, early, pen, ng, eos, pseed) in enumerate(CASES):
        prompt = np.random.default_rng(100 + pseed).integers(1, V, size=5)
        ids = torch.tensor(prompt[None], dtype=torch.long)

        def model_row(prefix):
            with torch.no_grad():
                return model(torch.tensor([list(prompt) + list(prefix)], dtype=torch.long)).logits[0, -1].numpy().copy()

        if eos < 0:
            eos = int(beam_ref.search(model_row, prompt, n, N, None, pen, ng, lp, early, pad=PAD)["sequences"][0, N // 2])
        used.append((n, N, lp, early, pen, ng, eos, pseed))
        with torch.no_grad():
            hf = model.generate(ids, attention_mask=torch.ones_like(ids), num_beams=n, do_sample=False, max_new_tokens=N,
                                length_penalty=lp, early_stopping=early, repetition_penalty=pen, no_repeat_ngram_size=ng,
                                eos_token_id=eos, pad_token_id=PAD, num_return_sequences=n, return_dict_in_generate=True,
                                output_scores=True)
        seq = hf.sequences[:, ids.shape[1]:].numpy()
        seqs = np.full((n, N), PAD, dtype=np.int64)
        seqs[:, :seq.shape[1]] = seq
        for row in seqs:  # (HF fills behind a hypothesis that ended early with EOS when pad_token_id is 0; the file holds the pad id)
            ends = np.nonzero(row == eos)[0]
            if ends.size:
                row[ends[0] + 1:] = PAD
        rows = {}

        def logits_fn(prefix):
            if prefix not in rows:
                rows[prefix] = model_row(prefix)
            return rows[prefix]

        ref = beam_ref.search(logits_fn, prompt, n, N, eos, pen, ng, lp, early, pad=PAD)
        assert np.array_equal(ref["sequences"], seqs), (c, ref["sequences"], seqs)
        assert np.allclose(ref["scores"], hf.sequences_scores.numpy(), rtol=1e-9, atol=0), (c, ref["scores"], hf.sequences_scores)
        reached += int((seqs == eos).any())
        keys = sorted(rows)
        pre = np.full((len(keys), N), -1, dtype=np.int64)
        for i, k in enumerate(keys):
            pre[i, :len(k)] = k
        data.update({f"c{c}_prompt": prompt.astype(np.int64), f"c{c}_sequences": seqs,
                     f"c{c}_scores": hf.sequences_scores.numpy().astype(np.float64), f"c{c}_prefixes": pre,
                     f"c{c}_rows": np.stack([rows[k] for k in keys]).astype(np.float64)})
        print(f"case {c}: n={n} N={N} lengths={(seqs != PAD).sum(1).tolist()} rows={len(keys)} eos={eos} reached={(seqs == eos).any()}")
    assert 2 * reached >= len(CASES), f"EOS reached in {reached} of {len(CASES)} cases only"
    data["cases"] = np.array(used, dtype=np.float64)
    np.savez_compressed(out_path, **data)
    print(out_path, os.path.getsize(out_path), "bytes; transformers", transformers.__version__)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tiny_beam.npz"))
