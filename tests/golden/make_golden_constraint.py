"""Makes tests/golden/tiny_constraint.npz: HF's own constrained greedy decoding on a tiny model, and the logits rows needed to
repeat it.

    python tests/golden/make_golden_constraint.py    (needs torch and transformers; the test that reads the file needs neither)

A seeded, randomly initialised ``transformers.LlamaForCausalLM`` in float64 (V = 48) runs ``generate(prefix_allowed_tokens_fn=...,
do_sample=False)`` for the cases below: tries of choices, an allowed vocabulary, a suppressed set and a union of two forms, with
and without ``repetition_penalty``, with an EOS inside the form (the row ends on it) and outside it (the row runs to
max_new_tokens).  The function handed to HF is the constraint's own host rule -- ``allowed(walk(generated)[0])``.  Per case the file
holds the automaton's arrays, HF's generated ``sequences`` and the raw logits row after every visited prefix, so that
tests/test_constraint_reference_cpu.py replays the case from the file alone."""
import os
import sys

import numpy as np
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tcavt_amd.constraint import TokenConstraint  # noqa: E402

V, PAD = 48, 0
TRIE = ([11, 12], [20, 21, 22, 23], [30])
SHARED = ([11, 12, 13], [11, 12], [11, 14, 15, 16])  # one choice is a prefix of another


def _constraints():
    trie, trie9, shared = (TokenConstraint.from_sequences(V, s, e) for s, e in ((TRIE, 5), (TRIE, 9), (SHARED, 5)))
    union, starts = TokenConstraint.union([trie, TokenConstraint.from_sequences(V, ([33, 34], [35]), 5)])
    return dict(trie=(trie, trie.start), trie9=(trie9, trie9.start), shared=(shared, shared.start),
                vocab=(TokenConstraint.from_allowed_tokens(V, [2, 3, 7, 17, 19, 29, 41, 47]), 0),
                vocab_eos=(TokenConstraint.from_allowed_tokens(V, [2, 5, 7, 17, 19, 29, 41, 47]), 0),
                suppress=(TokenConstraint.from_suppressed_tokens(V, [0, 5] + list(range(10, 40))), 0),
                suppress_few=(TokenConstraint.from_suppressed_tokens(V, [0, 1, 2, 3]), 0), union=(union, starts[1]))


# (constraint, N, repetition_penalty, eos, prompt seed)
CASES = [("trie", 8, 1.0, 5, 0), ("trie", 8, 1.2, 5, 1), ("trie9", 8, 1.0, 5, 2), ("shared", 8, 1.2, 5, 3), ("vocab", 10, 1.0, 5, 4),
         ("vocab_eos", 10, 1.2, 5, 5), ("suppress", 10, 1.0, 5, 6), ("suppress_few", 10, 1.2, 5, 7), ("trie", 6, 1.2, 5, 8),
         ("union", 8, 1.0, 5, 9), ("shared", 8, 1.0, 5, 10)]


def main(out_path):
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(vocab_size=V, hidden_size=16, intermediate_size=32, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=2, max_position_embeddings=64)
    model = transformers.LlamaForCausalLM(cfg).to(torch.float64).eval()
    with torch.no_grad():
        for p in model.parameters():  # a sharper distribution than the default initialisation's
            p.mul_(4.0)
    forms, data, ended = _constraints(), {}, 0
    for c, (name, N, pen, eos, pseed) in enumerate(CASES):
        C, start = forms[name]
        prompt = np.random.default_rng(300 + pseed).integers(1, V, size=5)
        ids = torch.tensor(prompt[None], dtype=torch.long)

        def allowed_fn(batch_id, input_ids):
            state, n_ok = C.walk(input_ids[len(prompt):].tolist(), start=start)
            assert n_ok == len(input_ids) - len(prompt)
            return C.allowed(state)

        with torch.no_grad():
            hf = model.generate(ids, attention_mask=torch.ones_like(ids), do_sample=False, max_new_tokens=N, repetition_penalty=pen,
                                eos_token_id=eos, pad_token_id=PAD, prefix_allowed_tokens_fn=allowed_fn)
        seq = hf[0, len(prompt):].numpy()
        seqs = np.full(N, PAD, dtype=np.int64)
        seqs[:seq.size] = seq
        n_gen = seq.size if eos not in seq.tolist() else seq.tolist().index(eos) + 1
        seqs[n_gen:] = PAD
        ended += int(eos in seq.tolist())
        rows = []
        with torch.no_grad():
            for i in range(n_gen):  # the raw row after every visited prefix
                rows.append(model(torch.tensor([list(prompt) + seqs[:i].tolist()], dtype=torch.long)).logits[0, -1].numpy().copy())
        data.update({f"c{c}_prompt": prompt.astype(np.int64), f"c{c}_sequences": seqs, f"c{c}_rows": np.stack(rows).astype(np.float64),
                     f"c{c}_token_class": C.token_class.numpy(), f"c{c}_trans": C.trans.numpy()})
        data.setdefault("cases", []).append((N, pen, eos, start, n_gen))
        print(f"case {c}: {name} N={N} pen={pen} start={start} tokens={seqs.tolist()} n_generated={n_gen}")
    assert 3 <= ended <= len(CASES) - 3, f"EOS ended {ended} of {len(CASES)} cases"
    data["cases"] = np.array(data["cases"], dtype=np.float64)
    np.savez_compressed(out_path, **data)
    print(out_path, os.path.getsize(out_path), "bytes; transformers", transformers.__version__)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tiny_constraint.npz"))
