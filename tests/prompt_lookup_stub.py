"""generation_stub's stub library with the entries of prompt-lookup decoding: tcavt_ngram_draft is recorded only, tcavt_spec_verify
plays the device's part as a sampler call does there -- every live sequence commits one token (no draft is ever accepted), so a row
ends at its budget and the host loop's polls see it.

``record_all()`` runs SCENARIOS and returns {scenario: {"calls", "workspace"}}; ``python tests/prompt_lookup_stub.py OUT.json``
writes that as the golden file tests/golden/prompt_lookup_trace.json (run with the package of the commit to record on the path)."""
import contextlib
import json
import os
import sys

import generation_stub as G


class StubLibrary(G.StubLibrary):
    def _spec_verify(self, args, stream):
        a = args._obj
        s = a.sample.contents
        self._advance(range(a.S), s.step, s.finished, s.max_new, s.out_row, s.stop)


@contextlib.contextmanager
def stubbed():
    """generation_stub.stubbed with the library above"""
    from tcavt_amd import ops

    stub = StubLibrary()
    saved = (ops.lib, ops.stream_ptr, ops._ALLOW_CPU, os.environ.get("TCAVT_DECODE_ROWMAJOR"))
    ops.lib, ops.stream_ptr, ops._ALLOW_CPU = (lambda: stub), (lambda: None), True
    os.environ["TCAVT_DECODE_ROWMAJOR"] = "1"
    try:
        yield stub
    finally:
        ops.lib, ops.stream_ptr, ops._ALLOW_CPU = saved[:3]
        if saved[3] is None:
            del os.environ["TCAVT_DECODE_ROWMAJOR"]
        else:
            os.environ["TCAVT_DECODE_ROWMAJOR"] = saved[3]


SCENARIOS = {  # name -> (requests, keyword arguments of generate_batch)
    "k3_n1": (3, dict(max_new_tokens=1, prompt_lookup_num_tokens=3)),
    "k3_n2": (3, dict(max_new_tokens=2, prompt_lookup_num_tokens=3)),
    "k3_n7": (3, dict(max_new_tokens=7, prompt_lookup_num_tokens=3)),
    "k1_m4_poll2_rules": (2, dict(max_new_tokens=6, prompt_lookup_num_tokens=1, max_matching_ngram_size=4, poll_every=2, **G.RULES)),
    "k7_nret2": (2, dict(max_new_tokens=4, prompt_lookup_num_tokens=7, num_return_sequences=2)),
}


def record(name):
    R, kw = SCENARIOS[name]
    with stubbed() as stub:
        cfg, m = G.tiny_model()
        vis, ids, mask = G._requests(cfg, R)
        res = m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, **kw)
    bufs = [[n, list(shape), str(dt)] for ws in (m.mllm._ws, m.mllm.llama_wrapper._ws) for n, shape, dt in ws._bufs]
    return dict(calls=stub.calls, workspace=bufs), res


def record_all():
    return {name: record(name)[0] for name in SCENARIOS}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(record_all(), f, separators=(",", ":"))
        f.write("\n")
