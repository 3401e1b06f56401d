"""The launch sequence of generate_batch(num_beams=n) on the stub library of tests/generation_stub.py (extended here by the two
beam entries): prefill -> state_fanout -> select -> reorder -> (N - 1) x (decode_step_shared -> select -> reorder), with the rows,
beams and shapes in the integer scalars; and num_beams=1, passed explicitly, records exactly the golden trace of the call without."""
import ctypes
import json
import os

import pytest
import torch

import generation_stub

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generation_trace.json")
I32P = ctypes.POINTER(ctypes.c_int32)


class BeamStub(generation_stub.StubLibrary):
    """The device's part of the two beam entries: the step words count up, and with ``done_at`` every prompt is done (all rows
    finished) once that many selections have run."""

    done_at = None

    def _beam_select(self, args, stream):
        a = args._obj
        step = ctypes.cast(a.step, I32P)
        if self.done_at is not None and step[0] + 1 >= self.done_at:
            for r in range(a.R):
                ctypes.cast(a.finished, I32P)[r] = 1

    def _beam_reorder(self, args, stream):
        a = args._obj
        for b in range(a.R // a.n):
            ctypes.cast(a.step, I32P)[b] += 1


@pytest.fixture
def beam_stub(monkeypatch):
    monkeypatch.setattr(generation_stub, "StubLibrary", BeamStub)
    return BeamStub


def _run(N, **kw):
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 2)
        res = m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=N, use_graph=False, pad_token_id=7,
                                    do_sample=False, **kw)
    return stub.calls, res, cfg, m


@pytest.mark.parametrize("N", [1, 2, 5])
def test_launch_sequence_of_three_beams(beam_stub, N):
    calls, out, cfg, _ = _run(N, num_beams=3)
    names = [c[0] for c in calls]
    i = names.index("tcavt_state_fanout")
    assert "tcavt_llama_stack_forward" in names[:i] and not any(nm.startswith(("tcavt_sample", "tcavt_beam", "tcavt_kv_fanout")) for nm in names[:i])
    step = ["tcavt_llama_decode_step_shared", "tcavt_beam_select", "tcavt_beam_reorder"]
    assert names[i:] == ["tcavt_state_fanout", "tcavt_beam_select", "tcavt_beam_reorder"] + step * (N - 1)
    sel = next(c[1][0] for c in calls if c[0] == "tcavt_beam_select")
    assert (sel["R"], sel["n"], sel["V"], sel["N"], sel["early_stopping"]) == (6, 3, cfg.llama.vocab, N, 0)
    reo = next(c[1][0] for c in calls if c[0] == "tcavt_beam_reorder")
    assert (reo["R"], reo["n"], reo["suffix_lmax"], reo["n_layers"]) == (6, 3, max(N - 1, 1), cfg.llama.layers)
    assert tuple(out.shape) == (2, N) and out.dtype == torch.int64  # num_return_sequences = 1: the best hypothesis per prompt


def test_return_sequences_info_and_early_exit(beam_stub):
    beam_stub.done_at = 3
    try:
        calls, (out, info), _, _ = _run(8, num_beams=4, num_return_sequences=2, return_info=True, poll_every=1, early_stopping=True,
                                        length_penalty=0.5)
    finally:
        beam_stub.done_at = None
    assert tuple(out.shape) == (4, 8)
    assert info["steps"] == 2 and [c[0] for c in calls].count("tcavt_llama_decode_step_shared") == 2  # all done after 3 selections
    assert set(info) == {"sequences_scores", "n_generated", "finish_reason", "steps", "beam_trace"}
    assert info["sequences_scores"].shape == (4,) and info["sequences_scores"].dtype == torch.float32
    assert info["n_generated"].dtype == torch.int32 and info["finish_reason"].tolist() == [4] * 4
    assert info["beam_trace"]["parent"].shape == (3, 2, 8) and info["beam_trace"]["acc"].dtype == torch.float32
    assert next(c[1][0] for c in calls if c[0] == "tcavt_beam_select")["early_stopping"] == 1


def test_share_prefix_makes_no_difference(beam_stub):
    a = _run(4, num_beams=2, share_prefix=True)[0]
    b = _run(4, num_beams=2, share_prefix=False)[0]
    assert a == b


@pytest.mark.parametrize("kv_cache", ["fp16", "fp8"])
def test_one_beam_records_exactly_the_golden_trace(kv_cache):
    with open(GOLDEN) as f:
        want = json.load(f)[f"batch_n5/{kv_cache}"]
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 3)
        m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, kv_cache=kv_cache,
                              max_new_tokens=5, num_beams=1, length_penalty=1.0, early_stopping=False)
    bufs = [[n, list(shape), str(dt)] for ws in (m.mllm._ws, m.mllm.llama_wrapper._ws) for n, shape, dt in ws._bufs]
    assert json.loads(json.dumps(stub.calls)) == want["calls"]
    assert json.loads(json.dumps(bufs)) == want["workspace"]
