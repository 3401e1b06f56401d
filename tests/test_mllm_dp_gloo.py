"""Data-parallel stage-1 step on CPU: 2 ranks over gloo (training.MllmTrainer(data_parallel=True)).

Kernels cannot run here, so the C library is stubbed (as in test_dp_gloo.py) and the model's LM pass and the two backward
walks are replaced by stand-ins that plant per-rank losses, labelled-row counts and gradients; what is checked is the
distributed logic: the construction broadcast, each bucket summed exactly once over all its elements, 1 / world in the clip
call, one loss for every rank's gate, and the g_loss values of the global token mean."""
import math
import os
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dp_gloo import _StubLib, _free_port

COUNTS = {"ragged": (30, 10), "empty": (40, 0)}  # labelled rows of rank 0 / rank 1
LOSSES = (2.0, 5.0)


def _worker(rank, world, port, q, front, norm, counts):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from tcavt_amd import config, model, ops, training
        from tcavt_amd.weights import make_weights

        stub = _StubLib()
        ops.lib = lambda: stub
        ops.stream_ptr = lambda: None
        ops._ALLOW_CPU = True
        cfg = config.tiny(use_lora=True)
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0)).eval()
        lora_w = [p for n, p in m.named_parameters() if ".lora_A." in n][0]
        if rank == 1:  # rank 1 starts from different weights: the broadcast must bring rank 0's over
            with torch.no_grad():
                lora_w.add_(1.0)
                m.mllm.q_proj.weight.add_(1.0)
        tr = training.MllmTrainer(m, train_mllm_front=front, process_group=None, data_parallel=True, loss_normalization=norm)
        ok_bcast = True
        for w in (lora_w, m.mllm.q_proj.weight):
            s = w.detach().clone()
            dist.broadcast(s, src=0)
            ok_bcast = ok_bcast and torch.equal(s, w.detach())
        assert tr.world == world and tr.data_parallel
        n, nl = tr.book.total, tr.n_lora
        assert (0 < nl < n) if front else (nl == n)
        assert all(".lora_" in k for k in tr.book.names[:4 * cfg.llama.layers])
        base = torch.arange(n, dtype=torch.float32) % 97 + 1
        N_r = counts[rank]
        loss_r = LOSSES[rank] if N_r > 0 else float("nan")
        seen = {}

        def lm_forward(vision_embs, context_str, input_ids=None, attention_mask=None, labels=None):
            st = SimpleNamespace(loss=torch.tensor([loss_r]), count=torch.tensor([N_r], dtype=torch.int32), B=2, L=8)
            return SimpleNamespace(loss=st.loss.reshape(()), n_tokens=st.count, state=st)

        def lm_loss_backward(st, g_loss=None, out=None):
            seen["g_loss"] = None if g_loss is None else float(g_loss)
            return torch.zeros(1)

        def lbw_run(g_final):
            tr.book.grads[:nl].copy_(base[:nl] * (rank + 1))
            return torch.zeros(1)

        m.mllm.lm_forward = lm_forward
        m.mllm.llama_wrapper.lm_loss_backward = lm_loss_backward
        tr.lbw.run = lbw_run
        if front:
            tr.qbw.run = lambda g_h0, B, L: tr.book.grads[nl:].copy_(base[nl:] * (rank + 1))
            tr.bw._leaf_streams = []
        loss = tr.forward_backward(None, None, None, None)
        ok_sum = torch.equal(tr.book.grads, base * sum(r + 1 for r in range(world)))
        m.mllm.llama_wrapper.refresh_lora = lambda *a, **k: None
        tr.optimizer_step()
        _, cargs = [c for c in stub.calls if c[0] == "tcavt_clip_grad_norm"][-1]
        ok_clip = abs(cargs[2] - 1.0) < 1e-9 and abs(cargs[3] - 1.0 / world) < 1e-9
        _, gargs = [c for c in stub.calls if c[0] == "tcavt_adamw_gated"][-1]
        ok_gate = abs(gargs[10] - 1.0) < 1e-9 and gargs[11].value == tr._gate_loss.data_ptr() and gargs[12].value is not None
        q.put((rank, ok_bcast, ok_sum, ok_clip, ok_gate, float(loss), float(tr._gate_loss), seen["g_loss"]))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))
        raise


def _run(front, norm, counts, target=_worker):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q, front, norm, counts)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(60)
    for r in results:
        assert len(r) == 8, r
        assert all(r[1:5]), r
    return results


@pytest.mark.timeout(300)
@pytest.mark.parametrize("front", [False, True], ids=["adapters", "adapters+front"])
def test_rank_normalization_exchange(front):
    r0, r1 = _run(front, "rank", COUNTS["ragged"])
    assert r0[5] == r1[5] == r0[6] == r1[6] == (LOSSES[0] + LOSSES[1]) / 2  # the mean of the ranks' losses, on both ranks
    assert r0[7] is None and r1[7] is None  # each rank's own token mean: g_loss stays 1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("front", [False, True], ids=["adapters", "adapters+front"])
def test_global_normalization_g_loss_and_loss(front):
    world, (n0, n1) = 2, COUNTS["ragged"]
    r0, r1 = _run(front, "global", COUNTS["ragged"])
    assert r0[7] == pytest.approx(world * n0 / (n0 + n1), rel=1e-6) and r1[7] == pytest.approx(world * n1 / (n0 + n1), rel=1e-6)
    assert r0[5] == r1[5] == r0[6] == r1[6]
    assert r0[5] == pytest.approx((n0 * LOSSES[0] + n1 * LOSSES[1]) / (n0 + n1), rel=1e-6)


@pytest.mark.timeout(300)
def test_a_rank_without_labels():
    """global: its g_loss is 0 and its NaN mean never reaches the reported loss; rank: the NaN reaches every rank's gate."""
    r0, r1 = _run(False, "global", COUNTS["empty"])
    assert r0[7] == pytest.approx(2.0, rel=1e-6) and r1[7] == 0.0
    assert r0[5] == r1[5] == r0[6] == r1[6] == pytest.approx(LOSSES[0], rel=1e-6)
    r0, r1 = _run(False, "rank", COUNTS["empty"])
    assert all(math.isnan(v) for v in (r0[5], r1[5], r0[6], r1[6]))


def _refused_worker(rank, world, port, q, front, norm, counts):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from tcavt_amd import config, model, training
        from tcavt_amd.weights import make_weights

        cfg = config.tiny(use_lora=True)
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0))
        msg = [""] * 2
        for i, kw in enumerate(({}, {"data_parallel": False})):
            try:
                training.MllmTrainer(m, **kw)
            except RuntimeError as e:
                msg[i] = str(e)
        try:
            training.MllmTrainer(m, data_parallel=True, loss_normalization="batch")
            bad = ""
        except ValueError as e:
            bad = str(e)
        ok = all("single process" in s and "2 ranks" in s for s in msg)
        q.put((rank, ok, "loss_normalization" in bad, True, True, 0.0, 0.0, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))
        raise


@pytest.mark.timeout(300)
def test_world_two_without_data_parallel_is_still_refused():
    _run(False, "rank", COUNTS["ragged"], target=_refused_worker)
