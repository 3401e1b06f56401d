"""Data-parallel stage-1 step with REAL kernels: training.MllmTrainer(data_parallel=True) on two ranks that share the one card
and exchange over gloo (the spawn pattern of tests/test_dp_gpu.py: RCCL refuses two ranks on one device), and on a one-rank
RCCL group with TCAVT_FORCE_DP=1.  Tiny configuration, eval arithmetic (dropout masks depend on the position in the local
batch).  Ragged batch: rank 0 holds samples 0 and 1 with 27 labels, rank 1 sample 2 with 9.

  "global": loss, flat gradient and parameters after one step against ONE process on the whole batch
  "rank"  : against one process that averages the two half-batch gradients (what HF + DDP computes)
Both sides of either comparison approximate the same exact gradient within the adapter-gradient bars of
tests/test_lm_loss_model_gpu.py (norm deviation of the flat gradient, 1 - cosine), so the bar here is twice those constants.
Parameters: AdamW's first step moves every element by lr * sign(g), so an element whose gradient is a rounding away from zero
may move the other way; the bar is the one tests/test_dp_gpu.py uses, distance apart < 5 % of the distance moved.  The loss
sums the same row losses in another order: 1e-6 relative.  Both ranks must end with identical parameters (torch.equal)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_dp_gpu import _free_port
from tests.test_lm_loss_model_gpu import GRAD_COS_BAR, GRAD_NORM_BAR, _model
from tests.util import batch_tensors, load_case

pytestmark = pytest.mark.gpu

CASE = "tiny_6_12_lora_ragged"
KEYS = ("vision_emb", "input_ids", "attention_mask", "labels")
ROWS = (slice(0, 2), slice(2, 3))  # the samples of rank 0 / rank 1
LR = 1e-3
SCENARIOS = [("fp16", "global", "ragged"), ("fp16", "rank", "ragged"), ("bf16", "global", "ragged"), ("bf16", "rank", "ragged"),
             ("fp16", "global", "empty"), ("fp16", "rank", "empty")]


def _batch(kind):
    """The whole batch on the host: rank 0's samples carry three times rank 1's labels (27 / 9); kind "empty": rank 1 has none."""
    _, _, fx = load_case(CASE)
    t = {k: v.clone() for k, v in batch_tensors(fx).items() if k in KEYS}
    t["labels"][1, 7:] = -100
    if kind == "empty":
        t["labels"][2] = -100
    n = (t["labels"] != -100).sum(1)
    assert int(n[0] + n[1]) == 27 and int(n[2]) == (9 if kind == "ragged" else 0)
    return t


def _args(t, rows, dev):
    return [t[k][rows].contiguous().to(dev) for k in KEYS]


def _trainer(storage, dev, **kw):
    from tcavt_amd import training

    cfg, weights, _ = load_case(CASE)
    m = _model(cfg, weights, dev, storage)
    return training.MllmTrainer(m, lr=LR, **kw)


def _finish(tr, loss):
    """(loss, gradient as forward_backward left it, parameters before / after the update, optimizer counters)"""
    torch.cuda.synchronize()
    grads, before = tr.book.grads.detach().clone().cpu(), tr.book.params.detach().clone().cpu()
    tr.optimizer_step()
    torch.cuda.synchronize()
    tr.check_flags()
    return {"loss": float(loss), "grads": grads, "before": before, "params": tr.book.params.detach().clone().cpu(),
            "counters": tr.optimizer_counters()}


def _dp_worker(rank, world, port, outdir):
    import torch.distributed as dist

    from tcavt_amd import capi

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        capi.init(0)
        dev = torch.device("cuda", 0)
        out = {}
        for storage, norm, kind in SCENARIOS:
            tr = _trainer(storage, dev, data_parallel=True, loss_normalization=norm)
            assert tr.world == world and tr.data_parallel
            loss = tr.forward_backward(*_args(_batch(kind), ROWS[rank], dev))
            out[(storage, norm, kind)] = _finish(tr, loss)
        torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def dp_results(tmp_path_factory):
    """One pair of fresh child processes runs every scenario; each child under its own time limit."""
    out = tmp_path_factory.mktemp("mllm_dp")
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, str(out))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        if p.is_alive():
            p.kill()
    assert [p.exitcode for p in procs] == [0] * world
    return [torch.load(out / f"rank{r}.pt") for r in range(world)]


def _single(storage, kind, norm, dev):
    tr = _trainer(storage, dev)
    t = _batch(kind)
    if norm == "global":  # one process on the whole batch
        return _finish(tr, tr.forward_backward(*_args(t, slice(0, 3), dev)))
    parts = []  # one process that averages the two half-batch gradients and losses
    for rows in ROWS:
        loss = tr.forward_backward(*_args(t, rows, dev))
        torch.cuda.synchronize()
        parts.append((loss.clone(), tr.book.grads.detach().clone()))
    tr.book.grads.copy_((parts[0][1] + parts[1][1]) / 2)
    tr._gate_loss = ((parts[0][0] + parts[1][0]) / 2).reshape(1)
    return _finish(tr, tr._gate_loss)


def _compare(r0, r1, ref, storage, what):
    assert torch.equal(r0["grads"], r1["grads"]) and r0["loss"] == r1["loss"], f"{what}: the ranks hold different sums"
    assert torch.equal(r0["params"], r1["params"]), f"{what}: the replicas diverged"
    assert r0["counters"] == r1["counters"] == ref["counters"] == (1, 0)
    g, gr = r0["grads"].double() / 2, ref["grads"].double()  # SUM over two ranks -> DDP's mean
    norm_dev = abs(float(g.norm()) - float(gr.norm())) / float(gr.norm())
    cos = float(g @ gr / (g.norm() * gr.norm()))
    e_loss = abs(r0["loss"] - ref["loss"]) / abs(ref["loss"])
    moved = float((ref["params"] - ref["before"]).double().norm())
    apart = float((r0["params"] - ref["params"]).double().norm())
    print(f"[mllm dp {what}] loss {r0['loss']:.6f} vs {ref['loss']:.6f} (rel {e_loss:.2e}); flat gradient: norm deviation {norm_dev:.2e}, "
          f"1 - cosine {1 - cos:.2e}; parameters moved {moved:.3e}, apart {apart:.3e}")
    assert e_loss <= 1e-6
    # measured on an MI355X: loss equal to the last bit in every case; norm deviation 7.0e-10 (global fp16), 3.0e-11 (global
    # bf16), 0 (rank, and global with an unlabelled rank); 1 - cosine <= 2.4e-15; parameters apart <= 6.1e-8 of 1.15e-1 moved
    assert norm_dev < 2 * GRAD_NORM_BAR[storage] and 1 - cos < 2 * GRAD_COS_BAR[storage]
    assert moved > 0 and apart < 0.05 * moved


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
@pytest.mark.parametrize("norm", ["global", "rank"])
def test_two_ranks_on_a_ragged_batch(gpu, dp_results, storage, norm):
    r0, r1 = (r[(storage, norm, "ragged")] for r in dp_results)
    assert torch.equal(r0["before"], r1["before"])
    _compare(r0, r1, _single(storage, "ragged", norm, gpu["device"]), storage, f"{norm} {storage}")


def test_a_rank_without_labels_global(gpu, dp_results):
    """The rank contributes a zero gradient and g_loss 0; the update is applied on both ranks and equals the single-process step."""
    r0, r1 = (r[("fp16", "global", "empty")] for r in dp_results)
    _compare(r0, r1, _single("fp16", "empty", "global", gpu["device"]), "fp16", "global, rank 1 without labels")


def test_a_rank_without_labels_rank(gpu, dp_results):
    """Rank 1's mean is NaN: the exchanged loss is NaN on both ranks, both skip, and the replicas stay identical."""
    r0, r1 = (r[("fp16", "rank", "empty")] for r in dp_results)
    assert r0["counters"] == r1["counters"] == (0, 1)
    assert r0["loss"] != r0["loss"] and r1["loss"] != r1["loss"]
    for r in (r0, r1):
        assert torch.equal(r["params"], r["before"])
    assert torch.equal(r0["params"], r1["params"])


def _rccl_worker(port, outdir):
    import torch.distributed as dist

    from tcavt_amd import capi

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    capi.init(0)
    dev = torch.device("cuda", 0)
    t = _batch("ragged")
    out = {}
    for name in ("plain", "plain_again"):  # two runs of the step without the exchange: how far the backward itself repeats
        tr = _trainer("fp16", dev)
        out[name] = _finish(tr, tr.forward_backward(*_args(t, slice(0, 3), dev)))
    os.environ["TCAVT_FORCE_DP"] = "1"
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        for norm in ("rank", "global"):
            tr = _trainer("fp16", dev, data_parallel=True, loss_normalization=norm)
            assert tr._force_dp and tr.data_parallel and tr.world == 1
            buckets, inner = [], tr._allreduce_bucket

            def spy(lo, hi):  # the bucket as the backward left it against what the RCCL all-reduce made of it
                before = tr.book.grads[lo:hi].detach().clone()
                inner(lo, hi)
                buckets.append((int(lo), int(hi), bool(torch.equal(before, tr.book.grads[lo:hi]))))

            tr._allreduce_bucket = spy
            loss = tr.forward_backward(*_args(t, slice(0, 3), dev))
            torch.cuda.synchronize()
            same_loss = bool(torch.equal(tr._gate_loss.reshape(()), tr.last.loss))
            state = [x.detach().clone() for x in (tr.book.grads, tr.book.params, tr.m, tr.v, tr._ctl)]
            r = _finish(tr, loss)
            # the update of the step without the exchange, from the same gradient and state
            for dst, src in zip((tr.book.grads, tr.book.params, tr.m, tr.v, tr._ctl), state):
                dst.copy_(src)
            tr.data_parallel, tr._gate_loss = False, tr.last.loss.reshape(1)
            tr.optimizer_step()
            torch.cuda.synchronize()
            r.update(buckets=buckets, same_loss=same_loss, params_without=tr.book.params.detach().clone().cpu(), total=tr.book.total)
            out[norm] = r
        torch.save(out, os.path.join(outdir, "rccl.pt"))
    finally:
        dist.destroy_process_group()
        os.environ.pop("TCAVT_FORCE_DP", None)


@pytest.mark.timeout(300)
def test_one_rank_rccl_group_is_the_identity(gpu, tmp_path):
    """A SUM over one rank is the identity: gradients, parameters and loss are torch.equal to the step without the exchange.

    The LoRA backward accumulates some gradients with float atomics and does not repeat bit for bit from one run to the next
    (ABI version 5; on an MI355X the step through the one-rank group differed from a SEPARATE run
    of the plain step beyond the fourth digit of some gradient elements, while every bucket is bit-unchanged by its
    all-reduce; the run-to-run differences are printed), so "the step without the exchange" is taken from the SAME backward: every bucket is compared before and
    after its RCCL all-reduce, the gate's loss with the LM forward's, and the parameters with those the update without
    the exchange path gives from the same gradient and optimizer state -- all bit for bit.  Against a second run of the
    plain step the bars are those tests/test_dp_gpu.py uses for the same comparison."""
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), str(tmp_path)))
    p.start()
    p.join(200)
    if p.is_alive():
        p.kill()
    assert p.exitcode == 0, f"worker exit code {p.exitcode}"
    r = torch.load(os.path.join(str(tmp_path), "rccl.pt"))
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    print(f"[mllm dp rccl] two runs of the plain step: flat gradient rel {rel(r['plain_again']['grads'], r['plain']['grads']):.2e}, "
          f"parameters rel {rel(r['plain_again']['params'], r['plain']['params']):.2e}")
    for norm in ("rank", "global"):
        d = r[norm]
        assert [b[:2] for b in d["buckets"]] == [(0, d["total"])] and all(b[2] for b in d["buckets"]), (norm, d["buckets"])
        assert d["same_loss"] and d["loss"] == r["plain"]["loss"], norm
        assert torch.equal(d["params"], d["params_without"]), norm
        assert d["counters"] == (1, 0)
        e_g, e_p = rel(d["grads"], r["plain"]["grads"]), rel(d["params"], r["plain"]["params"])
        print(f"[mllm dp rccl {norm}] vs a second run without the exchange: flat gradient rel {e_g:.2e}, parameters rel {e_p:.2e}")
        assert e_g < 1e-5 and e_p < 1e-3
