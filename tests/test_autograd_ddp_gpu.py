"""The reference's DistributedDataParallel wrap (scripts/train.py:1127-1142: DDP(model, device_ids, find_unused_parameters=True)
BEFORE the MLLM is frozen) around MultiModalTrajectoryModel, with loss.backward() through the autograd bridge (autograd.py):
(a) a one-rank RCCL group gives the bare loop's gradients bit for bit; (b) two gloo ranks on the one card, each with half of
the batch, give what one process computes on the whole batch."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tests.util import batch_tensors, load_case, rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

CASE = "tiny_6_12_lora_ragged"
JOIN_S = 400


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _literal(rows, dev, ddp=None):
    """train.py:1127-1145 and 1168-1183 on the fixture's batch rows -> (loss, {name: grad}, {name: parameter after the step})."""
    from tcavt_amd import model

    cfg, weights, fx = load_case(CASE)
    g = {k: v[rows].contiguous().to(dev) for k, v in batch_tensors(fx).items()}
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
    run = m
    if ddp is not None:
        from torch.nn.parallel import DistributedDataParallel

        run = DistributedDataParallel(m, **ddp)  # wrapped while every parameter still requires grad (train.py:1127-1132)
    for p in m.mllm.parameters():  # train.py:1141-1142
        p.requires_grad_(False)
    trainable = [p for p in m.parameters() if p.requires_grad]
    optimizer = torch.optim.AdamW(trainable, lr=5e-4, weight_decay=1e-4)
    optimizer.zero_grad()
    loss, _ = run(g["traj_emb"], g["vision_emb"], None, g["lane_polygon"], g["lane_polygon_len"], y=g["target_traj"],
                  norm_stat=g["norm_stat"], input_ids=g["input_ids"], attention_mask=g["attention_mask"], labels=g["labels"])
    loss.backward()
    grads = {n: p.grad.detach().clone().cpu() for n, p in m.named_parameters() if p.requires_grad}
    optimizer.step()
    torch.cuda.synchronize()
    params = {n: p.detach().clone().cpu() for n, p in m.named_parameters() if p.requires_grad}
    return float(loss.item()), grads, params


def _join(procs):
    for p in procs:
        p.join(JOIN_S)
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.kill()
        p.join()
    assert not alive, f"{len(alive)} worker(s) outlived the {JOIN_S} s join timeout and were killed"
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def _rccl_worker(port, outdir):
    import torch.distributed as dist

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    bare = _literal(slice(0, 2), dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        wrapped = _literal(slice(0, 2), dev, ddp=dict(device_ids=[0], find_unused_parameters=True))
    finally:
        dist.destroy_process_group()
    torch.save({"bare": bare, "ddp": wrapped}, os.path.join(outdir, "rccl.pt"))


def test_one_rank_rccl_ddp_equals_the_bare_loop(gpu, tmp_path):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), str(tmp_path)))
    p.start()
    _join([p])
    r = torch.load(os.path.join(str(tmp_path), "rccl.pt"))
    (l0, g0, p0), (l1, g1, p1) = r["bare"], r["ddp"]
    assert l0 == l1 and sorted(g0) == sorted(g1) and len(g0) > 0
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    assert all(torch.equal(p0[n], p1[n]) for n in p0)


def _gloo_worker(rank, world, port, outdir):
    import torch.distributed as dist

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out = _literal(slice(rank, rank + 1), torch.device("cuda", 0), ddp=dict(device_ids=[0], find_unused_parameters=True))
        torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process_on_the_whole_batch(gpu, tmp_path):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    _join(procs)
    (l0, g0, p0), (l1, g1, p1) = (torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(world))
    assert all(torch.equal(g0[n], g1[n]) for n in g0) and all(torch.equal(p0[n], p1[n]) for n in p0)
    loss, g_full, p_full = _literal(slice(0, world), gpu["device"])
    assert abs(0.5 * (l0 + l1) - loss) / loss < 1e-4
    names = sorted(g_full)
    worst = max(rel_err(g0[n], g_full[n]) for n in names if g_full[n].abs().max() > 0)
    flat = rel_err(torch.cat([g0[n].reshape(-1) for n in names]), torch.cat([g_full[n].reshape(-1) for n in names]))
    print(f"[ddp autograd] gradients: flat rel {flat:.2e}, worst tensor {worst:.2e}")
    assert flat < 1e-4 and worst < 1e-3  # (DDP averages: only the summation order over the batch differs)
    _, weights, _ = load_case(CASE)
    moved = torch.cat([(p_full[n] - torch.from_numpy(weights[n])).reshape(-1) for n in names]).double().norm()
    apart = torch.cat([(p0[n] - p_full[n]).reshape(-1) for n in names]).double().norm()
    print(f"[ddp autograd] parameters moved {moved:.3e}, two ranks vs one process {apart:.3e}")
    assert apart < 0.05 * moved
