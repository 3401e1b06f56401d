"""The LM eval pass at the model level: LlamaMultiModal.lm_evaluate against lm_forward (same bits) and against the composed
path (ops.gemm_bf16 into fp32 logits, torch.argmax), and evaluate.evaluate_mllm -- token-weighted loss, accuracies, restored
state, two gloo ranks on one card -- on the tiny configuration of tests/test_lm_loss_model_gpu.py, in fp16 and bf16."""
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_dp_gpu import _free_port
from tests.test_lm_loss_gpu import U, _C_ACC
from tests.test_lm_loss_model_gpu import STORAGE, _model
from tests.util import batch_tensors, load_case

pytestmark = pytest.mark.gpu

CASE = "tiny_6_12_lora_ragged"
KEYS = ("vision_emb", "input_ids", "attention_mask", "labels")


def _batches(dev):
    """Two batches of the fixture's samples with very different labelled counts: all of the fixture's labels, and the first
    two labels of each sample only."""
    _, _, fx = load_case(CASE)
    t = batch_tensors(fx)
    full = {k: t[k].to(dev) for k in KEYS}
    few = dict(full)
    lab = torch.full_like(full["labels"], -100)
    for b in range(lab.shape[0]):
        idx = torch.nonzero(full["labels"][b] != -100).flatten()[:2]
        lab[b, idx] = full["labels"][b, idx]
    few["labels"] = lab
    n_full, n_few = int((full["labels"] != -100).sum()), int((lab != -100).sum())
    assert n_few > 0 and n_full >= 3 * n_few
    return [full, few]


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
def test_lm_evaluate_matches_lm_forward_and_the_composed_argmax(gpu, storage):
    from tcavt_amd import ops

    dev = gpu["device"]
    cfg, weights, _ = load_case(CASE)
    m = _model(cfg, weights, dev, storage)
    b = _batches(dev)[0]
    labels = b["labels"]
    B, Lt = labels.shape
    with torch.no_grad():
        ref = m.mllm.lm_forward(b["vision_emb"], None, b["input_ids"], b["attention_mask"], labels)
        loss_f, n_f = ref.loss.clone(), ref.n_tokens.clone()
        out = m.mllm.lm_evaluate(b["vision_emb"], None, b["input_ids"], b["attention_mask"], labels)
        torch.cuda.synchronize()
        m.mllm.check_flags()
        assert torch.equal(out.loss, loss_f) and torch.equal(out.n_tokens, n_f)
        assert out.loss.dim() == 0 and out.loss.dtype == torch.float32 and out.loss.is_cuda
        Nq = out.num_image_tokens
        L = Nq + Lt
        assert out.pred.dtype == torch.int64 and tuple(out.pred.shape) == (B, Lt) and tuple(out.row_loss.shape) == (B, Lt)
        assert tuple(out.final_hidden.shape) == (B, L, cfg.llama.hidden)
        # alignment with labels: -1 / 0 exactly where labels == -100
        lab = labels != -100
        assert (out.pred[~lab] == -1).all() and (out.pred[lab] >= 0).all() and (out.pred[lab] < cfg.llama.vocab).all()
        assert (out.row_loss[~lab] == 0).all() and (out.row_loss[lab] > 0).all()
        # the composed path on the same 16-bit operands
        h16 = ref.final_hidden_bf16[: B * L]
        table = m.mllm.llama_wrapper._prepared().table
        logits = ops.gemm_bf16(h16.contiguous(), table, out_dtype=torch.float32).view(B, L, -1)[:, Nq - 1:L - 1]
        bound = _C_ACC * U * (h16.double().abs() @ table.double().abs().T).view(B, L, -1)[:, Nq - 1:L - 1].max(dim=-1).values
        top2 = logits.double().topk(2, dim=-1).values
        sure = lab & ((top2[..., 0] - top2[..., 1]) > 2 * bound)
        excluded = int((lab & ~sure).sum())
        assert excluded <= 0.01 * int(lab.sum()), f"{excluded} of {int(lab.sum())} rows excluded"
        assert torch.equal(out.pred[sure], logits.argmax(dim=-1)[sure])
        # row_loss in the same alignment: cross-entropy of the composed logits (fp32 logits: 1e-5)
        ce = torch.nn.functional.cross_entropy(logits.double().reshape(B * Lt, -1), labels.reshape(-1), ignore_index=-100, reduction="none")
        assert torch.allclose(out.row_loss.double().reshape(-1), ce, rtol=1e-4, atol=1e-5)
        # counts and per-sample sums follow from pred / row_loss
        hit = lab & (out.pred == labels)
        assert int(out.n_correct) == int(hit.sum()) and int(out.n_tokens) == int(lab.sum())
        assert torch.equal(out.sample_tokens.long(), lab.sum(1)) and torch.equal(out.sample_correct.long(), hit.sum(1))
        ref_nll = out.row_loss.double().sum(1)
        assert ((out.sample_nll.double() - ref_nll).abs() <= 1e-6 * ref_nll.abs()).all()
    print(f"[lm_evaluate {storage}] loss {float(out.loss):.5f}, {int(out.n_correct)} of {int(out.n_tokens)} right, {excluded} rows excluded")


def _reference_metrics(m, batches):
    """What evaluate_mllm must return, from per-batch lm_evaluate outputs, in float64 on the host."""
    nll = ntok = ncor = nsmp = nall = 0.0
    means = []
    with torch.no_grad():
        for b in batches:
            o = m.mllm.lm_evaluate(b["vision_emb"], None, b["input_ids"], b["attention_mask"], b["labels"])
            lab = b["labels"] != -100
            hit = lab & (o.pred == b["labels"])
            nll += float(o.row_loss.double().sum())
            ntok += int(lab.sum())
            ncor += int(hit.sum())
            has = lab.sum(1) > 0
            nsmp += int(has.sum())
            nall += int((has & (hit.sum(1) == lab.sum(1))).sum())
            means.append(float(o.loss))
    return {"loss": nll / ntok, "token_accuracy": ncor / ntok, "sequence_accuracy": nall / nsmp, "n_tokens": int(ntok),
            "n_samples": int(nsmp)}, means


def _check_metrics(got, want):
    assert got["n_tokens"] == want["n_tokens"] and got["n_samples"] == want["n_samples"]
    assert got["token_accuracy"] == want["token_accuracy"] and got["sequence_accuracy"] == want["sequence_accuracy"]
    assert abs(got["loss"] - want["loss"]) <= 1e-6 * abs(want["loss"])
    assert abs(got["perplexity"] - math.exp(want["loss"])) <= 2e-6 * math.exp(want["loss"])


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
def test_evaluate_mllm_is_token_weighted_and_restores_the_model(gpu, storage):
    from tcavt_amd import evaluate

    dev = gpu["device"]
    cfg, weights, _ = load_case(CASE)
    m = _model(cfg, weights, dev, storage)
    batches = _batches(dev)
    want, means = _reference_metrics(m, batches)
    lw = m.mllm.llama_wrapper
    m.train(True)
    lw.save_for_backward = True
    got = evaluate.evaluate_mllm(m, batches)
    assert m.training and lw.save_for_backward is True
    assert set(got) == {"loss", "perplexity", "token_accuracy", "sequence_accuracy", "n_tokens", "n_samples"}
    _check_metrics(got, want)
    mean_of_means = sum(means) / len(means)
    assert abs(got["loss"] - mean_of_means) > 1e-6 * abs(got["loss"]), "the two batch means must not average to the token mean"
    print(f"[evaluate_mllm {storage}] {got}; mean of the batch means {mean_of_means:.6f}")

    def raising():
        yield batches[0]
        raise KeyError("loader failed")

    with pytest.raises(KeyError):
        evaluate.evaluate_mllm(m, raising())
    assert m.training and lw.save_for_backward is True
    m.train(False)
    lw.save_for_backward = False
    assert evaluate.evaluate_mllm(m, batches[:1])["n_tokens"] == int((batches[0]["labels"] != -100).sum())
    assert not m.training and lw.save_for_backward is False
    # no labelled token at all: NaN ratios, nothing raises
    none = dict(batches[0])
    none["labels"] = torch.full_like(none["labels"], -100)
    empty = evaluate.evaluate_mllm(m, [none])
    assert empty["n_tokens"] == 0 and empty["n_samples"] == 0
    assert all(math.isnan(empty[k]) for k in ("loss", "perplexity", "token_accuracy", "sequence_accuracy"))
    # a bad label in any batch is reported at the end of the loop
    bad = dict(batches[0])
    bad["labels"] = bad["labels"].clone()
    bad["labels"][0, 0] = cfg.llama.vocab
    with pytest.raises(ValueError, match="labels"):
        evaluate.evaluate_mllm(m, [bad])


def _eval_worker(rank, world, port, storage, outdir):
    import torch.distributed as dist

    from tcavt_amd import capi, evaluate

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        capi.init(0)
        dev = torch.device("cuda", 0)
        cfg, weights, _ = load_case(CASE)
        m = _model(cfg, weights, dev, storage)
        got = evaluate.evaluate_mllm(m, _batches(dev)[rank::world])
        torch.save(got, os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_return_the_single_process_result(gpu, tmp_path):
    from tcavt_amd import evaluate

    world, storage = 2, "fp16"
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_eval_worker, args=(r, world, port, storage, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)  # each child under its own time limit
        if p.is_alive():
            p.kill()
    assert [p.exitcode for p in procs] == [0] * world
    cfg, weights, _ = load_case(CASE)
    m = _model(cfg, weights, gpu["device"], storage)
    want = evaluate.evaluate_mllm(m, _batches(gpu["device"]))
    for r in range(world):
        got = torch.load(tmp_path / f"rank{r}.pt")
        _check_metrics(got, want)
