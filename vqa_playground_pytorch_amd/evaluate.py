"""Evaluation of the reference (train.py:110-191, visu.py:188-194): forward in eval mode without autograd, the logits turned
into answers on the GPU (csrc/loss.hip), the results written as the reference's JSON records.

    ev = Evaluator(model)                      # graph=True: the forward + predictions replayed as one hipGraph
    results, acc = ev.run(loader, a_vocab, eval_metric="OpenEnded")
    write_results(results, results_filename(log_dir, "val", "OpenEnded", epoch))

OpenEnded answers are the argmax of the logits, MultipleChoice answers the best-scoring column among a sample's
``a_mc_idx`` candidates (padded with -1), with the order of metrics.py (NaN above every number, ties to the lower column).
"""
import json
import os

import torch

from . import metrics


class Evaluator:
    """Forward + predictions of one batch, graph-replayed on the GPU.

    graph=True follows the trainer's recipe: the first batches run kernel by kernel (allocator, kernel attributes, the tuned
    GEMM table), then one forward + predictions pass on a side stream and ONE hipGraph captured on the batch shape it saw
    first, audited for memset nodes before it is instantiated.  A batch of another shape (the last one of an epoch) or with
    other keys runs kernel by kernel; so does every batch when the forward draws a host-side dropout seed.  The graph has
    its own memory pool: a trainer's captured graphs stay valid across an evaluation."""

    EAGER_STEPS_BEFORE_CAPTURE = 2

    def __init__(self, model, graph=True, k=5):
        self.model = model
        self.k = int(k)
        first = next(iter(model.parameters()), None)
        self.cuda = first is not None and first.is_cuda
        self.device = first.device if first is not None else torch.device("cpu")
        self.want_graph = bool(graph) and self.cuda
        self._graph = None
        self._eager_steps = 0
        self.graph_nodes = {}
        if self.cuda:
            from . import tuned_gemms
            tuned_gemms.enable()

    @staticmethod
    def _model_keys(sample):
        v = "v_packed" if "v_packed" in sample else "v"              # packed region batches (feed.store_batches(packed=True))
        v = "v_idx" if "v_idx" in sample else v                      # resident store: the images' indices (store_batches(resident=))
        keys = (v, "q_idxes") if "q_idxes" in sample else (v, "q")
        return keys + ("v_len",) if "v_len" in sample else keys      # per-sample region counts (cor2.Model.forward)

    def _inputs(self, sample):
        """The tensors one pass reads, on the model's device: the model's inputs, the target 'a', the candidates 'a_mc_idx'.
        'v_len' (region counts) is validated when it comes from the host and becomes the int32 device tensor the kernels read,
        so the replayed forward keeps it in a static input buffer like the rest.  A packed batch's 'v_packed' stands where 'v' does."""
        keys = list(self._model_keys(sample)) + [k for k in ("a", "a_mc_idx") if k in sample]
        inputs = {k: sample[k].to(self.device, non_blocking=True) for k in keys if k not in ("v_len", "v_idx")}
        if "v_idx" in sample:
            # a resident-store batch: the indices, range-checked when they come from the host, as the int32 device tensor the
            # gather reads -- a static input of the replayed forward like the rest; the counts are the store's
            from . import ops
            store = getattr(self.model, "region_store", None)
            if store is None:
                raise ValueError("'v_idx' needs a resident region store: attach one with model.use_region_store(...)")
            inputs["v_idx"] = ops.image_indices(sample["v_idx"], len(store), self.device)
        if "v_len" in sample and "v_idx" not in sample:
            from . import ops
            v = sample["v_packed"] if "v_packed" in sample else sample["v"]     # (packed: N rows for every entry of 'v_len')
            b = sample["v_len"].size(0) if "v_packed" in sample else v.size(0)
            inputs["v_len"] = ops.region_counts(sample["v_len"], v.numel() // (max(b, 1) * 2048), self.device)
        return inputs

    def _pass(self, inputs):
        """forward + predictions (what the graph holds) -> dict of output tensors."""
        logits = self.model({k: inputs[k] for k in self._model_keys(inputs)})
        top_idx, top_prob, hits = metrics.predict_topk(logits, self.k, target=inputs.get("a"))
        out = {"pred": top_idx[:, 0], "top_idx": top_idx, "top_prob": top_prob, "pred_mc": None}
        if "a_mc_idx" in inputs:
            out["pred_mc"] = metrics.predict_candidates(logits, inputs["a_mc_idx"])
        if hits is not None:
            out["hits"] = hits
        return out

    def step(self, sample):
        """One batch -> {'pred' [B], 'top_idx' [B,k], 'top_prob' [B,k], 'pred_mc' [B] (None without 'a_mc_idx'), and 'hits'
        int32 [k] when the sample carries its target 'a'}.  A replayed batch returns the graph's OWN output tensors,
        overwritten by the next replay (copy what you keep).  The model's train() / eval() mode is restored afterwards."""
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                return self._step(self._inputs(sample))
        finally:
            self.model.train(was_training)

    def _matches(self, inputs):
        g = self._graph
        return set(inputs) == set(g["inputs"]) and all(
            inputs[k].shape == t.shape and inputs[k].dtype == t.dtype for k, t in g["inputs"].items())

    def _step(self, inputs):
        if not self.want_graph:
            return self._pass(inputs)
        if self._graph is None:
            from . import ops
            seeds_before = ops.host_seed_draws
            out = self._pass(inputs)
            self._eager_steps += 1
            if ops.host_seed_draws != seeds_before:
                self.want_graph = False           # host-seeded dropout in the forward: a replay would freeze its mask
            elif self._eager_steps >= self.EAGER_STEPS_BEFORE_CAPTURE:
                try:
                    self._capture(inputs)
                except Exception as e:            # noqa: BLE001 -- any capture failure: keep evaluating kernel by kernel
                    from .trainer import report_capture_failure
                    self.want_graph = False
                    report_capture_failure("evaluator", e, "continuing with eager launches")
            return out
        g = self._graph
        if not self._matches(inputs):
            return self._pass(inputs)
        for k, t in g["inputs"].items():
            t.copy_(inputs[k], non_blocking=True)
        g["graph"].replay()
        return g["out"]

    def _capture(self, inputs):
        from .trainer import audit_and_instantiate
        static = {k: v.clone() for k, v in inputs.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._pass(static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, pool=torch.cuda.graph_pool_handle()):
            out = self._pass(static)
        self.graph_nodes = audit_and_instantiate({"graph": graph}, "evaluation")["graph"]
        self._graph = {"graph": graph, "inputs": static, "out": out}

    def run(self, batches, a_vocab=None, eval_metric="OpenEnded", max_step=None):
        """test() of the reference over `batches` (dicts as feed.collate makes them, with 'q_id'): -> (results, accuracy).
        results = [{'question_id', 'answer'}] with answer = a_vocab.idx2word(i) when a vocabulary is given, the column index
        otherwise, and None for a MultipleChoice row whose a_mc_idx holds no valid column (the reference would pass -1 to
        idx2word, which raises); accuracy = (Acc@1, Acc@5) in percent over every batch that carried its target 'a' (Acc@1 alone when
        k < 5), None when none did."""
        if eval_metric not in ("OpenEnded", "MultipleChoice"):
            raise ValueError("<evaluate.py> %s is not allowed" % eval_metric)
        topk = (1, 5) if self.k >= 5 else (1,)
        results, hits, n = [], None, 0
        for i, sample in enumerate(batches):
            if max_step is not None and i >= max_step:
                break
            if eval_metric == "MultipleChoice" and "a_mc_idx" not in sample:
                raise ValueError("MultipleChoice evaluation needs 'a_mc_idx' in every batch")
            out = self.step(sample)
            pred = (out["pred_mc"] if eval_metric == "MultipleChoice" else out["pred"]).cpu().tolist()
            q_id = sample["q_id"]
            q_id = q_id.tolist() if torch.is_tensor(q_id) else list(q_id)
            for qid, p in zip(q_id, pred):
                if p < 0:
                    answer = None                 # MultipleChoice row without a valid candidate: no answer (JSON null)
                else:
                    answer = a_vocab.idx2word(int(p)) if a_vocab is not None else int(p)
                results.append({"question_id": int(qid), "answer": answer})
            if "hits" in out:
                h = out["hits"].to(torch.int64).cpu()
                hits = h if hits is None else hits + h
                n += len(pred)
        acc = tuple(metrics.accuracy(hits, n, topk)) if hits is not None else None
        return results, acc


def results_filename(log_dir, split, eval_metric, epoch):
    """train.py:182-187: log_dir/epoch_<epoch>/vqa_<metric>_mscoco_<split>2015_<log dir name><epoch:03d>_results.json
    (split 'test_dev' is written 'test-dev')."""
    if split == "test_dev":
        split = "test-dev"
    method = "%s%.3d" % (log_dir.split("/")[-1], epoch)
    return os.path.join(log_dir, "epoch_%s" % epoch, "vqa_%s_mscoco_%s2015_%s_results.json" % (eval_metric, split, method))


def write_results(results, path):
    """The result records as plain JSON (the reference's data2file); creates the directory."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as fh:
        json.dump(results, fh)
    return path
