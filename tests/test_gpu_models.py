"""GPU parity of the full CoR2 / ODA heads (HIP kernels through the C ABI) against the golden vectors
produced by the reference itself (tests/golden/*.npz) and against the torch-CPU oracle.
Tolerance: 1e-3 relative fp32 (BASELINE.json north_star), written as RTOL below."""
import os

import numpy as np
import pytest
import torch

from kernel_harness import dev
from oracle import reference_faithful as RF
from oracle import seeded

pytestmark = pytest.mark.gpu

RTOL = 1e-3


def rel(got, want):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-20)


ATOL = 1e-7  # gradients that are mathematically zero (the region-side Mutan biases and the attention-conv bias sit
#              in front of a softmax over regions: a per-glimpse constant shift) come out as ~1e-9..1e-8 rounding
#              noise on both sides; every other gradient here is O(1e-4..1), so 1e-7 absolute is fp32 noise


def grad_err(got, want, atol=ATOL):
    """max |got-want| measured against RTOL*scale + atol; <= 1 passes."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return np.abs(got - want).max() / (RTOL * np.abs(want).max() + atol)


ATOL_512 = 4e-6  # the same mathematically-zero gradients summed over 512 x 36 rows (with the dropout factor 2).  What the product
#                  holds there is not random noise alone: a sample's d_logits sum to (1 - sum_n alpha_n) * <alpha, dal>, and a float32
#                  softmax is normalised to ~1e-7 -- 512 such residuals, each times an inner product of O(1e-2), add up to 1e-6 ... 2e-6
#                  (measured over rounds 4-6 and both engines: 0.7e-6 ... 2.15e-6, depending on the summation order of the kernels in
#                  front).  Every other gradient of these models is O(1e-3..1) at its maximum, where this floor is nothing.


def check_grads(model, gold):
    worst = 0.0
    for name, p in model.named_parameters():
        gq = p.grad.detach().cpu().numpy().astype(np.float64)
        n = np.sqrt((gq ** 2).sum())
        gn = float(gold["g." + name + ".norm"])
        assert abs(n - gn) <= RTOL * gn + ATOL * np.sqrt(gq.size), (name, n, gn)
        # compare elements on the tensor's own scale (a corner of a big weight grad can be tiny)
        tol = RTOL * np.abs(gq).max() + ATOL
        e = np.abs(gq.reshape(gq.shape[0], -1)[:8, :8] - gold["g." + name + ".corner"]).max() / tol
        assert e <= 1.0, (name, e)
        if "g." + name + ".full" in gold.files:
            e = np.abs(gq - gold["g." + name + ".full"]).max() / tol
            assert e <= 1.0, (name, e)
        worst = max(worst, e)
    return worst


def build(cls, nans, **kw):
    from vqa_playground_pytorch_amd import CoR2Model, ODAModel
    model = {"cor2": CoR2Model, "oda": ODAModel}[cls](["PAD", "UNK"], nans, **kw)
    return seeded.load_state(model, 0).eval().to(dev())


@pytest.mark.parametrize("k4_form", ["folded", "engine"])
@pytest.mark.parametrize("mode", [1, 0])
def test_cor2_matches_reference_golden(golden_dir, mode, k4_form, monkeypatch):
    """The reference's own outputs and gradients (B = 4), with the relation step in both modes and the Mutan fusion in
    both of its forms (at 4 samples the default picks the R-GEMM one; training batches get the rank-folded one)."""
    from vqa_playground_pytorch_amd import ops
    monkeypatch.setattr(ops, "_K4_FORM", k4_form)
    gold = np.load(os.path.join(golden_dir, "cor2_b4.npz"))
    model = build("cor2", 2000, relation_mode=mode)
    v, q, a = seeded.seeded_inputs(4, answers=2000, seed=1)
    qt = torch.from_numpy(q).to(dev()).requires_grad_()
    logits = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": qt})
    loss = RF.kld_sum_loss(logits, torch.from_numpy(a).to(dev()))
    loss.backward()
    assert rel(logits, gold["logits"]) <= RTOL
    assert abs(loss.item() - gold["loss"]) <= RTOL * abs(gold["loss"])
    assert rel(qt.grad, gold["dq"]) <= RTOL
    ad = model.alpha_dict
    assert isinstance(ad["alpha1"], tuple) and len(ad["alpha1"]) == 4 and ad["alpha1"][0].shape == (4, 36, 1)
    assert rel(torch.cat(ad["alpha1"], 2), gold["alpha_dict.alpha1"]) <= RTOL
    assert rel(torch.cat(ad["alpha2"], 2), gold["alpha_dict.alpha2"]) <= RTOL
    assert ad["feature"].shape == (4, 2, 2048) and rel(ad["feature"], gold["alpha_dict.feature"]) <= RTOL
    check_grads(model, gold)


@pytest.mark.parametrize("head_form", ["auto", "grouped", "legacy"])
def test_cor2_intermediates_match_reference_golden(golden_dir, head_form, monkeypatch):
    """Module outputs captured by forward hooks.  With the grouped head (auto: CoR2's default) fusion_final runs inside a phase
    (head.VectorFusion): the module itself is not called, so its hook only fires with the legacy head."""
    from vqa_playground_pytorch_amd import head
    monkeypatch.setattr(head, "MODE", head_form)
    gold = np.load(os.path.join(golden_dir, "cor2_b4.npz"))
    model = build("cor2", 2000)
    caps = {}
    names = ["fusion_vq1", "fusion_vq2", "compress_v", "compress_v2"] + (["fusion_final"] if head_form == "legacy" else [])
    hooks = [getattr(model, k).register_forward_hook(lambda _m, _i, o, k=k: caps.__setitem__(k, o)) for k in names]
    hooks.append(model.compress_v2.register_forward_pre_hook(lambda _m, i: caps.__setitem__("v2_feature", i[0])))
    v, q, _ = seeded.seeded_inputs(4, answers=2000, seed=1)
    with torch.no_grad():
        model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    for k in names + ["v2_feature"]:
        assert rel(caps[k], gold[k]) <= RTOL, k
    for h in hooks:
        h.remove()


def test_oda_matches_reference_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, "oda_b4.npz"))
    model = build("oda", 3000)
    v, q, a = seeded.seeded_inputs(4, answers=3000, seed=1)
    qt = torch.from_numpy(q).to(dev()).requires_grad_()
    logits = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": qt})
    loss = RF.kld_sum_loss(logits, torch.from_numpy(a).to(dev()))
    loss.backward()
    assert rel(logits, gold["logits"]) <= RTOL
    assert abs(loss.item() - gold["loss"]) <= RTOL * abs(gold["loss"])
    assert rel(qt.grad, gold["dq"]) <= RTOL
    assert model.alpha_dict["alphas"].shape == (4, 36, 1)
    assert rel(model.alpha_dict["alphas"], gold["alpha_dict.alphas"]) <= RTOL
    check_grads(model, gold)


@pytest.mark.parametrize("cls,nans", [("cor2", 2000), ("oda", 3000)])
def test_batch_of_one_and_odd_batches(cls, nans):
    """The reference crashes at B=1 (squeeze bug); the drop-in must not.  Also a ragged B=5."""
    model = build(cls, nans)
    oracle = seeded.load_state({"cor2": RF.CoR2Oracle, "oda": RF.ODAOracle}[cls](nans), 0).eval()
    for B in (1, 5):
        v, q, _ = seeded.seeded_inputs(B, answers=nans, seed=40 + B)
        with torch.no_grad():
            got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
            want = oracle({"v": torch.from_numpy(v), "q": torch.from_numpy(q)})
        assert got.shape == (B, nans)
        assert rel(got, want.numpy()) <= RTOL


# ---- the heads at the BASELINE batch (512 x 36 x 2048) against the float64 restatement -------------------------------------
EPS_EDGE = 3e-5        # a relu pre-activation closer to zero than this (float64 run) makes its sample a "knife-edge" sample
KEEP_MIN = {"cor2": 0.4, "oda": 0.7}   # share of the 512 samples that must be free of them (measured: ~0.45 / ~0.78)
RTOL_EDGE_FRO = 1e-2   # knife-edge samples: relative Frobenius error of a gradient tensor (a handful of flipped relu units does
#                        not move the norm: this is the bar that would catch a systematic error) ...
RTOL_EDGE_MAX = 1e-1   # ... and its max-abs error on the tensor's own scale: a sanity bound only -- ONE flipped unit moves one
#                        row of a glimpse layer's gradient by that sample's whole contribution (measured: 1.8e-2 of the scale
#                        for a single sample, 3.9e-2 over ODA's 149 knife-edge samples of this batch)
VARIANTS = [("cor2", 2000, "default"), ("cor2", 2000, "pairwise"), ("cor2", 2000, "k4_engine"), ("cor2", 2000, "legacy_head"),
            ("cor2", 2000, "grouped_head"), ("oda", 3000, "default"), ("oda", 3000, "grouped_head"),
            ("cor2", 2000, "fp32_mfma"), ("oda", 3000, "fp32_mfma"), ("cor2", 2000, "grouped_split")]
_oracle_cache = {}


def build_variant(cls, nans, variant, monkeypatch):
    """default = what bench.py times; pairwise = relation_mode 0 (the relation tensor built from every (i,j) term);
    k4_engine = the Mutan fusion in its R-GEMM form on the LDS tile engine (VQA_K4_FORM=engine); legacy_head / grouped_head =
    the [B,.]-sized layers all on library GEMMs + epilogue kernels / all as grouped phases (VQA_HEAD=legacy / grouped; the
    default, auto, groups CoR2's phases except the glimpse projections and keeps ODA on the library); grouped_split = EVERY grouped
    phase's GEMM launch on the split kernel (csrc/grouped_gemm_split.hip; the default runs four of the eight there).  Every
    variant but fp32_mfma runs the region projections on the split engine (the default since round 5: fp32 products from three-way bf16 splits on the
    bf16 matrix pipe, csrc/gemm_f32_split.hpp); fp32_mfma = the same on the fp32 MFMA engine (VQA_F32_PRODUCTS=mfma) -- both
    engines are held to the SAME bars."""
    from vqa_playground_pytorch_amd import head, ops
    monkeypatch.setenv("VQA_F32_PRODUCTS", "mfma" if variant == "fp32_mfma" else "split")
    if variant == "k4_engine":
        monkeypatch.setattr(ops, "_K4_FORM", "engine")
    if variant in ("legacy_head", "grouped_head"):
        monkeypatch.setattr(head, "MODE", variant.split("_")[0])
    if variant == "grouped_split":
        monkeypatch.setattr(head.Phase, "ENGINE", "split")
    return build(cls, nans, **({"relation_mode": 0} if variant == "pairwise" else {}))


def oracle_at_512(cls, nans, v, q, a, key, masks=None):
    """The float64 restatement over the batch, 64 samples at a time (the reference's [B,N,N,2048] relation tensor is 11 GB in
    float64 at B = 512; the loss is a sum over samples, so chunk gradients add up).  -> logits, the mask of the samples
    free of knife-edge relu units, and TWO gradient sets: of the loss over those samples, and of the loss over the rest.
    masks: {site: mask tensor [B, ...]} switches the restatement's own dropout off and multiplies every Drop* layer's
    input by the given mask (training-mode comparison).  Cached per key: the variants of one head share it."""
    if key in _oracle_cache:
        return _oracle_cache[key]
    B = v.shape[0]
    o64 = seeded.load_state({"cor2": RF.CoR2Oracle, "oda": RF.ODAOracle}[cls](nans), 0)
    o64 = (o64.train() if masks is not None else o64.eval()).double()
    rng = [0, 0]
    if masks is not None:
        sites = 0
        for name, mod in o64.named_modules():
            if isinstance(mod, (RF.DropLinear, RF.DropConv1x1)):
                assert mod.p == 0.5 and name in masks, name
                mod.p = None                                    # (its own F.dropout off: the site's input is masked by the hook)
                mod.register_forward_pre_hook(lambda _m, args, name=name: (args[0] * masks[name][rng[0]:rng[1]].double(),))
                sites += 1
        assert sites == len(masks) == {"cor2": 19, "oda": 9}[cls]
    closest = []
    activate = RF._activate

    def spy(x, af, dim):
        if af == "relu":
            closest.append(x.detach().abs().reshape(x.size(0), -1).amin(1))
        return activate(x, af, dim)

    params = [p for _, p in o64.named_parameters()]
    g_keep = [torch.zeros_like(p) for p in params]
    g_edge = [torch.zeros_like(p) for p in params]
    RF._activate = spy
    keep, want = [], []
    try:
        for lo in range(0, B, 64):
            rng[0], rng[1] = lo, lo + 64
            del closest[:]
            w64 = o64({"v": torch.from_numpy(v[lo:lo + 64]).double(), "q": torch.from_numpy(q[lo:lo + 64]).double()})
            assert len(closest) >= 4
            k = torch.stack(closest).amin(0) >= EPS_EDGE
            t64 = torch.from_numpy(a[lo:lo + 64]).double()
            for sel, acc in ((k, g_keep), (~k, g_edge)):
                if bool(sel.any()):
                    gs = torch.autograd.grad(RF.kld_sum_loss(w64[sel], t64[sel]), params, retain_graph=True, allow_unused=True)
                    for dst, g in zip(acc, gs):
                        if g is not None:
                            dst.add_(g)
            keep.append(k)
            want.append(w64.detach())
    finally:
        RF._activate = activate
    names = [n for n, _ in o64.named_parameters()]
    out = (torch.cat(want), torch.cat(keep), dict(zip(names, (g.numpy() for g in g_keep))),
           dict(zip(names, (g.numpy() for g in g_edge))))
    _oracle_cache[key] = out
    return out


def compare_at_512(cls, model, got, a, want, keep, g_keep, g_edge, tag):
    """Logits on all 512 samples at RTOL; parameter gradients of the loss over the knife-edge-free samples at RTOL; and -- so
    that no sample's gradient goes unverified -- of the loss over the knife-edge samples at the looser stated bars."""
    B = got.shape[0]
    assert rel(got, want.numpy()) <= RTOL
    n_keep = int(keep.sum())
    assert n_keep >= KEEP_MIN[cls] * B, (tag, n_keep)
    kd = keep.to(dev())
    at = torch.from_numpy(a).to(dev())
    params = dict(model.named_parameters())
    gs = torch.autograd.grad(RF.kld_sum_loss(got[kd], at[kd]), list(params.values()), retain_graph=True)
    for (n, _), g in zip(params.items(), gs):
        assert grad_err(g, g_keep[n], ATOL_512) <= 1.0, (tag, n, n_keep)
    if n_keep < B:
        gs = torch.autograd.grad(RF.kld_sum_loss(got[~kd], at[~kd]), list(params.values()))
        worst = 0.0
        for (n, _), g in zip(params.items(), gs):
            g64 = g.detach().cpu().numpy().astype(np.float64)
            w = g_edge[n]
            assert np.isfinite(g64).all()
            e_max = np.abs(g64 - w).max() / (RTOL_EDGE_MAX * np.abs(w).max() + ATOL_512)
            e_fro = np.sqrt(((g64 - w) ** 2).sum()) / (RTOL_EDGE_FRO * np.sqrt((w ** 2).sum()) + ATOL_512 * np.sqrt(w.size))
            assert e_max <= 1.0 and e_fro <= 1.0, (tag, n, B - n_keep, e_max, e_fro)
            worst = max(worst, e_max * RTOL_EDGE_MAX)
        print("[%s] knife-edge samples: %d of %d, worst max-abs gradient error %.2e of the tensor's scale" % (tag, B - n_keep, B, worst))


@pytest.mark.parametrize("cls,nans,variant", VARIANTS)
def test_baseline_batch_against_oracle(cls, nans, variant, monkeypatch):
    """BASELINE configs[1] size -- 512 samples of 36 x 2048 regions -- through the whole head, eval mode (the dropout masks are
    the one thing the two sides cannot share): logits and EVERY parameter gradient against the restatement of the reference
    run in float64 on the CPU.  At this size the model dispatches to the kernels the benchmark times (rank-folded K4 on the
    register-tile engine, the fused relation + projection node and its in-tile data gradient, the single-launch K3
    backward, K2 on the 4x4 MFMA), which the B = 4 reference goldens do not reach; the `pairwise` and `k4_engine` variants
    run the same comparison with the relation step's forward on the pairwise kernel and with K4 in its R-GEMM form.

    Among the 6-11 million relu pre-activations of such a batch a few dozen lie within float32 rounding of zero, and which
    side they fall on decides whether that unit's gradient exists: there the reference's own float32 arithmetic is 2e-3
    (CoR2 compress_v2) to 2e-2 (one unit of an ODA glimpse layer) away from its float64 value, and so is any float32
    implementation.  The samples that own such a pre-activation (|x| < EPS_EDGE in the float64 run) are split off: the
    gradient of the loss over the other samples (>= 40 % of the batch for CoR2, >= 70 % for ODA, asserted) is compared at
    RTOL, the gradient of the loss over the knife-edge samples at RTOL_EDGE_MAX of each tensor's scale and RTOL_EDGE_FRO in
    the Frobenius norm.  Samples are independent and the batch that runs through the kernels is 512 in both passes."""
    B = 512
    model = build_variant(cls, nans, variant, monkeypatch)
    v, q, a = seeded.seeded_inputs(B, answers=nans, seed=512)
    got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    assert got.shape == (B, nans)
    want, keep, g_keep, g_edge = oracle_at_512(cls, nans, v, q, a, (cls, "eval"))
    compare_at_512(cls, model, got, a, want, keep, g_keep, g_edge, "%s/%s/eval" % (cls, variant))


def forward_recording_masks(model, cls, v, q):
    """One training-mode forward of the product with every dropout mask it applies rebuilt from the seeds it drew (each mask of
    the HIP path is a pure function of (seed, element index)): -> logits, {restatement site: mask}, the seeds.  Also asserts the
    wiring -- one seed per site, the site-to-mask layouts of both head forms."""
    from vqa_playground_pytorch_amd import ops
    B, N = v.shape[0], v.shape[1]
    assert N == 36
    seeds, rec, orig = [], [], {}
    for name in ("next_dropout_seed", "dropout", "linear_act", "attention_logits", "softmax_attention_pool_drop",
                 "relation_projection", "relation_apply", "object_difference_attention"):
        orig[name] = getattr(ops, name)

    def next_seed():
        seeds.append(orig["next_dropout_seed"]())
        return seeds[-1]

    def spy_dropout(x, p_drop, groups=0):
        n0 = len(seeds)
        out = orig["dropout"](x, p_drop, groups)
        if len(seeds) > n0:
            rec.append(("dropout", ops.DropoutGroups.apply(torch.ones_like(x.contiguous()), p_drop, seeds[-1], groups)))
        return out

    def flat_mask(kind, like, p_drop, seed):
        if p_drop:
            K = like.shape[-1]
            rec.append((kind, ops.linear_dropout_mask(like.numel() // K, K, p_drop, seed, like.device).view(like.shape)))

    def spy_linear_act(x, w, bias=None, act=None, p_drop=0.0, seed=0, pregated=False):
        flat_mask("linear_act", x, p_drop, seed)
        return orig["linear_act"](x, w, bias, act, p_drop, seed, pregated)

    def spy_attention_logits(x, w, bias, p_drop=0.0, seed=0):
        flat_mask("attention_logits", x, p_drop, seed)
        return orig["attention_logits"](x, w, bias, p_drop, seed)

    def spy_pool_drop(logits, inputs, p_drop, seed, *rest):
        flat_mask("pool_drop", torch.empty(inputs.shape[0], logits.shape[2], inputs.shape[2], device=inputs.device), p_drop, seed)
        return orig["softmax_attention_pool_drop"](logits, inputs, p_drop, seed, *rest)

    def spy_relation_projection(vv, t, c2, w, bias, p_drop=0.0, seed=0, *rest):
        flat_mask("relation_projection", vv, p_drop, seed)
        return orig["relation_projection"](vv, t, c2, w, bias, p_drop, seed, *rest)

    def spy_relation_apply(x, t, c2, p_drop=0.0, seed=0):
        flat_mask("relation_apply", x, p_drop, seed)
        return orig["relation_apply"](x, t, c2, p_drop, seed)

    def spy_k2(vl, ql, w, bias, p_drop=0.0, seed=0, **kw):
        if p_drop:
            rec.append(("k2", ops.object_difference_dropout_mask(vl.shape[0], vl.shape[1], vl.shape[2], p_drop, seed, vl.device)))
        return orig["object_difference_attention"](vl, ql, w, bias, p_drop, seed, **kw)

    spies = {"next_dropout_seed": next_seed, "object_difference_attention": spy_k2, "dropout": spy_dropout, "linear_act": spy_linear_act,
             "attention_logits": spy_attention_logits, "softmax_attention_pool_drop": spy_pool_drop,
             "relation_projection": spy_relation_projection, "relation_apply": spy_relation_apply}
    from vqa_playground_pytorch_amd import head
    for name, f in spies.items():
        setattr(ops, name, f)
    # (the grouped head -- the [B,.]-sized layers -- reports the masks its kernels apply through its own spy)
    head._mask_spy = lambda site, rows, cols, p_, seed: rec.append(
        ("head:" + site, ops.linear_dropout_mask(rows, cols, p_, seed, dev())))
    try:
        torch.manual_seed(5)
        got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    finally:
        head._mask_spy = None
        for name, f in orig.items():
            setattr(ops, name, f)
    kinds = [k for k, _ in rec]
    m = [t.cpu() for _, t in rec]
    assert len(set(seeds)) == len(seeds) == len(rec)
    for t in m:
        assert set(torch.unique(t).tolist()) == {0.0, 2.0} and abs(float(t.mean()) - 1.0) < 0.01
    if cls == "cor2":
        if kinds[0].startswith("head:"):       # the grouped head (default): same sites, same layouts, reported by name
            assert kinds == ["head:question_in", "head:question_out", "linear_act", "attention_logits", "pool_drop",
                             "relation_projection", "attention_logits", "relation_apply", "head:fusion_out"], kinds
            m[0], m[1] = m[0].view(4, B, 2400), m[1].view(2, B, 310)
        else:
            assert kinds == ["dropout", "dropout", "linear_act", "attention_logits", "pool_drop", "relation_projection",
                             "attention_logits", "relation_apply", "dropout"], kinds
        assert m[0].shape == (4, B, 2400) and m[1].shape == (2, B, 310) and m[4].shape == (B, 4, 2048) and m[7].shape == (B, 4, 2048)
        masks = {"compress_q": m[0][0], "linear_q": m[0][1], "compress_q_1": m[0][2], "compress_q_2": m[0][3],
                 "expand_q_1": m[1][0], "expand_q_2": m[1][1], "compress_v": m[2], "att1.conv_att": m[3], "compress_v2": m[5],
                 "att2.conv_att": m[6], "linear_classif": m[8]}
        for g in range(4):
            masks["att1.list_linear_v_fusion.%d" % g] = m[4][:, g]
            masks["att2.list_linear_v_fusion.%d" % g] = m[7][:, g]
    else:
        if kinds[1].startswith("head:"):
            assert kinds == ["linear_act", "head:question_in", "k2", "pool_drop", "head:fusion_out"], kinds
            m[1] = m[1].view(2, B, 2400)
        else:
            assert kinds == ["linear_act", "dropout", "k2", "pool_drop", "dropout"], kinds
        assert m[1].shape == (2, B, 2400) and m[2].shape == (B, N, N * 310) and m[3].shape == (B, 4, 2048)
        masks = {"compress_v": m[0], "compress_q": m[1][0], "linear_q": m[1][1], "att.conv_att": m[2], "linear_classif": m[4]}
        for g in range(4):
            masks["att.list_linear_v_fusion.%d" % g] = m[3][:, g]

    return got, masks, seeds


@pytest.mark.parametrize("cls,nans,variant", VARIANTS)
def test_training_step_with_shared_masks_against_oracle(cls, nans, variant, monkeypatch):
    """The configuration the benchmark times -- CoR2 / ODA, 512 x 36 x 2048, TRAINING mode, dropout 0.5 at every site --
    against the float64 restatement of the reference fed the SAME masks.  Every mask of the HIP path is a pure function of
    (seed, element index) (`vqa_linear_dropout_mask` writes it for any [M,K] site), so the seeds the forward drew are
    enough to rebuild them: the restatement's own F.dropout is switched off and each Drop* layer's input is multiplied by the
    mask of the corresponding site instead.  Checks the wiring the per-kernel masked tests cannot: one seed per site, the
    site-to-mask layouts (four question projections sharing one draw, the gates' [2,B,310] draw, the pooled glimpses masked
    inside K3 / inside the relation map, K2's one-bit mask over [B,N,N*L]), backward regenerating the forward's masks.  Knife-edge
    relu samples are compared separately, as in test_baseline_batch_against_oracle; the variants are the same as there."""
    B = 512
    model = build_variant(cls, nans, variant, monkeypatch).train()
    v, q, a = seeded.seeded_inputs(B, answers=nans, seed=513)
    got, masks, seeds = forward_recording_masks(model, cls, v, q)
    want, keep, g_keep, g_edge = oracle_at_512(cls, nans, v, q, a, (cls, "train", tuple(str(x) for x in seeds)), masks)
    compare_at_512(cls, model, got, a, want, keep, g_keep, g_edge, "%s/%s/train" % (cls, variant))


def test_cor2_100_regions_against_oracle():
    """N=100 (BASELINE config 5's region count; the reference hard-codes 36, so the oracle is the checker)."""
    model = build("cor2", 500)
    oracle = seeded.load_state(RF.CoR2Oracle(500), 0).eval()
    v, q, a = seeded.seeded_inputs(2, regions=100, answers=500, seed=77)
    got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    want = oracle({"v": torch.from_numpy(v), "q": torch.from_numpy(q)})
    assert rel(got, want.detach().numpy()) <= RTOL
    RF.kld_sum_loss(got, torch.from_numpy(a).to(dev())).backward()
    RF.kld_sum_loss(want, torch.from_numpy(a)).backward()
    for (n, p), (_, po) in zip(model.named_parameters(), oracle.named_parameters()):
        assert grad_err(p.grad, po.grad.numpy()) <= 1.0, n


def test_train_mode_dropout_statistics():
    """Dropout cannot be bit-matched to torch's CPU stream; check train mode runs, is stochastic, finite,
    and that its mean logits over many draws approach the eval-mode logits' scale."""
    model = build("oda", 300).train()
    v, q, _ = seeded.seeded_inputs(8, answers=300, seed=9)
    s = {"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())}
    torch.manual_seed(0)
    a = model(s)
    b = model(s)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert (a - b).abs().max().item() > 0
    a.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    torch.manual_seed(0)
    c = model(s)
    assert torch.equal(a, c), "same torch seed must reproduce the same dropout masks"


@pytest.mark.parametrize("cls,fname,nans", [("cor2", "cor2_b4.npz", 2000), ("oda", "oda_b4.npz", 3000)])
def test_train_step_matches_reference_trajectory(cls, fname, nans, golden_dir):
    """The GPU train step (HIP forward/backward + gathered flat gradients + fused clip/Adam kernels) reproduces the
    3-step loss / grad-norm / lr / weight trajectory recorded from the reference model with the train.py:41-107
    step order (eval mode: dropout off)."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    gold = np.load(os.path.join(golden_dir, fname))
    model = build(cls, nans)
    tr = DataParallelTrainer(model, lr=1e-4, clip=0.25)
    losses, norms = [], []
    for step in range(3):
        v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(4, answers=nans, seed=101 + step))
        loss, norm = tr.step({"v": v, "q_idxes": q}, a)
        losses.append(loss.item())
        norms.append(norm.item())
    np.testing.assert_allclose(losses, gold["train3.loss"], rtol=RTOL)
    np.testing.assert_allclose(norms, gold["train3.gnorm"], rtol=RTOL)
    assert abs(tr.lr - float(gold["train3.lr"])) <= 1e-12 * tr.lr
    for name, p in model.named_parameters():
        if float(gold["g." + name + ".norm"]) < 1e-6:
            # mathematically-zero gradient (a bias in front of the softmax over regions): Adam turns the ~1e-9
            # rounding noise into +-lr steps whose signs differ between any two fp32 implementations
            continue
        w = p.detach().cpu().numpy().astype(np.float64)
        gn = float(gold["train3.w." + name + ".norm"])
        assert abs(np.sqrt((w ** 2).sum()) - gn) <= 1e-5 * gn, name
    sd = model.state_dict()          # parameters are views of the flat buffer now: the state_dict ABI is unchanged
    assert sd["compress_v.conv.weight"].shape == (310, 2048, 1)
    model.load_state_dict(sd)


def test_fused_adam_matches_torch_adam():
    from vqa_playground_pytorch_amd import ops
    torch.manual_seed(0)
    n = 100003
    p = torch.randn(n, device=dev())
    g = torch.randn(n, device=dev()) * 3
    ref_p = p.clone().requires_grad_()
    opt = torch.optim.Adam([ref_p], lr=1e-3)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    nc = torch.zeros(2, device=dev())
    ws = torch.empty(1024, device=dev(), dtype=torch.float64)
    for step in range(1, 4):
        gi = g * step
        ops.grad_norm_clip_coef(gi, 0.25, nc, ws)
        want_norm = torch.linalg.vector_norm(gi.double()).item()
        assert abs(nc[0].item() - want_norm) <= 1e-6 * want_norm
        ref_p.grad = gi.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], 0.25)
        opt.step()
        ops.adam_step(p, gi, m, v, nc, 1e-3, 0.9, 0.999, 1e-8, step)
        assert (p - ref_p.detach()).abs().max().item() <= 2e-6


def test_graph_replay_equals_eager_steps():
    """The hipGraph-replayed train step (two captured graphs, per-step scalars in device memory) follows exactly the
    same trajectory as the kernel-by-kernel step (eval mode: no dropout, so both are deterministic)."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    out = {}
    for mode in (False, True):
        model = build("cor2", 300)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=mode)
        v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(64, answers=300, seed=21))
        losses = []
        for step in range(7):
            loss, norm = tr.step({"v": v, "q_idxes": q}, a)
            losses.append((loss.item(), norm.item()))
        if mode:
            assert tr._graph is not None, "step was not captured"
            v2, q2, a2 = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(64, answers=300, seed=22))
            loss, _ = tr.step({"v": v2, "q_idxes": q2}, a2)      # new tensors: copied into the captured placeholders
            losses.append((loss.item(), 0.0))
        else:
            v2, q2, a2 = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(64, answers=300, seed=22))
            loss, _ = tr.step({"v": v2, "q_idxes": q2}, a2)
            losses.append((loss.item(), 0.0))
        # a batch of another shape (the short last batch of an epoch) is stepped kernel by kernel, and the captured
        # graphs keep serving the regular batches after it
        v3, q3, a3 = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(5, answers=300, seed=23))
        loss, _ = tr.step({"v": v3, "q_idxes": q3}, a3)
        losses.append((loss.item(), 0.0))
        v4, q4, a4 = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(64, answers=300, seed=24))
        loss, _ = tr.step({"v": v4, "q_idxes": q4}, a4)      # (the captured placeholders ARE the first batch's tensors)
        losses.append((loss.item(), 0.0))
        out[mode] = (losses, [p.detach().clone() for p in model.parameters()], tr.lr)
    # not bitwise: the d_alpha reductions of K1/K3 use float atomics and Adam renormalises every gradient, so the last
    # bits of near-zero gradients become +-lr steps; a small lr keeps that below the comparison threshold
    for (l0, n0), (l1, n1) in zip(out[False][0], out[True][0]):
        assert abs(l0 - l1) <= 1e-4 * abs(l0) and abs(n0 - n1) <= 1e-4 * max(abs(n0), 1e-6)
    assert out[False][2] == out[True][2]
    for p0, p1 in zip(out[False][1], out[True][1]):
        assert (p0 - p1).abs().max().item() <= 2e-3 * max(p0.abs().max().item(), 1e-3)


def test_stacked_parameters_are_views_of_the_flat_buffer():
    """After the trainer lays the parameters out, the per-step stack of same-shaped layers (glimpse projections, question
    projections, Mutan ranks) is a strided view of the flat buffer -- no copy -- and gradients still reach every member."""
    from vqa_playground_pytorch_amd import ops
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    model = build("cor2", 300)
    lins = [m.linear for m in model.att1.list_linear_v_fusion]
    before = ops.stack_params([l.weight for l in lins])
    assert before.data_ptr() != lins[0].weight.data_ptr()            # separate allocations: a real stack
    tr = DataParallelTrainer(model, lr=1e-4, clip=0.25)
    for group in ([l.weight for l in lins], [l.bias for l in lins],
                  [m.linear.weight for m in (model.compress_q, model.linear_q, model.compress_q_1, model.compress_q_2)],
                  [m.linear.weight for m in model.fusion_vq1.list_linear2]):
        st = ops.stack_params(group)
        assert st.data_ptr() == group[0].data_ptr() and st.shape == (len(group),) + tuple(group[0].shape)
        assert torch.equal(st, torch.stack([p.detach() for p in group]))
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(4, answers=300, seed=5))
    tr.step({"v": v, "q_idxes": q}, a)
    assert all(l.weight.grad is not None and torch.isfinite(l.weight.grad).all() for l in lins)
    sd = model.state_dict()
    assert sd["att1.list_linear_v_fusion.2.linear.weight"].shape == (155, 2048)


@pytest.mark.parametrize("name,nans", [("cor2", 300), ("oda", 300)])
def test_parameter_gradients_are_written_into_the_flat_buffer(name, nans):
    """The backward kernels write every parameter gradient at its offset of the trainer's flat gradient buffer
    (ops._grad_like): the per-step gather has nothing to copy, and the buffer holds what a plain backward computes."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    model = build(name, nans).eval()                      # eval: no dropout, the two backward passes see the same function
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(6, answers=nans, seed=11))
    sample = {"v": v, "q_idxes": q}
    from vqa_playground_pytorch_amd import ops
    loss = ops.kld_sum_loss(model(sample), a)
    ref = torch.autograd.grad(loss, [p for p in model.parameters() if p.requires_grad])   # separate tensors: no slots registered
    tr = DataParallelTrainer(model, lr=0.0, clip=0.0)
    f = tr.flat
    loss = ops.kld_sum_loss(model(sample), a)
    f.begin_backward()
    try:
        loss.backward()
    finally:
        f.end_backward()
    in_place = sum(p.grad is not None and p.grad.data_ptr() == g.data_ptr() for p, g in zip(f.params, f.g_views))
    names = {id(p): n for n, p in model.named_parameters()}
    copied = [names[id(p)] for p, g in zip(f.params, f.g_views) if p.grad is None or p.grad.data_ptr() != g.data_ptr()]
    f.gather_grads()
    assert f.last_gathered == 0 and in_place == len(f.params), copied
    by_id = {id(p): g for p, g in zip([p for p in model.parameters() if p.requires_grad], ref)}
    for p, view in zip(f.params, f.g_views):
        torch.testing.assert_close(view, by_id[id(p)], rtol=1e-4, atol=1e-6)


def test_relation_modes_agree_on_the_fused_node():
    """At batches the fused relation + projection node serves (B * 36 >= 1024 rows), relation_mode 0 runs the node's forward
    on the pairwise kernel and shares the rest with the closed form: logits and every parameter gradient of the two modes
    agree (eval mode: no dropout)."""
    torch.manual_seed(3)
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(32, answers=300, seed=13))
    v = v.repeat(9, 1, 1)[:260].contiguous()                # 260 samples: the in-register pairwise kernel wants B * D >= 2^19
    q, a = q.repeat(9, 1)[:260].contiguous(), a.repeat(9, 1)[:260].contiguous()
    from vqa_playground_pytorch_amd import ops
    m1 = build("cor2", 300).eval()
    m0 = build("cor2", 300, relation_mode=0).eval()
    m0.load_state_dict(m1.state_dict())
    grads = []
    for m in (m1, m0):
        loss = ops.kld_sum_loss(m({"v": v, "q_idxes": q}), a)
        gs = torch.autograd.grad(loss, [p for p in m.parameters() if p.requires_grad])
        grads.append((loss.item(), gs))
    assert abs(grads[0][0] - grads[1][0]) <= 1e-4 * abs(grads[0][0])
    for (n, _), g1, g0 in zip(m1.named_parameters(), grads[0][1], grads[1][1]):
        scale = g1.abs().max().item() + 1e-12
        # (+ 1e-6 absolute: the bias in front of a softmax over regions has a mathematically zero gradient -- rounding noise)
        assert (g1 - g0).abs().max().item() <= 1e-3 * scale + 1e-6, n


def test_graph_trainer_fed_by_prefetcher_matches_eager():
    """Distinct batches streamed from pinned host memory through feed.DevicePrefetcher (which recycles its two device
    slots) into the graph-replayed trainer: the loss sequence equals the eager trainer's on the same batches, and the
    caller's tensors are never written (the replayed graphs read private input buffers unless adopt_inputs=True)."""
    from vqa_playground_pytorch_amd.feed import DevicePrefetcher
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    batches = []
    for i in range(9):
        v, q, a = (torch.from_numpy(x).pin_memory() for x in seeded.seeded_inputs(32, answers=300, seed=60 + i))
        batches.append({"v": v, "q_idxes": q, "a": a})
    out = {}
    for mode in (False, True):
        tr = DataParallelTrainer(build("cor2", 300), lr=2e-5, clip=0.25, graph=mode)
        losses = []
        for b in DevicePrefetcher(batches, dev()):
            loss, _ = tr.step({"v": b["v"], "q_idxes": b["q_idxes"]}, b["a"])
            losses.append(loss.clone())              # device-side copy, no host read: the feeder keeps running ahead
        torch.cuda.synchronize()
        out[mode] = [x.item() for x in losses]
        if mode:
            assert tr._graph is not None, "step was not captured"
            mine = [t.data_ptr() for t in tr._graph["sample"].values()] + [tr._graph["target"].data_ptr()]
            assert not any(t.data_ptr() in mine for b in batches for t in b.values())
    for l0, l1 in zip(out[False], out[True]):
        assert abs(l0 - l1) <= 1e-4 * abs(l0), (out[False], out[True])


@pytest.mark.parametrize("overlap", [False, "force"])
def test_graph_per_input_slot_reads_batches_in_place(overlap):
    """input_slots (bench.py's rotating batches; a feeder's ring of resident buffers): the forward + backward graph is captured
    once per slot and reads the slot's tensors in place.  Same batches, same seeds as a trainer with ONE pair of graph input
    buffers that every batch is copied into: the loss sequences are identical -- and the slotted trainer's replays issue no copy
    of a batch (its graphs' input tensors ARE the callers'), also with the backward in two halves."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    ring = []
    for i in range(3):
        v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(64, answers=300, seed=80 + i))
        ring.append(({"v": v, "q_idxes": q}, a))
    keep = [(s["v"].clone(), s["q_idxes"].clone(), a.clone()) for s, a in ring]
    out = {}
    for slots in (1, 3):
        torch.manual_seed(21)
        tr = DataParallelTrainer(build("cor2", 300).train(), lr=2e-5, clip=0.25, graph=True, adopt_inputs=slots > 1,
                                 overlap=overlap, input_slots=slots)
        losses = []
        for i in range(14):
            loss, norm = tr.step(*ring[i % 3])
            losses.append((loss.clone(), norm.clone()))
        torch.cuda.synchronize()
        out[slots] = [(x.item(), n.item()) for x, n in losses]
        assert tr._graph is not None, "step was not captured"
        assert len(tr._slots) == slots
        if slots > 1:
            ptrs = {slot["sample"]["v"].data_ptr() for slot in tr._slots}
            assert ptrs == {s["v"].data_ptr() for s, _ in ring}           # every slot graph reads its batch in place
            assert bool(tr.overlap) == bool(overlap)
    for (s, a), (v0, q0, a0) in zip(ring, keep):                          # and nobody wrote the callers' tensors
        assert torch.equal(s["v"], v0) and torch.equal(s["q_idxes"], q0) and torch.equal(a, a0)
    for (l1, n1), (l3, n3) in zip(out[1], out[3]):
        assert abs(l1 - l3) <= 1e-5 * abs(l1) and abs(n1 - n3) <= 1e-4 * abs(n1), (out[1], out[3])


def test_graph_replays_queued_without_host_sync():
    """bench.py's flow: replays queued back to back with no host read in between, at the headline batch.  The loss and
    gradient norm read once at the end must equal those of the same steps launched kernel by kernel.  (Regression: a
    memset node -- hipMemsetAsync in K1/K3 backward, and inside torch's multi-block sum of the loss -- replays wrongly
    on ROCm 7.2; the step now contains none.)"""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    got = {}
    for mode in (False, True):
        model = build("cor2", 2000)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=mode)
        gen = torch.Generator(device="cpu").manual_seed(11)
        v = torch.randn(512, 36, 2048, generator=gen).to(dev())
        q = torch.randn(512, 2400, generator=gen).to(dev())
        a = torch.softmax(2.0 * torch.randn(512, 2000, generator=gen), dim=1).to(dev())
        for _ in range(12):
            loss, norm = tr.step({"v": v, "q_idxes": q}, a)
        torch.cuda.synchronize()
        got[mode] = (loss.item(), norm.item())
        if mode:
            assert tr._graph is not None, "step was not captured"
            nodes = tr.graph_nodes
            # (the whole step is in the two graphs: ~100 kernel nodes forward + backward in eval mode, 3 for clip + Adam)
            assert nodes["front"].get("kernel", 0) > 60 and nodes["tail"].get("kernel", 0) >= 3, nodes
            assert all(c.get("memset", 0) == 0 for c in nodes.values()), nodes
    (l0, n0), (l1, n1) = got[False], got[True]
    assert 100.0 < l0 < 2000.0, l0
    assert abs(l0 - l1) <= 1e-4 * abs(l0) and abs(n0 - n1) <= 1e-3 * abs(n0), (got[False], got[True])


def test_graph_replays_far_behind_the_host_keep_their_step_scalars():
    """The per-step Adam scalars (lr / bias corrections) and the dropout seed travel through an 8-slot pinned ring.  A host
    that runs more than 8 replays ahead of the GPU (here: 24 steps queued behind a device-side sleep) must not rewrite a
    slot before the GPU has copied it: the weights after the queued steps equal those of the same steps run one by one."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(8, answers=300, seed=71))
    updates = []
    for queued in (False, False, True):
        model = build("cor2", 300)                          # eval mode: no dropout
        tr = DataParallelTrainer(model, lr=1e-3, clip=0.25, gamma=0.9, graph=True)     # gamma 0.9: lr moves fast per step
        for _ in range(4):
            tr.step({"v": v, "q_idxes": q}, a)
        assert tr._graph is not None
        torch.cuda.synchronize()
        start = tr.flat.p.clone()
        if queued:
            torch.cuda._sleep(int(2.4e9))                   # ~1 s: every replay below is enqueued behind it
        for _ in range(24):
            tr.step({"v": v, "q_idxes": q}, a)
            if not queued:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        updates.append((tr.flat.p - start).double())
    # Two synchronised runs differ by the float atomics of the small-batch backward kernels, which Adam amplifies to a full
    # +-lr per step on the few weights whose gradient is near zero: element-wise that noise can reach the size of an update,
    # in the norm of the 24 steps' summed update it is ~1e-3.  A rewritten ring slot would apply lr * 0.9^8 = 0.43 lr in
    # EVERY weight's step: the summed update would move by tens of per cent in that norm.
    scale = updates[0].norm().item()
    noise = (updates[0] - updates[1]).norm().item() / scale
    diff = (updates[0] - updates[2]).norm().item() / scale
    assert diff <= max(5.0 * noise, 2e-2), (diff, noise)
    assert noise <= 2e-2, noise


def test_graph_trainer_respects_train_eval_switch():
    """Dropout is baked into the captured graphs: after model.eval() the trainer must not replay the train-mode graph."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    model = build("cor2", 300).train()
    torch.manual_seed(0)
    tr = DataParallelTrainer(model, lr=0.0, clip=0.25, graph=True)          # lr 0: the weights stay put
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(16, answers=300, seed=70))
    for _ in range(5):
        tr.step({"v": v, "q_idxes": q}, a)
    assert tr._graph is not None
    model.eval()
    l1 = tr.step({"v": v, "q_idxes": q}, a)[0].item()      # (a replayed step returns the graph's loss buffer: read it
    l2 = tr.step({"v": v, "q_idxes": q}, a)[0].item()      #  before the next step overwrites it)
    assert l1 == l2, "eval-mode steps must be deterministic (no dropout)"
    model.train()
    l3 = tr.step({"v": v, "q_idxes": q}, a)[0].item()
    l4 = tr.step({"v": v, "q_idxes": q}, a)[0].item()
    assert l3 != l4, "train-mode steps draw fresh masks"


def test_oda_graph_replay_draws_fresh_masks():
    """ODA in train mode: K2's dropout seed lives in device memory, so the step is graph-captured and every replay
    still draws a new mask (losses differ from step to step on identical data; same torch seed -> same sequence)."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer

    def run():
        torch.manual_seed(7)
        model = build("oda", 300).train()
        tr = DataParallelTrainer(model, lr=1e-6, clip=0.25, graph=True)
        v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(8, answers=300, seed=31))
        losses = [tr.step({"v": v, "q_idxes": q}, a)[0].item() for _ in range(8)]
        return losses, tr._graph is not None

    l1, graphed = run()
    l2, _ = run()
    assert graphed, "ODA train step should be graph-captured now that the mask seed is a device word"
    assert len(set(round(x, 4) for x in l1[3:])) > 2, l1          # replays do not repeat one frozen mask
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l1, l2)), (l1, l2)


@pytest.mark.gpu
def test_checkpoint_round_trip_and_torch_adam_interop(tmp_path):
    """train.py:250-284 on the GPU path: the three checkpoint files carry the reference's names, the optimizer file
    loads into a stock torch.optim.Adam over the same parameter list, and a replica that resumes from the files
    takes the same next steps (hipGraph-replayed) as the trainer that wrote them."""
    import os
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    model = build("cor2", 300)
    tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True)
    data = [tuple(torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(16, answers=300, seed=40 + i)) for i in range(9)]
    for v, q, a in data[:5]:
        tr.step({"v": v, "q_idxes": q}, a)
    assert tr._graph is not None
    path = tr.save_checkpoint({"epoch": 3, "exp_logger": None}, str(tmp_path))
    assert sorted(os.listdir(path)) == ["ckpt_info.pth.tar", "ckpt_model.pth.tar", "ckpt_optim.pth.tar"]
    saved = torch.load(os.path.join(path, "ckpt_model.pth.tar"))
    assert list(saved) == list(model.state_dict())
    assert all(not t.is_cuda for t in saved.values())

    # stock Adam accepts the optimizer file; its moments are the trainer's flat buffers, parameter by parameter
    optim_sd = torch.load(os.path.join(path, "ckpt_optim.pth.tar"))
    params = [p for p in model.parameters() if p.requires_grad]
    clones = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    adam = torch.optim.Adam(clones, lr=1e-4)
    adam.load_state_dict(optim_sd)
    where = {id(p): o for p, o in zip(tr.flat.params, tr.flat.offsets)}
    for p, c in zip(params, clones):
        st = adam.state[c]
        assert int(st["step"]) == 5
        o = where[id(p)]
        assert torch.equal(st["exp_avg"], tr.flat.m[o:o + p.numel()].view_as(p).cpu())
        assert torch.equal(st["exp_avg_sq"], tr.flat.v[o:o + p.numel()].view_as(p).cpu())

    # ... and stock Adam's own state dict (tensor-valued `step`) loads back into the fused optimizer unchanged
    m_before, v_before = tr.flat.m.clone(), tr.flat.v.clone()
    tr.load_optimizer_state_dict(adam.state_dict())
    assert tr.adam_steps == 5 and torch.equal(tr.flat.m, m_before) and torch.equal(tr.flat.v, v_before)

    # resume in a replica with other initial weights
    from vqa_playground_pytorch_amd import CoR2Model
    torch.manual_seed(7)
    other = CoR2Model(["PAD", "UNK"], 300).eval().to(dev())
    tr2 = DataParallelTrainer(other, lr=2e-5, clip=0.25, graph=True)
    assert tr2.load_checkpoint(path) is None
    for p, q in zip(model.parameters(), other.parameters()):
        assert torch.equal(p, q)
    assert tr2.adam_steps == 5 and tr2.iteration == 0
    tr.iteration = 0                       # the reference's schedule restarts on resume; Adam's step count does not
    for v, q, a in data[5:]:
        l1, n1 = tr.step({"v": v, "q_idxes": q}, a)
        l1, n1 = l1.item(), n1.item()
        l2, n2 = tr2.step({"v": v, "q_idxes": q}, a)
        assert abs(l1 - l2.item()) <= 1e-4 * abs(l1) and abs(n1 - n2.item()) <= 1e-4 * n1
    assert tr.lr == tr2.lr and tr2.adam_steps == 9
    for p, q in zip(model.parameters(), other.parameters()):
        assert (p - q).abs().max().item() <= 2e-3 * max(p.abs().max().item(), 1e-3)


@pytest.mark.gpu
def test_reset_optimizer_under_graph_replay():
    """learning_scheduler(cf) again (train.py:718-721) while the step is replayed from hipGraphs: the moments are zeroed
    in place, so the captured graphs stay valid and the next step equals the first step of a new trainer."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    import types
    # the rule of config/CoR2.py (restart_epoch None, keeping_epoch 40) at a step size that keeps +-lr sign flips of
    # near-zero gradients below the comparison threshold
    cf = types.SimpleNamespace(lr=2e-5, restart_epoch=None, keeping_epoch=40)
    model = build("cor2", 300)
    tr = DataParallelTrainer(model, lr=cf.lr, clip=0.25, graph=True)
    data = [tuple(torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(16, answers=300, seed=60 + i)) for i in range(6)]
    for v, q, a in data[:5]:
        tr.step({"v": v, "q_idxes": q}, a)
    assert tr._graph is not None
    assert tr.begin_epoch(1, cf) is True
    assert tr.adam_steps == 0 and tr.iteration == 0 and float(tr.flat.m.abs().max()) == 0.0
    twin = build("cor2", 300)
    twin.load_state_dict(model.state_dict())
    tr2 = DataParallelTrainer(twin, lr=cf.lr, clip=0.25, graph=False)
    v, q, a = data[5]
    l1, _ = tr.step({"v": v, "q_idxes": q}, a)          # replayed
    l2, _ = tr2.step({"v": v, "q_idxes": q}, a)         # eager, step 1 of a new optimizer
    assert abs(l1.item() - l2.item()) <= 1e-4 * abs(l2.item())
    assert tr.lr == tr2.lr
    for p, q_ in zip(model.parameters(), twin.parameters()):
        assert (p - q_).abs().max().item() <= 2e-3 * max(p.abs().max().item(), 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nans,kw", [("cor2", 2000, {}), ("cor2", 2000, {"relation_mode": 0}), ("oda", 3000, {}),
                                          ("cor2", 2000, {"compute_dtype": torch.bfloat16})])
def test_inference_without_grad(name, nans, kw):
    """eval() + torch.no_grad() (the reference's test / visu loops, train.py:139,:210; visu.py:188): every custom
    autograd Function of the path must also run when nothing requires a gradient, and give the same logits."""
    from vqa_playground_pytorch_amd import CoR2Model, ODAModel
    torch.manual_seed(0)
    model = {"cor2": CoR2Model, "oda": ODAModel}[name](["PAD"], nans, **kw).to(dev()).eval()
    for B in (1, 5, 64):
        v, q = torch.randn(B, 36, 2048, device=dev()), torch.randn(B, 2400, device=dev())
        with torch.no_grad():
            y = model({"v": v, "q_idxes": q})
            ad = model.alpha_dict
        y2 = model({"v": v, "q_idxes": q})
        assert y.shape == (B, nans) and torch.isfinite(y).all() and not y.requires_grad
        assert torch.allclose(y, y2, rtol=1e-4, atol=1e-5)
        for val in ad.values():
            for t in (val if isinstance(val, tuple) else (val,)):
                assert torch.isfinite(t).all() and not t.requires_grad


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("mode", [1, 0])
def test_two_half_backward_matches_single_pass(graph, mode):
    """DataParallelTrainer(overlap=...): backward stops at the tensors the second reasoning step reads from the first
    (CoR2Model.forward_with_cut), the late parameters' gradients are gathered (and, with more than one rank, all-reduced
    under the second half), then backward resumes.  Same losses, gradient norms and weights as the single-pass step --
    eager and hipGraph-replayed, closed-form and pairwise relation step."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    data = [tuple(torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(48, answers=300, seed=80 + i)) for i in range(7)]
    out = {}
    for overlap in (False, "force"):
        model = build("cor2", 300, relation_mode=mode)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=graph, overlap=overlap)
        assert tr.overlap == bool(overlap)
        traj = []
        for v, q, a in data:
            loss, norm = tr.step({"v": v, "q_idxes": q}, a)
            traj.append((loss.item(), norm.item()))
        if graph:
            assert tr._graph is not None, "step was not captured"
            if overlap:
                assert set(tr.graph_nodes) == {"front_a", "front_b", "tail"}
        out[overlap] = (traj, [p.detach().clone() for p in model.parameters()])
    for (l0, n0), (l1, n1) in zip(out[False][0], out["force"][0]):
        assert abs(l0 - l1) <= 1e-4 * abs(l0) and abs(n0 - n1) <= 1e-4 * max(abs(n0), 1e-6), (out[False][0], out["force"][0])
    for p0, p1 in zip(out[False][1], out["force"][1]):
        assert (p0 - p1).abs().max().item() <= 2e-3 * max(p0.abs().max().item(), 1e-3)


@pytest.mark.gpu
def test_late_parameters_cover_exactly_the_second_step():
    """The late bucket holds the parameters whose gradients are complete at the cut, contiguous at the head of the flat
    gradient buffer; every other parameter gets its gradient in the second half (none is missed, none is in both)."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    model = build("cor2", 300)
    tr = DataParallelTrainer(model, overlap="force")
    assert tr.overlap
    late, early = {id(p) for p in tr._late}, {id(p) for p in tr._early}
    assert not (late & early) and late | early == {id(p) for p in model.parameters()}
    names = {id(p): n for n, p in model.named_parameters()}
    assert all(names[i].split(".")[0] in ("compress_v2", "fusion_vq2", "att2", "fusion_final", "linear_classif") for i in late)
    assert max(tr.flat.offset_of(p) + p.numel() for p in tr._late) <= tr._split <= min(tr.flat.offset_of(p) for p in tr._early)
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(8, answers=300, seed=5))
    used = torch.zeros_like(tr.flat.g, dtype=torch.bool)        # (alignment gaps between segments belong to no parameter)
    for p in tr.flat.params:
        o = tr.flat.offset_of(p)
        used[o:o + p.numel()] = True
    tr.flat.g.fill_(float("nan"))
    tr._front_a({"v": v, "q_idxes": q}, a, device_seed=False)
    head = used.clone()
    head[tr._split:] = False
    assert torch.isfinite(tr.flat.g[head]).all()                   # late gradients are in place after the first half
    assert torch.isnan(tr.flat.g[used & ~head]).all()              # ... and nothing else has been touched yet
    tr._front_b()
    assert torch.isfinite(tr.flat.g[used]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_two_half_backward_oda(graph):
    """The same for ODA: the cut is behind the attention (fusion_final + classifier are the late bucket)."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    data = [tuple(torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(40, answers=300, seed=90 + i)) for i in range(6)]
    out = {}
    for overlap in (False, "force"):
        model = build("oda", 300)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=graph, overlap=overlap)
        assert tr.overlap == bool(overlap)
        traj = []
        for v, q, a in data:
            loss, norm = tr.step({"v": v, "q_idxes": q}, a)
            traj.append((loss.item(), norm.item()))
        if graph:
            assert tr._graph is not None, "step was not captured"
        out[overlap] = (traj, [p.detach().clone() for p in model.parameters()])
    for (l0, n0), (l1, n1) in zip(out[False][0], out["force"][0]):
        assert abs(l0 - l1) <= 1e-4 * abs(l0) and abs(n0 - n1) <= 1e-4 * max(abs(n0), 1e-6), (out[False][0], out["force"][0])
    for p0, p1 in zip(out[False][1], out["force"][1]):
        assert (p0 - p1).abs().max().item() <= 2e-3 * max(p0.abs().max().item(), 1e-3)


def test_trainer_switches_the_tuned_gemm_table_on():
    """DataParallelTrainer turns TunableOp on in look-up mode (no tuning at run time) and the shipped table is accepted by
    this box's libraries (its validator rows match), so the [B,*] layers of the BASELINE batch get their recorded solutions."""
    import torch.cuda.tunable as tn
    from vqa_playground_pytorch_amd import tuned_gemms
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    DataParallelTrainer(build("oda", 50).train(), lr=1e-4)
    assert tuned_gemms.enable() in ("1", "tune", "user")
    if tuned_gemms.enable() == "1":
        assert tn.is_enabled() and not tn.tuning_is_enabled()
        x = torch.randn(512, 510, device=dev())
        w = torch.randn(2000, 510, device=dev())
        b = torch.randn(2000, device=dev())
        torch.nn.functional.linear(x, w, b)                   # (TunableOp reads its table at the first GEMM)
        rows = [line.strip().split(",") for line in open(tuned_gemms.TABLE) if line.strip()]
        mine = {r[1]: r[2] for r in rows if r[0] == "Validator"}
        theirs = {k: v for k, v in tn.get_validators()}
        assert all(theirs.get(k) == v for k, v in mine.items()), (mine, theirs)
        assert len(tn.get_results()) >= 50


@pytest.mark.parametrize("cls,nans,head_mode", [("cor2", 300, "auto"), ("cor2", 300, "grouped"), ("oda", 300, "grouped")])
def test_pregated_gradients_have_a_single_consumer(cls, nans, head_mode, monkeypatch):
    """head.py's phases hand gradients over ALREADY multiplied by the producer's activation / dropout gate (the consumer holds
    the producer's stored output): QuestionProjections -> GatesAndRankFactors, GlimpseProjections -> VectorFusion,
    VectorFusion -> Classifier.  That is only sound while the handed-over tensor has no second consumer -- autograd would sum
    a gated and an ungated gradient.  The contract is checked on the graph the models really build: every output of those
    phase nodes is referenced by at most ONE next-function edge, and that edge comes from the phase that gates for it."""
    from vqa_playground_pytorch_amd import head
    monkeypatch.setattr(head, "MODE", head_mode)
    model = build(cls, nans).train()
    v, q, a = seeded.seeded_inputs(4, answers=nans, seed=21)
    logits = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    consumers, nodes = {}, {}            # (producer node name, its id, output index) -> [consumer node names]
    seen, stack = set(), [logits.grad_fn]
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        for nxt, idx in node.next_functions:
            if nxt is not None:
                consumers.setdefault((nxt.name(), id(nxt), idx), []).append(node.name())
                nodes[id(nxt)] = nxt
                stack.append(nxt)
    allowed = {"QuestionProjectionsBackward": {"GatesAndRankFactorsBackward"},
               "GlimpseProjectionsBackward": {"VectorFusionBackward"},
               "VectorFusionBackward": {"ClassifierBackward"}}
    checked = 0
    for (name, nid, idx), users in consumers.items():
        if name in allowed:
            # a group the producer was told is `ungated` (ODA's q_low, which the object-difference kernel reads as well)
            # receives plain gradients and gates them itself: any number of consumers
            ungated = nodes[nid].cfg[5] if name == "QuestionProjectionsBackward" else ()
            if idx in ungated:
                continue
            assert len(users) == 1 and users[0] in allowed[name], (name, idx, users)
            checked += 1
    assert checked >= (3 if cls == "cor2" else 2), (checked, sorted({k[0] for k in consumers}))


# ---- the same comparison with the product's relu decisions handed to the restatement: ALL 512 samples at RTOL -------------------
FLIP_FRACTION_F32 = 5e-6   # units per site where the float64 restatement's own gate differs from the product's (measured on the
#                            MI355X: 2 of 5 713 920 compress_v2 units = 3.5e-7, none anywhere else, CoR2 and ODA) ...
FLIP_EDGE_F32 = 1e-5       # ... and how far from zero its pre-activation may be there, in rms of the site's pre-activations
#                            (measured 3.8e-7: float32 rounding of a sum of 2048 products)
RTOL_FORCED_F32 = 2e-4     # with the gates equal: every gradient of the loss over all 512 samples (measured: 2.0e-5 CoR2, 5.5e-5 ODA)


@pytest.mark.parametrize("engine", ["split", "mfma"])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("cls,nans", [("cor2", 2000), ("oda", 3000)])
def test_baseline_batch_with_the_products_gates(cls, nans, mode, engine, monkeypatch, measured):
    """test_baseline_batch_against_oracle splits off the samples that own a relu unit within float32 rounding of zero (more
    than half of a CoR2 batch) and holds them to a looser bar, because a unit that falls on the other side of zero moves a
    whole row of a gradient.  Here that ONE ingredient is taken out instead: the product's own relu decisions at every relu
    site of the head (compress_v, compress_v2, the question projections, the glimpse projections) are recorded in the
    forward -- module hooks and wrappers around the calls that produce them -- and the float64 restatement multiplies its
    pre-activations by them instead of applying relu (its activation function is swapped for the duration of the run, in
    call order).  Asserted: the two sides decide differently at <= FLIP_FRACTION_F32 of a site's units and only where the
    restatement's |pre-activation| <= FLIP_EDGE_F32 rms (a wrong gate in the product would show here); and then logits and
    EVERY parameter gradient of the loss over ALL 512 samples agree at RTOL_FORCED_F32 = 2e-4 -- five times inside north_star's
    1e-3, no sample set aside.
    engine: the region projections on the split engine (the default, what bench.py's headline runs) and on the fp32 MFMA
    engine.  mode = train: the configuration the benchmark times -- dropout 0.5 at every site -- with the product's masks
    rebuilt from its seeds and handed to the restatement (forward_recording_masks), gates forced on top of that."""
    from vqa_playground_pytorch_amd import cor2 as cor2_mod
    from vqa_playground_pytorch_amd import head
    from vqa_playground_pytorch_amd import oda as oda_mod
    B = 512
    monkeypatch.setenv("VQA_F32_PRODUCTS", engine)
    model = build(cls, nans)
    if mode == "train":
        model.train()
    v, q, a = seeded.seeded_inputs(B, answers=nans, seed=512 if mode == "eval" else 514)
    rec, masks = {}, None
    hooks = [model.compress_v.register_forward_hook(lambda m, args, out: rec.__setitem__("compress_v", (out > 0).cpu()))]
    for name in (("att1", "att2") if cls == "cor2" else ("att",)):
        att = getattr(model, name)

        def attend(*args, _inner=att.attend, _name=name, **kw):
            res = _inner(*args, **kw)
            rec[_name + ".glimpses"] = (res[0] > 0).cpu()
            return res
        att.attend = attend
    if cls == "cor2":
        assert head.MODE == "auto"
        inner_q = head.QuestionProjections.apply

        def question_projections(*args, **kw):
            lows = inner_q(*args, **kw)
            rec["q_proj"] = [(t > 0).cpu() for t in lows]     # compress_q, linear_q, compress_q_1, compress_q_2
            return lows
        monkeypatch.setattr(head.QuestionProjections, "apply", question_projections)
        inner_rp = cor2_mod.ops.relation_projection

        def relation_projection(*args, **kw):
            out = inner_rp(*args, **kw)
            rec["compress_v2"] = (out > 0).cpu()
            return out
        monkeypatch.setattr(cor2_mod.ops, "relation_projection", relation_projection)
    else:
        inner_ml = oda_mod.my_linears

        def my_linears(mods, x, **kw):
            out = inner_ml(mods, x, **kw)
            if len(mods) == 2 and mods[0] is model.compress_q:
                rec["q_proj"] = [(out[0] > 0).cpu(), (out[1] > 0).cpu()]      # compress_q, linear_q
            return out
        monkeypatch.setattr(oda_mod, "my_linears", my_linears)
    try:
        if mode == "train":
            got, masks, _ = forward_recording_masks(model, cls, v, q)
        else:
            got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    finally:
        for h in hooks:
            h.remove()
        for name in (("att1", "att2") if cls == "cor2" else ("att",)):
            del getattr(model, name).attend
    RF.kld_sum_loss(got, torch.from_numpy(a).to(dev())).backward()
    # the restatement's relu sites in call order (oracle/reference_faithful.py: CoR2Oracle.forward / ODAOracle.forward)
    if cls == "cor2":
        assert set(rec) == {"compress_v", "compress_v2", "q_proj", "att1.glimpses", "att2.glimpses"}
        A = rec["att1.glimpses"].shape[1] // 4
        order = [("compress_q", rec["q_proj"][0]), ("compress_v", rec["compress_v"])] + \
            [("att1.glimpses", rec["att1.glimpses"][:, g * A:(g + 1) * A]) for g in range(4)] + \
            [("compress_q_1", rec["q_proj"][2], "expand_q_1"), ("compress_q_2", rec["q_proj"][3], "expand_q_2"),
             ("compress_v2", rec["compress_v2"])] + \
            [("att2.glimpses", rec["att2.glimpses"][:, g * A:(g + 1) * A]) for g in range(4)] + [("linear_q", rec["q_proj"][1])]
    else:
        assert set(rec) == {"compress_v", "q_proj", "att.glimpses"}
        A = rec["att.glimpses"].shape[1] // 4
        order = [("compress_v", rec["compress_v"]), ("compress_q", rec["q_proj"][0])] + \
            [("att.glimpses", rec["att.glimpses"][:, g * A:(g + 1) * A]) for g in range(4)] + [("linear_q", rec["q_proj"][1])]
    o64 = seeded.load_state({"cor2": RF.CoR2Oracle, "oda": RF.ODAOracle}[cls](nans), 0)
    o64 = (o64.train() if masks is not None else o64.eval()).double()
    flips, cursor, rng = {}, [0], [0, 0]
    if masks is not None:     # the restatement's own F.dropout off; every Drop* layer's input times the product's mask of that site
        sites = 0
        for name, mod in o64.named_modules():
            if isinstance(mod, (RF.DropLinear, RF.DropConv1x1)):
                assert mod.p == 0.5 and name in masks, name
                mod.p = None
                mod.register_forward_pre_hook(lambda _m, args, name=name: (args[0] * masks[name][rng[0]:rng[1]].double(),))
                sites += 1
        assert sites == len(masks) == {"cor2": 19, "oda": 9}[cls]
    activate = RF._activate

    def forced(x, af, dim):
        if af != "relu":
            return activate(x, af, dim)
        site, gate = order[cursor[0]][:2]
        consumer = order[cursor[0]][2] if len(order[cursor[0]]) > 2 else None
        cursor[0] += 1
        gate = gate[rng[0]:rng[1]].reshape(x.shape)
        xd = x.detach()
        if masks is not None and consumer is not None:
            # training mode: the grouped head hands these two projections over with the NEXT layer's input dropout already applied
            # (head.QuestionProjections), so the recorded sign is gate AND keep; where the unit was dropped its gate reaches
            # nothing (the restatement multiplies by the same mask right behind) -- the restatement's own decision stands there
            keep = masks[consumer][rng[0]:rng[1]].reshape(x.shape) > 0
            gate = torch.where(keep, gate, xd > 0)
        diff = (xd > 0) != gate
        rms = float(xd.pow(2).mean().sqrt())
        n, units, edge = flips.get(site, (0, 0, 0.0))
        flips[site] = (n + int(diff.sum()), units + diff.numel(),
                       max(edge, float(xd[diff].abs().max()) / rms if bool(diff.any()) else 0.0))
        return x * gate.to(x.dtype)

    params = [p for _, p in o64.named_parameters()]
    want = []
    RF._activate = forced
    try:
        for lo in range(0, B, 64):
            rng[0], rng[1], cursor[0] = lo, lo + 64, 0
            w64 = o64({"v": torch.from_numpy(v[lo:lo + 64]).double(), "q": torch.from_numpy(q[lo:lo + 64]).double()})
            assert cursor[0] == len(order)
            RF.kld_sum_loss(w64, torch.from_numpy(a[lo:lo + 64]).double()).backward()
            want.append(w64.detach())
    finally:
        RF._activate = activate
    for site, (n, units, edge) in sorted(flips.items()):
        print("  [%s] gates %-14s differ at %d of %d units (%.1e), largest |pre| / rms there %.1e" % (cls, site, n, units, n / units, edge))
        assert n <= max(1, FLIP_FRACTION_F32 * units) and edge <= FLIP_EDGE_F32, (site, n, units, edge)
    e_logits = rel(got, torch.cat(want).numpy())
    measured("logits rel err", e_logits, RTOL)
    assert e_logits <= RTOL
    worst = (0.0, "")
    for (n, p), po in zip(model.named_parameters(), params):
        g64, w64 = p.grad.detach().cpu().numpy().astype(np.float64), po.grad.numpy()
        assert np.isfinite(g64).all()
        err, scale = np.abs(g64 - w64).max(), np.abs(w64).max()
        # 2e-4 of the tensor's scale; the absolute floor ATOL_512 is for the gradients that are mathematically ZERO (a bias in
        # front of a softmax over regions: conv_att's, the region-side Mutan biases), where both sides hold rounding noise of a
        # sum over 512 x 36 rows -- a few 1e-7 in eval mode, up to 1e-6 with the dropout factors 2 of training mode
        assert err <= RTOL_FORCED_F32 * scale + ATOL_512, (cls, n, err, scale)
        e = err / (scale + ATOL_512 / RTOL_FORCED_F32)                  # (error on the tensor's scale)
        worst = max(worst, (e, n))
    print("[%s B=512 %s, %s engine, gates forced] all %d samples: worst gradient error %.2e of its tensor's scale (%s)"
          % (cls, mode, engine, B, worst[0], worst[1]))
    measured("worst gradient err / scale", worst[0], RTOL_FORCED_F32, worst[1])


def test_widen_bf16_is_exact():
    """ops.widen_bf16 (vqa_widen_bf16: the feed's bf16 transport of the regions into the fp32 path): every bf16 value -- all 65 536 bit
    patterns, NaNs' payloads included -- comes out as the fp32 with the same upper half, at sizes that are and are not a multiple
    of the kernel's eight elements per lane."""
    from vqa_playground_pytorch_amd import ops
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    for n in (65536, 65531, 8, 7, 1):
        src = bits[:n].view(torch.bfloat16).to(dev())
        got = ops.widen_bf16(src)
        want = (bits[:n].to(torch.int32) & 0xFFFF) << 16
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32).cpu(), want)
    x = torch.randn(3, 36, 2048).to(torch.bfloat16).to(dev())
    assert torch.equal(ops.widen_bf16(x), x.float())


@pytest.mark.parametrize("cls,nans", [("cor2", 2000), ("oda", 3000)])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_step_is_bitwise_reproducible_and_bf16_transport_is_the_fp32_step(cls, nans, mode):
    """Two things at the BASELINE batch, both asserted with torch.equal on the logits and on EVERY parameter gradient:
    (1) the step is bitwise reproducible from run to run (two fresh models, same seeded parameters, same inputs, same dropout
        seeds).  Rounds 1-5 were not: K3's backward added the 16 partial sums of every (region, glimpse) pair with LDS float atomics
        in arrival order, and every gradient upstream of the attention logits differed in its last bits between runs
        (tools/determinism_probe.py: 2e-7 ... 6e-7 of a tensor's scale).  Round 6 sums them in a fixed order
        (csrc/attention_pool.hip: a slot per wave).  [The small-batch form of that backward (B < VQA_K3_FUSED_MIN_B: 64 for fp32, 512 for bf16 regions) and the
        pairwise relation backward (relation_mode 0) still use float atomics.]
    (2) VERDICT r05 next #8: region features that cross PCIe as bf16 (feed.store_batches(region_dtype=torch.bfloat16): half the
        bytes of the step's dominant stream) enter the fp32 path through ONE exact widening pass (ops.widen_bf16); on features
        that are bf16-representable the bf16-fed step IS the fp32-fed step, bit for bit."""
    B = 512
    v, q, a = seeded.seeded_inputs(B, answers=nans, seed=77)
    v16 = torch.from_numpy(v).to(torch.bfloat16)
    out = {}
    for transport in ("f32", "f32_again", "bf16"):
        model = build(cls, nans)
        if mode == "train":
            model.train()
        torch.manual_seed(5)                    # (the fused masks' seeds are drawn from torch's CPU generator)
        vin = (v16 if transport == "bf16" else v16.float()).to(dev())
        logits = model({"v": vin, "q_idxes": torch.from_numpy(q).to(dev())})
        RF.kld_sum_loss(logits, torch.from_numpy(a).to(dev())).backward()
        out[transport] = (logits.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()})
    for other in ("f32_again", "bf16"):
        assert torch.equal(out["f32"][0], out[other][0]), other
        differ = [n for n in out["f32"][1] if not torch.equal(out["f32"][1][n], out[other][1][n])]
        assert not differ, (other, differ)
