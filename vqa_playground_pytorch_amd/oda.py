"""ODA ("Object-Difference Attention") head on the MI355X kernels -- drop-in for config/ODA.py:177-240.

Same constructor / forward / ``alpha_dict`` / state_dict names as the reference ``Model``
(``att.conv_att.conv.weight`` keeps its (4, N*310, 1) shape).  The [B,N,N*310] difference tensor and
its dropout mask are never built: HIP kernel K2 contracts them against the attention filter on the fly.
"""
import os

import torch

from . import head, ops
from .layers import MutanFusion, MyATT, MyConv1d, MyLinear, RegionQuestionModel, _rate, _seed, linear_stack_groups, my_linears, \
    question_feature


class Model(RegionQuestionModel):
    def __init__(self, vocab_words=None, num_ans=None, seq2vec=None, regions=36, encoder_dtype=None, encoder_input_dtype=None,
                 region_counts=False, encoder_length_aware=None):
        super().__init__()
        self.vocab_words = vocab_words
        self.num_classes = num_ans
        self.regions = regions
        # opt-in: read sample['v_len'] (int [B], 1..regions) and mask the object-difference kernel and the attention with it.
        # A different model, not only a faster one: the filter slot conv_att.weight[g, j*310:(j+1)*310] is then trained by the
        # samples with more than j regions only.  False: the key is refused, as before.
        self.region_counts = bool(region_counts)

        self._set_seq2vec(seq2vec, vocab_words, encoder_dtype, encoder_input_dtype, encoder_length_aware)
        self.compress_v = MyConv1d(2048, 310, 1, 1, p=0.5, af="relu")
        self.compress_q = MyLinear(2400, 310, p=0.5, af="relu")
        self.att = MyATT(fuse_dim=regions * 310, glimpses=4, inputs_dim=2048, att_dim=620, af="relu")
        self.linear_q = MyLinear(2400, 310, p=0.5, af="relu")
        self.fusion_final = MutanFusion(620, 310, 510, 5)
        self.linear_classif = MyLinear(510, self.num_classes, p=0.5)
        self.alpha_dict = {}
        self._mask_step = 0
        # compress_v's relu output feeds K2 and nothing else: K2's backward holds it in registers (for d q) and hands the
        # gradient back already multiplied by (output > 0), so the projection's weight-gradient kernel runs ungated
        # (VQA_ODA_GATE_IN_K2=0: the gate in the projection's own backward, as in round 2)
        self.compress_v.grad_pregated = os.environ.get("VQA_ODA_GATE_IN_K2", "1") == "1"

    def stack_groups(self):
        return linear_stack_groups([self.compress_q, self.linear_q])

    def difference_logits(self, v_feature_low, q_feature_low, lens=None):
        """config/ODA.py:216-222 + the dropout/1x1-conv of conv_att (config/ODA.py:149), fused (K2).
        lens (optional): int32 [B] device tensor of region counts (ops.region_counts): the masked K2."""
        conv = self.att.conv_att
        p = _rate(conv)
        w = conv.conv.weight.view(conv.out_channels, -1)
        return ops.object_difference_attention(v_feature_low, q_feature_low, w, conv.conv.bias, p, _seed(p),
                                               gate_dvl=self.compress_v.grad_pregated, lens=lens)

    def _grouped_head_ok(self, q_feature, cut):
        """As cor2.Model._grouped_head_ok: the [B,.]-sized layers as grouped phases (head.py)."""
        return (cut is None and q_feature.is_cuda and q_feature.dtype == torch.float32 and not q_feature.requires_grad
                and self.compress_q.af == "relu" and self.linear_q.af == "relu" and self.compress_q.p == self.linear_q.p
                and self.linear_classif.af in (None, "") and self.att.grouped_ok(q_feature)
                and head.supported("oda", q_feature.size(1), self.compress_q.out_features, self.fusion_final.hidden_dim,
                                   self.fusion_final.input_dim1, self.num_classes))

    def late_parameters(self):
        """Parameters behind the attention (fusion_final, the classifier: 3.9 M of the 7.3 M): their gradients are complete
        before backward enters the attention and the region projection (see cor2.CoR2Model.late_parameters)."""
        return [p for m in (self.fusion_final, self.linear_classif) for p in m.parameters()]

    def forward(self, sample, _cut=None):
        resident_counts = "v_idx" in sample and self.region_store is not None and self.region_store.counts is not None
        if ("v_len" in sample or "v_packed" in sample or resident_counts) and not self.region_counts:
            # (a packed batch is one with counts; so is a 'v_idx' batch whose resident store has them)
            # the attention weights of this model are indexed by region slot (fuse_dim = regions * 310): masking them changes
            # which samples train which slot, so the model reads the counts only when it was built to
            raise ValueError("ODA.Model takes no per-sample region counts: drop 'v_len' from the sample, or build the model "
                             "with region_counts=True (CoR2Model masks with it)")
        # 'v_len' (region_counts=True, optional): the masked K2 sums differences over the real rows only and writes exact zeros
        # on the padding, the masked K3 gives the padding alpha = 0; without the key the model runs unmasked.
        v_feature, v_len = self._region_input(sample, counts=self.region_counts)
        if v_feature.size(1) != self.regions:
            raise ValueError("ODA.Model was built for %d regions, input has %d" % (self.regions, v_feature.size(1)))
        q_feature = question_feature(self.seq2vec, sample["q_idxes"] if "q_idxes" in sample else sample["q"])

        v_feature_low = self.compress_v(v_feature)
        grouped = self._grouped_head_ok(q_feature, _cut)
        if grouped:
            # the [B,.]-sized layers as grouped phases (head.py): the two question projections (the object-difference kernel
            # reads the first one: its gradient comes back ungated), then fusion_final's question-side rank factors
            proj = [self.compress_q, self.linear_q]
            p_in = _rate(proj[0])
            q_feature_low, q_final = head.QuestionProjections.apply(
                q_feature.contiguous(), p_in, _seed(p_in), (), 0.0, 0, (0,),
                *[m.linear.weight for m in proj], *[m.linear.bias for m in proj])
            lin2 = list(self.fusion_final.list_linear2)
            (h2_final,) = head.GatesAndRankFactors.apply(2, (), ((1, self.fusion_final.R),), (1.0, 1.0), q_feature_low, q_final,
                                                         *[l.linear.weight for l in lin2], *[l.linear.bias for l in lin2])
        else:
            # the two MyLinear(2400 -> 310) on the question vector (config/ODA.py:185,193 applied at :207,:233): one batched GEMM
            q_both = my_linears([self.compress_q, self.linear_q], q_feature, group_first=True)   # [2,B,310]
            q_feature_low, q_final = ops.split_groups(q_both, (1, 1))                              # views; one cat kernel backward
        logits = self.difference_logits(v_feature_low, q_feature_low, lens=v_len)
        v_final, alphas, _ = self.att.attend(v_feature, logits, grouped=grouped, lens=v_len)

        self.alpha_dict = {"alphas": alphas[0].detach()}
        if grouped:
            return self._grouped_tail(h2_final, v_final)

        if _cut is not None:
            v_final, q_final = self._cut_aliases(_cut, [v_final, q_final])       # the cut is (attended features, q_final)
        x = self.fusion_final(v_final, q_final)
        return self.linear_classif(x)
