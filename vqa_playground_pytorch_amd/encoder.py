"""Question encoder slot ``seq2vec``: SkipThoughts = embedding(620) + BayesianGRU(620 -> 2400), the step in front of the
hot path (putils/__init__.py:878-985 SkipThoughts, :604-746 BayesianGRUCell / BayesianGRU, :503-539 SequentialDropout).

Same module tree and parameter names as the reference (``embedding.weight``, ``gru.gru_cell.weight_{ir,ii,in}.{weight,
bias}``, ``gru.gru_cell.weight_{hr,hi,hn}.weight``), so a reference checkpoint's ``seq2vec.*`` entries load.  The
uni-skip weight files the reference downloads at construction (putils/__init__.py:902-911) are not fetched here: pass
``pretrained={'utable': ..., 'dictionary': [...], 'uni_skip': {...}}`` to load them, otherwise the module is randomly
initialised.  Pure torch ops (library GEMMs) -- upstream of the path north_star names; what is restructured is the data
flow: the three input-side projections of all T steps are three [B*T,620]x[620,2400] GEMMs instead of 3*T small ones,
and the last valid state is gathered instead of masked-and-summed.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


def _af(name):
    return {"tanh": torch.tanh, "relu": F.relu, "sigmoid": torch.sigmoid}[name]


class _RecurrentProductBf16(torch.autograd.Function):
    """a = bf(hm) bf(W)^T with the backward of the mixed-precision contract (csrc/gru_bf16.hip) in torch ops: the incoming gradient
    is rounded to bf16 for the two products it feeds, d_hm = bf(g) bf(W) and d_W = bf(g)^T bf(hm); the roundings themselves are
    straight-through.  Operands keep their dtype (the bf16 VALUES in fp32 / fp64 storage), so the products accumulate in it.
    The input side's contract (csrc/encoder_input_bf16.hip) is the same function of (x * mx_g, W_ig): input_dtype=bfloat16 uses it
    for the three input projections."""

    @staticmethod
    def forward(ctx, hm, w):
        hb, wb = hm.to(torch.bfloat16).to(hm.dtype), w.to(torch.bfloat16).to(w.dtype)
        ctx.save_for_backward(hb, wb)
        return hb @ wb.t()

    @staticmethod
    def backward(ctx, g):
        hb, wb = ctx.saved_tensors
        gb = g.to(torch.bfloat16).to(g.dtype)
        return gb @ wb, gb.t() @ hb


class BayesianGRUCell(nn.Module):
    """putils/__init__.py:604-646 (+ AbstractGRUCell :566-584): six nn.Linear; bias only on the input side."""

    def __init__(self, input_size, hidden_size, bias_ih=True, bias_hh=False, dropout=0.25, af="tanh"):
        super().__init__()
        self.input_size, self.hidden_size, self.dropout, self.af = input_size, hidden_size, dropout, af
        self.weight_ir = nn.Linear(input_size, hidden_size, bias=bias_ih)
        self.weight_ii = nn.Linear(input_size, hidden_size, bias=bias_ih)
        self.weight_in = nn.Linear(input_size, hidden_size, bias=bias_ih)
        self.weight_hr = nn.Linear(hidden_size, hidden_size, bias=bias_hh)
        self.weight_hi = nn.Linear(hidden_size, hidden_size, bias=bias_hh)
        self.weight_hn = nn.Linear(hidden_size, hidden_size, bias=bias_hh)


class BayesianGRU(nn.Module):
    """putils/__init__.py:672-746.  The six dropout masks are drawn once per sequence and shared by all time steps
    (SequentialDropout); ``forward(x [B,T,in], lengths [B]) -> [B,hidden]`` = the state at step lengths-1."""

    def __init__(self, input_size, hidden_size, bias_ih=True, bias_hh=False, dropout=0.25, return_last=True, af="tanh",
                 compute_dtype=None, input_dtype=None, length_aware=False):
        super().__init__()
        # True: stop computing the time steps past each question's end (include/vqa_mi355x.h and INTEGRATION.md section 2 state
        # the contract): row b runs steps t < L[b] as ever and keeps its state afterwards.  With return_last=True the returned
        # vector and every gradient are the default's bit for bit; all_hiddens / the return_last=False output hold the last valid
        # state past a question's end where the default, as the reference, lets it evolve over PAD embeddings -- hence a choice.
        self.length_aware = bool(length_aware)
        # torch.bfloat16: the recurrent products in mixed precision (bf16 operands, fp32 accumulation; csrc/gru_bf16.hip states
        # the contract).  Parameters, state and the input side stay fp32 either way.
        self.compute_dtype = ops.parse_compute_dtype(compute_dtype)
        # torch.bfloat16: the INPUT side in mixed precision -- the embedded input (times its dropout mask) and the three input
        # weights rounded to bf16, fp32 accumulation, fp32 gi and biases (csrc/encoder_input_bf16.hip states the contract).  A
        # switch of its own: either value combines with either compute_dtype.
        self.input_dtype = ops.parse_compute_dtype(input_dtype, "input_dtype")
        self.input_size, self.hidden_size = input_size, hidden_size
        self.dropout, self.return_last, self.af = dropout, return_last, af
        self.gru_cell = BayesianGRUCell(input_size, hidden_size, bias_ih, bias_hh, dropout=dropout, af=af)
        self.all_hiddens = None

    def _mask(self, like):
        if not (self.training and self.dropout > 0):
            return None
        return torch.bernoulli(torch.full_like(like, 1.0 - self.dropout)) / (1.0 - self.dropout)

    def stack_groups(self):
        c = self.gru_cell
        inp, hid = (c.weight_ir, c.weight_ii, c.weight_in), (c.weight_hr, c.weight_hi, c.weight_hn)
        groups = [[m.weight for m in inp], [m.weight for m in hid]]
        if inp[0].bias is not None:
            groups.append([m.bias for m in inp])
        return groups

    def _takes_hip(self, is_cuda):
        # (the mixed-precision modes never fall back to fp32 products: a width their kernels do not take raises in ops)
        mixed = torch.bfloat16 in (self.compute_dtype, self.input_dtype)
        return bool(is_cuda and self.af in ("relu", "tanh") and self.gru_cell.weight_hr.bias is None
                    and (mixed or self.hidden_size % 4 == 0))

    def _forward_hip_input_bf16(self, x, lengths, table, padding_idx):
        """_forward_hip with the input side in mixed precision: ops.encoder_input_bf16 instead of the masked copy of the input and
        the batched fp32 GEMM.  x: the token ids [B,T] when `table` (the embedding's weight) is given -- the lookup then happens
        inside the pack kernel --, else the float input [B,T,K].  The six masks are drawn in the order of the fp32 path."""
        c = self.gru_cell
        inp, hid = (c.weight_ir, c.weight_ii, c.weight_in), (c.weight_hr, c.weight_hi, c.weight_hn)
        B, T = x.shape[:2]
        like = table if table is not None else x
        mx = mh = None
        if self.training and self.dropout > 0:
            proto = like.new_empty(B, 1, self.input_size)
            mx = torch.stack([self._mask(proto) for _ in range(3)], 2).view(B, 3, self.input_size)       # shared over time
            mh = torch.stack([self._mask(like.new_zeros(B, self.hidden_size)) for _ in range(3)])       # [3,B,H]
        w_in = ops.stack_params([m.weight for m in inp])
        b_in = ops.stack_params([m.bias for m in inp]) if inp[0].bias is not None else None
        if table is not None:
            gi = ops.encoder_input_bf16(table, x, mx, w_in, b_in, padding_idx)
        else:
            gi = ops.encoder_input_bf16(x, None, mx, w_in, b_in)
        out = ops.gru_sequence(gi, ops.stack_params([m.weight for m in hid]), mh, self.af, self.compute_dtype,
                               lens=self._steps(lengths, B, T, x.device))                                            # [T,B,H]
        if not self.return_last:
            return out.transpose(0, 1)
        self.all_hiddens = out.detach().transpose(0, 1)
        idx = (lengths.long() - 1) % T
        return out[idx, torch.arange(B, device=x.device)]

    def _steps(self, lengths, B, T, device):
        """The effective lengths L [B] of the length-aware mode (int32, on `device`; None when the mode is off): L[b] = len[b] if
        1 <= len[b] <= T, else T -- the (len - 1) % T rule of the gather: an all-PAD question runs every step.  Torch ops only:
        the host never reads it, a replayed graph recomputes it from the batch it is given."""
        if not self.length_aware:
            return None
        if lengths is None:
            return torch.full((B,), T, device=device, dtype=torch.int32)
        n = lengths.to(device=device, dtype=torch.int64)
        return torch.where((n >= 1) & (n <= T), n, torch.full_like(n, T)).to(torch.int32)

    def _forward_hip(self, x, lengths):
        """GPU form: the three input projections of all T steps as one batched GEMM, then ops.GruSequence (per step one
        batched recurrent GEMM + one gate kernel, csrc/gru.hip; compute_dtype and the step counts pick its products and entry
        points)."""
        c = self.gru_cell
        B, T, K = x.shape
        inp, hid = (c.weight_ir, c.weight_ii, c.weight_in), (c.weight_hr, c.weight_hi, c.weight_hn)
        xg = x.reshape(B * T, 1, K).expand(B * T, 3, K)                        # stride-0 gate axis
        if self.training and self.dropout > 0:
            mx = torch.stack([self._mask(x[:, :1, :]) for _ in range(3)], 2)   # [B,1,3,K]: shared over time
            xg = (x.unsqueeze(2) * mx).reshape(B * T, 3, K)
            mh = torch.stack([self._mask(x.new_zeros(B, self.hidden_size)) for _ in range(3)])   # [3,B,H]
        else:
            mh = None
        w_in = ops.stack_params([m.weight for m in inp])
        b_in = ops.stack_params([m.bias for m in inp]) if inp[0].bias is not None else None
        gi = ops.batched_linear(xg, w_in, b_in, group_first=True).view(3, B, T, self.hidden_size)
        out = ops.gru_sequence(gi, ops.stack_params([m.weight for m in hid]), mh, self.af, self.compute_dtype,
                               lens=self._steps(lengths, B, T, x.device))                                            # [T,B,H]
        if not self.return_last:
            return out.transpose(0, 1)
        self.all_hiddens = out.detach().transpose(0, 1)
        idx = (lengths.long() - 1) % T
        return out[idx, torch.arange(B, device=x.device)]

    def forward(self, x, lengths=None, table=None, padding_idx=None):
        """table (+ padding_idx): SkipThoughts' way into the mixed-precision input side on the GPU -- x is then the int64 token
        ids [B,T] and `table` the embedding's weight (only with input_dtype=bfloat16 on a device _takes_hip accepts)."""
        c, af = self.gru_cell, _af(self.af)
        bf16 = self.compute_dtype == torch.bfloat16
        in_bf16 = self.input_dtype == torch.bfloat16
        if table is not None and not (in_bf16 and self._takes_hip(x.is_cuda)):
            raise ValueError("BayesianGRU: token ids with a table are taken by the input_dtype=bfloat16 GPU path only")
        if in_bf16 and self._takes_hip(x.is_cuda):
            return self._forward_hip_input_bf16(x, lengths, table, padding_idx)
        B, T, _ = x.shape
        # (the mixed-precision mode never falls back to fp32 products: a width its kernels do not take raises in ops.gru_sequence)
        if x.is_cuda and self.af in ("relu", "tanh") and c.weight_hr.bias is None and (bf16 or self.hidden_size % 4 == 0):
            return self._forward_hip(x, lengths)

        def recurrent(lin, hm):        # the same contract in torch ops: CPU tests and gloo runs see the same function
            if not bf16:
                return lin(hm)
            a = _RecurrentProductBf16.apply(hm, lin.weight)
            return a if lin.bias is None else a + lin.bias
        mx = [self._mask(x[:, :1, :]) for _ in range(3)]                       # [B,1,in], shared over time
        h = x.new_zeros(B, self.hidden_size)
        mh = [self._mask(h) for _ in range(3)]                                 # [B,hidden]
        if in_bf16:                    # gi_g = bf(x m_g) bf(W_ig)^T + b_g: the input side's contract (csrc/encoder_input_bf16.hip)
            gi = []
            for lin, m in zip((c.weight_ir, c.weight_ii, c.weight_in), mx):
                g = _RecurrentProductBf16.apply((x if m is None else x * m).reshape(B * T, -1), lin.weight).view(B, T, -1)
                gi.append(g if lin.bias is None else g + lin.bias)
        else:
            gi = [ops.linear(x if m is None else x * m, lin.weight, lin.bias)                # (replay-safe bias gradient)
                  for lin, m in zip((c.weight_ir, c.weight_ii, c.weight_in), mx)]
        outs = []
        steps = self._steps(lengths, B, T, x.device)                           # length-aware: a row past its end keeps its state
        for t in range(T):
            hr, hi, hn = (h if m is None else h * m for m in mh)
            r = torch.sigmoid(gi[0][:, t] + recurrent(c.weight_hr, hr))
            i = torch.sigmoid(gi[1][:, t] + recurrent(c.weight_hi, hi))
            n = af(gi[2][:, t] + r * recurrent(c.weight_hn, hn))
            h_new = (1 - i) * n + i * h
            h = h_new if steps is None else torch.where((steps > t).unsqueeze(1), h_new, h)
            outs.append(h)
        output = torch.stack(outs, dim=1)                                      # [B,T,hidden]
        if not self.return_last:
            return output
        self.all_hiddens = output.detach()
        idx = (lengths.long() - 1) % T                                         # length 0 picks the last step, as mask[i][-1] does
        return output[torch.arange(B, device=x.device), idx]


def encoder_dtype_from(encoder_dtype):
    """The compute dtype of the encoder a model builds: the caller's ``encoder_dtype`` (validated), or, when that is None, the
    environment variable VQA_ENCODER_DTYPE (``f32``, the default, or ``bf16``), read here -- where the encoder is built."""
    if encoder_dtype is not None:
        return ops.parse_compute_dtype(encoder_dtype, "encoder_dtype")
    env = os.environ.get("VQA_ENCODER_DTYPE", "f32")
    if env not in ("f32", "bf16"):
        raise ValueError("VQA_ENCODER_DTYPE must be f32 or bf16, got %r" % (env,))
    return torch.bfloat16 if env == "bf16" else torch.float32


def encoder_input_dtype_from(encoder_input_dtype):
    """encoder_dtype_from for the encoder's INPUT side: the caller's ``encoder_input_dtype`` (validated), or, when that is None,
    the environment variable VQA_ENCODER_INPUT_DTYPE (``f32``, the default, or ``bf16``)."""
    if encoder_input_dtype is not None:
        return ops.parse_compute_dtype(encoder_input_dtype, "encoder_input_dtype")
    env = os.environ.get("VQA_ENCODER_INPUT_DTYPE", "f32")
    if env not in ("f32", "bf16"):
        raise ValueError("VQA_ENCODER_INPUT_DTYPE must be f32 or bf16, got %r" % (env,))
    return torch.bfloat16 if env == "bf16" else torch.float32


def encoder_length_aware_from(encoder_length_aware):
    """Whether the encoder a model builds is length-aware: the caller's ``encoder_length_aware`` (a bool), or, when that is None,
    the environment variable VQA_ENCODER_LENGTHS (``0``, the default, or ``1``), read here -- where the encoder is built."""
    if encoder_length_aware is not None:
        if not isinstance(encoder_length_aware, bool):
            raise ValueError("encoder_length_aware must be None, True or False, got %r" % (encoder_length_aware,))
        return encoder_length_aware
    env = os.environ.get("VQA_ENCODER_LENGTHS", "0")
    if env not in ("0", "1"):
        raise ValueError("VQA_ENCODER_LENGTHS must be 0 or 1, got %r" % (env,))
    return env == "1"


class SkipThoughts(nn.Module):
    """putils/__init__.py:878-985: ``forward(q_idxes int64 [B,T], 0 = PAD) -> [B,2400]``."""

    def __init__(self, vocab_list, data_dir=None, gru="BayesianGRU", return_last=True, af="tanh", pretrained=None,
                 compute_dtype=None, input_dtype=None, length_aware=False):
        super().__init__()
        if gru != "BayesianGRU":
            raise ValueError("only the BayesianGRU encoder of config/CoR2.py:166 / config/ODA.py:183 is provided")
        self.vocab_list, self.data_dir, self.af = vocab_list, data_dir, af
        self.embedding = nn.Embedding(num_embeddings=len(vocab_list), embedding_dim=620, padding_idx=0)
        self.gru = BayesianGRU(input_size=620, hidden_size=2400, dropout=0.25, return_last=return_last, af=af,
                               compute_dtype=compute_dtype, input_dtype=input_dtype, length_aware=length_aware)
        self.length_aware = self.gru.length_aware
        self.compute_dtype = self.gru.compute_dtype
        self.input_dtype = self.gru.input_dtype
        if pretrained is not None:
            self.load_pretrained(pretrained)

    def load_pretrained(self, pre):
        """pre = {'dictionary': list of words, 'utable': [n,620] array, 'uni_skip': mapping with encoder_W/Wx/b/bx/U/Ux}
        (the three files of putils/__init__.py:902-904); the mapping onto parameters follows :913-973."""
        word_to_vec = {w: pre["utable"][i] for i, w in enumerate(pre["dictionary"])}
        rows = [word_to_vec[w] if w in word_to_vec else word_to_vec["UNK"] for w in self.vocab_list]
        sk = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in pre["uni_skip"].items()}
        with torch.no_grad():
            self.embedding.weight.copy_(torch.as_tensor(rows, dtype=torch.float32).reshape(len(rows), 620))
            c = self.gru.gru_cell
            c.weight_ir.weight.copy_(sk["encoder_W"].t()[:2400])
            c.weight_ii.weight.copy_(sk["encoder_W"].t()[2400:])
            c.weight_in.weight.copy_(sk["encoder_Wx"].t())
            c.weight_ir.bias.copy_(sk["encoder_b"][:2400])
            c.weight_ii.bias.copy_(sk["encoder_b"][2400:])
            c.weight_in.bias.copy_(sk["encoder_bx"])
            c.weight_hr.weight.copy_(sk["encoder_U"].t()[:2400])
            c.weight_hi.weight.copy_(sk["encoder_U"].t()[2400:])
            c.weight_hn.weight.copy_(sk["encoder_Ux"].t())

    def forward(self, x, return_hidden=False):
        if x.dtype != torch.long:
            raise ValueError("SkipThoughts expects int64 token ids [B,T] (0 = PAD)")
        if self.input_dtype == torch.bfloat16 and self.gru._takes_hip(x.is_cuda):
            # the lookup, the input masks and the bf16 rounding are one kernel there: no fp32 [B,T,620] tensor
            lengths = x.size(1) - x.eq(0).sum(1)
            out = self.gru(x, lengths, table=self.embedding.weight, padding_idx=self.embedding.padding_idx)
            return (out, self.gru.all_hiddens) if return_hidden else out
        emb = ops.embedding(self.embedding.weight, x, self.embedding.padding_idx) if x.is_cuda else self.embedding(x)
        lengths = x.size(1) - x.eq(0).sum(1)
        out = self.gru(emb, lengths)
        return (out, self.gru.all_hiddens) if return_hidden else out
