"""Per-sample region counts for ODA, the parts that need no GPU: the three `_len_` entry points of K2 exist in the header, the
binding and the library and refuse NULL pointers with nothing launched; oda.Model(region_counts=True) validates 'v_len' before
anything runs and the default model keeps refusing it; config.ODA.Model forwards the option; every VQA_LAUNCH site of
csrc/object_difference_masked.hip is the form of some GPU case of tests/test_gpu_oda_region_counts.py, and the reverse.  The
kernels and the model-level contract are that file's business: the layers have no CPU path to run them on."""
import ctypes
import os
import re

import pytest
import torch

from kernel_harness import forbid_launches
from vqa_playground_pytorch_amd import ODAModel, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, WS, BWD = ("vqa_object_difference_attention_len_fwd", "vqa_object_difference_attention_len_bwd_workspace_bytes",
                "vqa_object_difference_attention_len_bwd")


def test_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "vqa_mi355x.h"), encoding="utf-8") as fh:
        header = fh.read()
    L = _lib.lib()
    for name, ret, nargs in ((FWD, "int", 14), (WS, "size_t", 4), (BWD, "int", 20)):
        assert re.search(r"\b%s %s\(" % (ret, name), header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name), name
    # lens is the fifth pointer of both calls, in front of the outputs
    assert re.search(r"%s\((?:[^,]*,){4}\s*const int32_t\* lens," % FWD, header)
    assert re.search(r"%s\((?:[^,]*,){4}\s*const int32_t\* lens," % BWD, header)
    assert L.vqa_version() == 14 == _lib.ABI_VERSION
    assert "#define VQA_ABI_VERSION 14" in header
    assert L.vqa_object_difference_attention_len_bwd_workspace_bytes(512, 36, 310, 4) == \
        L.vqa_object_difference_attention_bwd_workspace_bytes(512, 36, 310, 4)


def _launched(L):
    return L.vqa_launch_log((ctypes.c_ulonglong * 16)(), 16)


def test_null_pointers_are_refused_without_a_gpu():
    L = _lib.lib()
    L.vqa_launch_log_reset()
    assert L.vqa_object_difference_attention_len_fwd(None, None, None, None, None, None, 0.5, 0, None, 2, 5, 8, 2, None) == -1
    assert b"null pointer" in L.vqa_last_error() and _launched(L) == 0
    assert L.vqa_object_difference_attention_len_bwd(None, None, None, None, None, None, None, None, None, None, 1 << 20,
                                                     0.5, 0, None, 2, 5, 8, 2, 0, None) == -1
    assert b"null pointer" in L.vqa_last_error() and _launched(L) == 0
    assert L.vqa_object_difference_attention_len_bwd_workspace_bytes(0, 5, 8, 2) == 0


def _sample(B=3, regions=36):
    return {"v": torch.zeros(B, regions, 2048), "q_idxes": torch.zeros(B, 2400)}


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bad", [0, 37, -3])
def test_oda_refuses_host_counts_outside_1_to_n_before_anything_runs(bad, dtype, monkeypatch):
    """the validation sits in front of every layer: with all of ops' launches made to fail the ValueError still comes first"""
    from vqa_playground_pytorch_amd import ops
    forbid_launches(monkeypatch, ops)
    model = ODAModel(["PAD", "UNK"], 50, region_counts=True).eval()
    monkeypatch.setattr(model.compress_v, "forward", lambda *a, **k: pytest.fail("a layer ran"))
    with pytest.raises(ValueError, match="1..36"):
        model(dict(_sample(), v_len=torch.tensor([36, bad, 1], dtype=dtype)))
    with pytest.raises(ValueError, match="v_len"):
        model(dict(_sample(), v_len=torch.tensor([36, 1], dtype=dtype)))            # [B - 1]
    with pytest.raises(ValueError, match="v_len"):
        model(dict(_sample(), v_len=torch.tensor([36.0, 1.0, 2.0])))               # not integers


def test_the_default_model_still_refuses_and_says_how_to_opt_in():
    model = ODAModel(["PAD", "UNK"], 50).eval()
    assert model.region_counts is False
    with pytest.raises(ValueError, match="v_len.*region_counts=True"):
        model(dict(_sample(), v_len=torch.tensor([36, 36, 36], dtype=torch.int32)))


def test_config_oda_model_forwards_the_option():
    import config.ODA
    assert config.ODA.Model(["PAD", "UNK"], 50, region_counts=True).region_counts is True
    assert config.ODA.Model(["PAD", "UNK"], 50).region_counts is False


def test_ops_refuse_bad_lens_without_a_gpu():
    """the lens check of ops.object_difference_attention needs a GPU tensor for vl first (no CPU path): that error comes first"""
    from vqa_playground_pytorch_amd import ops
    with pytest.raises(_lib.VqaLibraryError, match="GPU tensor"):
        ops.object_difference_attention(torch.zeros(2, 5, 8), torch.zeros(2, 8), torch.zeros(2, 40), torch.zeros(2),
                                        lens=torch.ones(2, dtype=torch.int32))


def test_every_launch_site_of_the_masked_file_is_declared():
    """a launch site added to (or renamed in) object_difference_masked.hip without a GPU case fails; so does a declared form
    that no launch site has.  The GPU file names a form where it asserts the launch log: forms_of() / bwd_log() return it"""
    import test_gpu_oda_kernels as unmasked
    import test_gpu_oda_region_counts as g
    sites = set(unmasked.launch_sites(os.path.join(ROOT, "vqa_playground_pytorch_amd", "csrc", "object_difference_masked.hip")))
    declared = set()
    for _, B, N, L, G, p, knobs, _, _ in g.CASES:
        declared |= set(g.forms_of(B, N, L, G, p, knobs)[:3])
    declared |= {g.REDUCE, g.DBIAS}
    assert sites - declared == set(), "launch sites that no case declares"
    assert declared - sites == set(), "declared forms that no launch site has"
    assert declared == {g.F_MFMA_T, g.F_MFMA_F, g.F_BIT, g.F_BYTE, g.F_PLAIN, g.D_SPLIT, g.D_BITS, g.D_BYTE, g.D_PLAIN,
                        g.W_MFMA_T, g.W_MFMA_F, g.W_BIT, g.W_BYTE, g.W_PLAIN, g.REDUCE, g.DBIAS}
