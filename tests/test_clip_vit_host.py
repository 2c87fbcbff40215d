"""CPU: tests/clip_ref.py (the plain-torch restatement the GPU tests lean on for shapes the golden does not hold) against
the reference's recorded outputs (tests/golden/clip_vit.npz, made by tests/golden/make_clip_vit_golden.py), and the
host-side interface of vln_bevbert_amd/clip_vit.py that needs no device."""
import os

import numpy as np
import pytest
import torch

from tests import clip_ref as R
from tests.helpers import read_shapes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "clip_vit.npz"))


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_equals_the_reference(gold, case):
    """1e-5 (max-abs / absmax) on x and on the stored sample of x_patch."""
    cfg, n, seed = R.CASES[case]
    with torch.no_grad():
        x, xp = R.forward(R.state_dict(cfg), cfg, R.transform(R.images(seed, n, cfg[0])))
    cols, toks = R.sample(xp)
    for name, got in (("x", x), ("xp_cols", cols), ("xp_toks", toks)):
        err = R.max_rel(got.numpy(), gold[f"{case}_{name}"])
        print(f"{case} {name}: max-abs / absmax {err:.3e}")
        assert err <= 1e-5, (case, name, err)


def test_golden_holds_attention_that_is_not_uniform_and_the_own_error_figures(gold):
    for case in R.CASES:
        assert float(gold[case + "_attn_row_max"]) >= 0.2
        for name in ("x", "xp_cols", "xp_toks"):
            f16, b16 = float(gold[f"{case}_fp16_rel_l2_{name}"]), float(gold[f"{case}_bf16_rel_l2_{name}"])
            print(f"{case} {name}: reference's own rel-L2 fp16 {f16:.3e} bf16 {b16:.3e}")
            assert 0 < f16 < b16 < 0.1


def test_key_list_and_weight_rule():
    shapes = read_shapes("clip_vit_keys.txt")
    assert list(shapes.items()) == list(R.shapes(R.KEYS_CONFIG).items())
    sd = R.state_dict(R.CASES["b16_l2"][0])
    g = sd["ln_pre.weight"]
    assert abs(float(g.mean()) - 1) < 0.02 and 0.05 < float(g.std()) < 0.15
    w = sd["transformer.resblocks.0.attn.in_proj_weight"]
    assert float(w[:1536].std()) > 3 * float(w[1536:].std())


def test_module_mirrors_the_reference_state_dict_and_refuses_what_the_kernels_cannot_take():
    from vln_bevbert_amd.clip_vit import ClipRGBEncoder, ClipVisionTransformer
    m = ClipVisionTransformer(*R.KEYS_CONFIG)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(read_shapes("clip_vit_keys.txt").items())
    cfg = R.CASES["b32_l2"][0]
    small = ClipVisionTransformer(*cfg)
    small.load_state_dict(R.state_dict(cfg), strict=True)
    assert not any(p.requires_grad for p in small.parameters()) and not small.training
    with pytest.raises(RuntimeError, match="finalize"):
        small(torch.zeros(1, 3, 224, 224))
    small.train()
    with pytest.raises(RuntimeError, match="forward-only"):
        small(torch.zeros(1, 3, 224, 224))
    with pytest.raises(ValueError, match="multiple of 256"):
        ClipVisionTransformer(224, 16, 384, 2, 6, 512)
    with pytest.raises(ValueError, match="must be 64"):
        ClipVisionTransformer(224, 16, 768, 2, 8, 512)
    enc = ClipRGBEncoder(224, 32, 768, 2, 12, 512)
    full = {"visual." + k: v for k, v in R.state_dict(cfg).items()}
    full.update({"transformer.resblocks.0.ln_1.weight": torch.ones(512), "token_embedding.weight": torch.zeros(8, 512),
                 "positional_embedding": torch.zeros(77, 512), "text_projection": torch.zeros(512, 512),
                 "logit_scale": torch.zeros(())})
    enc.load_clip_state_dict(full)
    assert torch.equal(enc.model.visual.positional_embedding, full["visual.positional_embedding"])
    with pytest.raises(KeyError):
        enc.load_clip_state_dict({"token_embedding.weight": torch.zeros(8, 512)})
