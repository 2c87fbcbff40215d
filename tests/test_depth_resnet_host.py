"""CPU: tests/depth_resnet_ref.py (the plain-torch restatement the GPU tests are gated on) against its recorded fp64 outputs
(tests/golden/depth_resnet.npz, made by tests/golden/make_depth_resnet_golden.py), the key list, and the host-side interface of
vln_bevbert_amd/depth_resnet.py that needs no device.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

from tests import depth_resnet_ref as R
from tests.helpers import read_shapes
from vln_bevbert_amd.depth_resnet import DepthResNetEncoder

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
KEYS = "depth_resnet_keys.txt"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "depth_resnet.npz"))


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_reproduces_the_golden(gold, case):
    """1e-5 (max-abs / absmax), in fp64 again and in fp32 (whose recorded distance is 1.5e-6 .. 4.1e-6)."""
    err = R.max_rel(R.run(case).numpy(), gold[case + "_out"])
    err32 = R.max_rel(R.run(case, torch.float32).numpy(), gold[case + "_out"])
    print(f"{case}: fp64 max-abs / absmax {err:.3e}, fp32 {err32:.3e} (recorded {float(gold[case + '_fp32_max_rel']):.3e})")
    assert err <= 1e-5 and err32 <= 1e-5


def test_golden_is_not_degenerate(gold):
    for case, (_, _, n, _) in R.CASES.items():
        y = gold[case + "_out"]
        zf, f32, b16 = float(gold[case + "_zero_fraction"]), float(gold[case + "_fp32_rel_l2"]), float(gold[case + "_bf16_rel_l2"])
        apart = min(R.rel_l2(y[i], y[j]) for i in range(n) for j in range(i))
        print(f"{case}: zero fraction {zf:.3f} (stored) {float((y == 0).mean()):.3f} (output), images at least {apart:.3f} apart "
              f"(rel-L2), own rel-L2 fp32 {f32:.3e} bf16 {b16:.3e}")
        assert 0.2 < zf < 0.8 and abs(zf - float((y == 0).mean())) < 1e-12
        assert apart > 0.1
        assert 0 < f32 < b16 < 0.1


def test_depth_rule_has_its_exact_rectangles_and_distinct_images():
    d = R.depth_images(5, 3, 64)
    assert d.shape == (3, 64, 64, 1) and d.dtype == torch.float32 and float(d.min()) == 0.0 and float(d.max()) == 1.0
    for i in range(3):
        assert int((d[i] == 0).sum()) >= 8 * 8 and int((d[i] == 1).sum()) >= 8 * 8
        assert not torch.equal(d[i], d[(i + 1) % 3])


def test_state_dict_keys_and_shapes_equal_the_list_and_the_restatement():
    listed = list(read_shapes(KEYS).items())
    assert len(listed) == 162 and sum(k.startswith("visual_encoder.backbone.") for k, _ in listed) == 159
    m = DepthResNetEncoder()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == listed
    assert list(R.shapes().items()) == listed
    assert not any(p.requires_grad for p in m.parameters()) and not m.training
    backbone = sum(v.numel() for k, v in m.state_dict().items() if ".backbone." in k)
    print(f"backbone parameters {backbone}, compression convolution {m.visual_encoder.compression[0].weight.numel()}")
    assert 5.8e6 < backbone < 6.0e6 and m.visual_encoder.compression[0].weight.numel() == 128 * 1024 * 9
    shallow = DepthResNetEncoder(128, layers=(1, 1, 1, 1))
    assert [(k, tuple(v.shape)) for k, v in shallow.state_dict().items()] == list(R.shapes((1, 1, 1, 1), 128).items())
    assert shallow.output_shape == (512, 2, 2)


def test_output_shape_is_the_flatten_width_the_waypoint_predictor_checks(gold):
    from vln_bevbert_amd import waypoint as W
    m = DepthResNetEncoder()
    n = R.CASES["r50_256"][2]
    assert gold["r50_256_out"].shape == (n, 128, 4, 4) == (n,) + m.output_shape
    assert W.WaypointPredictor().visual_fc_depth[1].in_features == 128 * 4 * 4 == int(np.prod(m.output_shape))


def test_load_ddppo_state_dict_follows_the_checkpoint_key_rule():
    sd = R.state_dict("shallow_128")
    ckpt = {"actor_critic.net." + k: v for k, v in sd.items()}
    ckpt.update({"actor_critic.net.visual_fc.1.weight": torch.zeros(512, 2048), "actor_critic.net.visual_fc.1.bias": torch.zeros(512),
                 "actor_critic.net.prev_action_embedding.weight": torch.zeros(5, 32),
                 "actor_critic.action_distribution.linear.weight": torch.zeros(4, 512)})
    m = DepthResNetEncoder(128, layers=(1, 1, 1, 1))
    m.load_ddppo_state_dict(ckpt)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    missing = dict(ckpt)
    del missing["actor_critic.net.visual_encoder.backbone.layer2.0.convs.3.weight"]
    with pytest.raises(RuntimeError, match="layer2.0.convs.3.weight"):
        m.load_ddppo_state_dict(missing)
    with pytest.raises(RuntimeError):         # nothing of the encoder in it
        m.load_ddppo_state_dict({"actor_critic.net.visual_fc.1.weight": torch.zeros(512, 2048)})


def test_refusals():
    with pytest.raises(NotImplementedError, match="spatial_output: False"):
        DepthResNetEncoder(spatial_output=True)
    with pytest.raises(NotImplementedError, match="resnet50"):
        DepthResNetEncoder(backbone="resnet18")
    m = DepthResNetEncoder(128, layers=(1, 1, 1, 1))
    depth = torch.zeros(1, 128, 128, 1)
    with pytest.raises(RuntimeError, match="finalize"):
        m({"depth": depth})
    with pytest.raises(RuntimeError, match="finalize"):
        m.encode(depth)
    m.train()
    with pytest.raises(RuntimeError, match="forward-only"):
        m({"depth": depth})
    m.eval()
    feats = torch.ones(1, 512, 2, 2)
    assert m({"depth": depth, "depth_features": feats}) is feats


def test_load_state_dict_after_finalize_demands_a_new_finalize():
    """finalize() itself needs a device; what it leaves is stood in for, and both ways of loading weights retire it."""
    m = DepthResNetEncoder(128, layers=(1, 1, 1, 1))
    sd = R.state_dict("shallow_128")
    for load in (lambda: m.load_state_dict(sd, strict=True),
                 lambda: m.load_ddppo_state_dict({"actor_critic.net." + k: v for k, v in sd.items()})):
        m._c = {"dtype": torch.float32, "max_images": 4}
        load()
        assert m._c is None
        with pytest.raises(RuntimeError, match="finalize"):
            m.encode(torch.zeros(1, 128, 128, 1))
