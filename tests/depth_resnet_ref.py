"""Plain-torch CPU restatement of the depth encoder of the CE agent (VlnResnetDepthEncoder around habitat-lab 0.1.7's
ResNetEncoder with resnet50, 32 base planes, 16 groups, no input normalisation), written from the architecture as
DESIGN.md section 7b states it, out of nn.Conv2d, nn.GroupNorm, F.avg_pool2d and F.max_pool2d; it runs in fp32 or fp64 and
shares no code with vln_bevbert_amd/depth_resnet.py.  Also the one place for the cases, the seeded weight rule and the seeded
depth images that tests/golden/make_depth_resnet_golden.py and the tests share.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

BASE, GROUPS, FLAT = 32, 16, 2048
# case -> (blocks per stage, input size, images, seed)
CASES = {"r50_256": ((3, 4, 6, 3), 256, 2, 201),
         "shallow_128": ((1, 1, 1, 1), 128, 3, 202)}


class Bottleneck(nn.Module):
    def __init__(self, cin, planes, stride, down):
        super().__init__()
        self.convs = nn.Sequential(
            nn.Conv2d(cin, planes, 1, bias=False), nn.GroupNorm(GROUPS, planes), nn.ReLU(),
            nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.GroupNorm(GROUPS, planes), nn.ReLU(),
            nn.Conv2d(planes, 4 * planes, 1, bias=False), nn.GroupNorm(GROUPS, 4 * planes))
        self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * planes, 1, stride, bias=False),
                                        nn.GroupNorm(GROUPS, 4 * planes)) if down else None

    def forward(self, x):
        return F.relu(self.convs(x) + (x if self.downsample is None else self.downsample(x)))


class Backbone(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(1, BASE, 7, 2, 3, bias=False), nn.GroupNorm(GROUPS, BASE), nn.ReLU())
        cin = BASE
        for i, n in enumerate(layers):
            planes = BASE * 2 ** i
            blocks = []
            for b in range(n):
                blocks.append(Bottleneck(cin, planes, 2 if (b == 0 and i > 0) else 1, b == 0))
                cin = 4 * planes
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.final_channels = cin

    def forward(self, x):
        x = F.max_pool2d(self.conv1(x), 3, 2, 1)
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))


class Encoder(nn.Module):
    def __init__(self, layers, size):
        super().__init__()
        self.backbone = Backbone(layers)
        s = int((size // 2) / 32)
        c = int(round(FLAT / s ** 2))
        self.compression = nn.Sequential(nn.Conv2d(self.backbone.final_channels, c, 3, 1, 1, bias=False), nn.GroupNorm(1, c),
                                         nn.ReLU())

    def forward(self, observations):
        x = observations["depth"].permute(0, 3, 1, 2)
        return self.compression(self.backbone(F.avg_pool2d(x, 2)))


class DepthRef(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), size=256):
        super().__init__()
        self.visual_encoder = Encoder(layers, size)

    def forward(self, observations):
        return self.visual_encoder(observations)


def shapes(layers=(3, 4, 6, 3), size=256):
    return {k: tuple(v.shape) for k, v in DepthRef(layers, size).state_dict().items()}


def state_dict(case):
    """Seeded weights: convolutions N(0, 2 / fan_in), GroupNorm gamma = 1 + 0.1 N(0, 1), beta = 0.1 N(0, 1)."""
    layers, size, _, seed = CASES[case]
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes(layers, size).items():
        r = torch.randn(s, generator=gen)
        if len(s) == 4:
            sd[k] = r * math.sqrt(2.0 / (s[1] * s[2] * s[3]))
        elif k.endswith(".weight"):
            sd[k] = 1.0 + 0.1 * r
        else:
            sd[k] = 0.1 * r
    return sd


def depth_images(seed, n, size):
    """Seeded (n, size, size, 1) fp32 in [0, 1]: a smooth ramp whose direction and offset differ per image, plus noise,
    clipped; one rectangle of exact zeros and one of exact ones per image, at places that differ per image."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, size), np.linspace(0, 1, size), indexing="ij")
    out = np.empty((n, size, size, 1), np.float32)
    for i in range(n):
        a, b, c = rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(0.3, 0.7)
        img = c + a * (yy - 0.5) + b * (xx - 0.5) + 0.15 * np.sin(6.0 * (xx + i) * (yy + 0.5)) + rng.normal(0, 0.05, (size, size))
        img = np.clip(img, 0.0, 1.0)
        q = size // 8
        y0, x0, y1, x1 = (int(v) for v in rng.integers(0, size - 2 * q, 4))
        img[y0:y0 + q, x0:x0 + 2 * q] = 0.0
        img[y1:y1 + 2 * q, x1:x1 + q] = 1.0
        out[i, :, :, 0] = img
    return torch.from_numpy(out)


_NETS = {}


def net(case, dtype=torch.float64):
    key = (case, dtype)
    if key not in _NETS:
        layers, size, _, _ = CASES[case]
        m = DepthRef(layers, size)
        m.load_state_dict(state_dict(case), strict=True)
        _NETS[key] = m.to(dtype).eval()
    return _NETS[key]


def run(case, dtype=torch.float64, autocast=False):
    """The case's output (n, C, s, s) on its own seeded images, computed once per (case, dtype, autocast)."""
    key = (case, dtype, autocast, "out")
    if key not in _NETS:
        _, size, n, seed = CASES[case]
        x = depth_images(seed, n, size).to(dtype)
        with torch.no_grad():
            if autocast:
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    y = net(case, dtype)({"depth": x})
            else:
                y = net(case, dtype)({"depth": x})
        _NETS[key] = y.double()
    return _NETS[key]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-300)))


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
