"""Device-side depth ResNet encoder: the depth backbone of the continuous-environment (CE) agent's panorama views.

In mode 'waypoint' the reference pushes the 12 depth views of every environment through VlnResnetDepthEncoder
(bevbert_ce/vlnce_baselines/models/encoders/resnet_encoders.py:13-86, built at Policy_ViewSelection_BEV.py:119-125, called
at :189), whose network is habitat-lab's ResNetEncoder: avg_pool2d(2), a GroupNorm ResNet-50 of 32 base planes, and a 3x3
compression convolution that leaves (128, 4, 4) per 256 x 256 view.  That package is not part of the reference tree; the
network is restated in DESIGN.md section 7b.  Here the stage is a fixed sequence of launches on one stream with fixed
shapes and no host synchronisation, so it can be captured in a hipGraph between encode_panorama and waypoint_step:

    DepthResNetEncoder      VlnResnetDepthEncoder: same state_dict (visual_encoder.*), forward(observations)
    encode_observations     the ViT, the depth grid and this encoder on one clockwise view map

Arithmetic: activations are NHWC in the compute dtype (fp32 or bf16), so a 1x1 convolution is ops.linear on them as they
are; the 3x3 and the strided 1x1 convolutions run ops.linear on gathered rows; the stem convolution and every GroupNorm are
kernels of csrc/depth_resnet.hip with fp32 statistics.  GEMM outputs ("raw" below) are in the compute dtype.
Not built: spatial_output=True, other backbones than resnet50, running-mean input normalisation, fp16 operands, any
backward, a direct (implicit-GEMM) convolution kernel.
"""
import torch
import torch.nn as nn

from . import ops
from .clip_vit import NUM_VIEWS, _Holder, _want, clockwise_view_map, encode_panorama
from .lib import dtype_code, ptr, stream

GN_EPS = 1e-5
STEM_PLANES = 32            # the stem kernel's channel count
FLAT_SIZE = 2048            # ResNetEncoder's after_compression_flat_size


def _want_dtype(fn, name, t):
    if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.bfloat16) or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous float32 or bfloat16 tensor")


def _want_map(fn, view_map):
    if view_map is not None and (view_map.dtype != torch.int32 or view_map.dim() != 1 or not view_map.is_contiguous()):
        raise ValueError(f"{fn}: view_map is a contiguous int32 vector")


def gn_shape_ok(C, G):
    """The (channels, groups) the GroupNorm kernels take."""
    return 4 <= C <= 1024 and C & (C - 1) == 0 and 1 <= G <= 16 and G & (G - 1) == 0 and C % G == 0 and \
        (C // G == 2 or (C // G) % 4 == 0)


def gn_chunks(HW, C):
    """Blocks per image of the statistics kernel: 8192 values each, rows whole."""
    return -(-HW // (8192 // C))


def stem_weight(conv_weight):
    """Conv2d(1, 32, 7) weight (32, 1, 7, 7) -> the stem kernel's (49, 32) fp32 operand."""
    return conv_weight.detach().float().reshape(STEM_PLANES, 49).t().contiguous()


def stem_conv(depth, weight_t, view_map=None, out=None):
    """avg_pool2d(2) + the 7x7 stride-2 pad-3 convolution, fp32: depth (n_src, H, W, 1) -> raw (N, H / 4, W / 4, 32) NHWC;
    output image i reads input image view_map[i] (int32, device; None: the identity)."""
    fn = "stem_conv"
    if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.dim() != 4 or depth.shape[3] != 1 or \
            not depth.is_contiguous() or depth.shape[1] % 4 or depth.shape[2] % 4:
        raise ValueError(f"{fn}: contiguous float32 (N, H, W, 1) with H and W multiples of 4 expected")
    _want_map(fn, view_map)
    _want(fn, "weight_t", weight_t, torch.float32, (49, STEM_PLANES))
    n_src, H, W = depth.shape[:3]
    N = n_src if view_map is None else view_map.numel()
    if out is None:
        out = torch.empty(N, H // 4, W // 4, STEM_PLANES, dtype=torch.float32, device=depth.device)
    _want(fn, "out", out, torch.float32, (N, H // 4, W // 4, STEM_PLANES))
    ops.call("bevbert_dr_stem", ptr(depth), ptr(view_map), ptr(weight_t), ptr(out), N, n_src, H, W, stream())
    return out


def group_norm_stats(x, G, eps=GN_EPS, partial=None, out=None):
    """x (N, HW, C) fp32 or bf16 -> (mean, rstd), each (N, G) fp32.  ``partial``: fp32 scratch of at least
    N * gn_chunks(HW, C) * G * 2 values (allocated when missing and needed)."""
    fn = "group_norm_stats"
    _want_dtype(fn, "x", x)
    if x.dim() != 3 or not gn_shape_ok(x.shape[2], G):
        raise ValueError(f"{fn}: x (N, HW, C) with a supported (C, G) expected, got {tuple(x.shape)} G={G}")
    N, HW, C = x.shape
    chunks = gn_chunks(HW, C)
    need = N * chunks * G * 2 if chunks > 1 else 0
    if partial is None and need:
        partial = torch.empty(need, dtype=torch.float32, device=x.device)
    if need and (partial.dtype != torch.float32 or partial.numel() < need or not partial.is_contiguous()):
        raise ValueError(f"{fn}: partial must be a contiguous float32 tensor of at least {need} values")
    if out is None:
        out = (torch.empty(N, G, dtype=torch.float32, device=x.device), torch.empty(N, G, dtype=torch.float32, device=x.device))
    _want(fn, "mean", out[0], torch.float32, (N, G))
    _want(fn, "rstd", out[1], torch.float32, (N, G))
    ops.call("bevbert_dr_gn_stats", ptr(x), ptr(partial) if need else None, partial.numel() if need else 0, ptr(out[0]),
             ptr(out[1]), N, HW, C, G, eps, dtype_code(x), stream())
    return out


def _want_norm(fn, tag, stats, gamma, beta, N, C, G):
    _want(fn, tag + "mean", stats[0], torch.float32, (N, G))
    _want(fn, tag + "rstd", stats[1], torch.float32, (N, G))
    _want(fn, tag + "gamma", gamma, torch.float32, (C,))
    _want(fn, tag + "beta", beta, torch.float32, (C,))


def group_norm_apply(x, stats, gamma, beta, G, residual=None, other=None, nchw=False, out=None):
    """relu(gn(x) [+ residual | + gn(other)]) over x (N, HW, C) with stats = (mean, rstd) of group_norm_stats.  residual: a
    tensor like x; other: (raw tensor like x, its stats, gamma, beta) -- the downsample branch; nchw: write (N, C, HW)."""
    fn = "group_norm_apply"
    _want_dtype(fn, "x", x)
    if x.dim() != 3 or not gn_shape_ok(x.shape[2], G):
        raise ValueError(f"{fn}: x (N, HW, C) with a supported (C, G) expected, got {tuple(x.shape)} G={G}")
    if (residual is not None) + (other is not None) + bool(nchw) > 1:
        raise ValueError(f"{fn}: residual, other and nchw exclude each other")
    N, HW, C = x.shape
    _want_norm(fn, "", stats, gamma, beta, N, C, G)
    mode, r, s2, g2, b2 = 0, None, (None, None), None, None
    if residual is not None:
        mode, r = 1, residual
    elif other is not None:
        mode, (r, s2, g2, b2) = 2, other
        _want_norm(fn, "other ", s2, g2, b2, N, C, G)
    elif nchw:
        mode = 3
    if r is not None:
        _want(fn, "second tensor", r, x.dtype, (N, HW, C))
    shape = (N, C, HW) if nchw else (N, HW, C)
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    _want(fn, "out", out, x.dtype, shape)
    ops.call("bevbert_dr_gn_apply", ptr(x), ptr(stats[0]), ptr(stats[1]), ptr(gamma), ptr(beta), ptr(r), ptr(s2[0]), ptr(s2[1]),
             ptr(g2), ptr(b2), ptr(out), N, HW, C, G, mode, dtype_code(x), stream())
    return out


def group_norm_relu_maxpool(x, stats, gamma, beta, G, dtype, out=None):
    """The stem's form: raw x (N, H, W, C) fp32 -> relu(max_pool2d(gn(x), 3, 2, 1)) as (N, ceil(H / 2), ceil(W / 2), C) in
    ``dtype``."""
    fn = "group_norm_relu_maxpool"
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous() or not gn_shape_ok(x.shape[3], G):
        raise ValueError(f"{fn}: contiguous float32 (N, H, W, C) with a supported (C, G) expected")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{fn}: output dtype must be float32 or bfloat16")
    N, H, W, C = x.shape
    _want_norm(fn, "", stats, gamma, beta, N, C, G)
    shape = (N, (H + 1) // 2, (W + 1) // 2, C)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=x.device)
    _want(fn, "out", out, dtype, shape)
    ops.call("bevbert_dr_gn_relu_maxpool", ptr(x), ptr(stats[0]), ptr(stats[1]), ptr(gamma), ptr(beta), ptr(out), N, H, W, C, G,
             dtype_code(dtype), stream())
    return out


def gather_rows(x, ksize, stride, out=None):
    """Rows of a ksize x ksize convolution (3: padding 1; 1: none) with ``stride`` 1 or 2 on x (N, H, W, C):
    (N * Ho * Wo, ksize * ksize * C), column order (ky, kx, c), zeros outside the image."""
    fn = "gather_rows"
    _want_dtype(fn, "x", x)
    if x.dim() != 4 or ksize not in (1, 3) or stride not in (1, 2) or (x.shape[3] * x.element_size()) % 16:
        raise ValueError(f"{fn}: x (N, H, W, C) with C * element size a multiple of 16, ksize 1 or 3, stride 1 or 2 expected")
    N, H, W, C = x.shape
    shape = (N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), ksize * ksize * C)
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    _want(fn, "out", out, x.dtype, shape)
    ops.call("bevbert_dr_gather_rows", ptr(x), ptr(out), N, H, W, C, ksize, stride, dtype_code(x), stream())
    return out


# ----------------------------------------------------------------------------------------------------------------------
def _conv(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, bias=False)


class _Bottleneck(nn.Module):
    """convs = (1x1, GN, ReLU, 3x3 with the stride, GN, ReLU, 1x1, GN); downsample = (1x1 with the stride, GN) in the first
    block of a layer.  Holds the parameters under the reference's names; the arithmetic is DepthResNetEncoder.encode."""

    def __init__(self, cin, planes, groups, stride, downsample):
        super().__init__()
        self.cin, self.planes, self.stride = cin, planes, stride
        self.convs = nn.Sequential(_conv(cin, planes, 1), nn.GroupNorm(groups, planes), nn.ReLU(True),
                                   _conv(planes, planes, 3, stride), nn.GroupNorm(groups, planes), nn.ReLU(True),
                                   _conv(planes, 4 * planes, 1), nn.GroupNorm(groups, 4 * planes))
        if downsample:
            self.downsample = nn.Sequential(_conv(cin, 4 * planes, 1, stride), nn.GroupNorm(groups, 4 * planes))
        else:
            self.downsample = None


class DepthResNetEncoder(nn.Module):
    """VlnResnetDepthEncoder with the shipped arguments (resnet_encoders.py:14-32: backbone resnet50, 32 base planes,
    baseplanes // 2 groups, no input normalisation; spatial_output False, run_r2r/iter_train.yaml:63): the same state_dict
    keys and shapes under ``visual_encoder.``, every parameter frozen, always eval.  forward only; ``finalize`` builds the
    compute-dtype GEMM operands and every intermediate this module owns; there is no CPU path.  ``layers`` overrides the
    blocks per stage (resnet50: 3, 4, 6, 3)."""

    def __init__(self, input_size=256, baseplanes=32, backbone="resnet50", spatial_output=False, layers=(3, 4, 6, 3)):
        super().__init__()
        if backbone != "resnet50":
            raise NotImplementedError(f"DepthResNetEncoder: backbone {backbone!r} is not built; the shipped configuration uses "
                                      f"backbone='resnet50' (resnet_encoders.py:19)")
        if spatial_output:
            raise NotImplementedError("DepthResNetEncoder: spatial_output=True is not built; the shipped configuration uses "
                                      "spatial_output: False (run_r2r/iter_train.yaml:63)")
        if baseplanes != STEM_PLANES:
            raise ValueError(f"DepthResNetEncoder: the stem kernel is built for {STEM_PLANES} base planes, got {baseplanes}")
        if input_size % 64 or input_size < 64 or len(layers) != 4 or min(layers) < 1:
            raise ValueError("DepthResNetEncoder: a square input of a multiple of 64 pixels and four stages of at least one "
                             "block expected")
        self.input_size, self.baseplanes, self.groups, self.layers = input_size, baseplanes, baseplanes // 2, tuple(layers)
        self.final_spatial = int((input_size // 2) / 32)
        self.final_channels = baseplanes * 8 * 4
        self.out_channels = int(round(FLAT_SIZE / self.final_spatial ** 2))
        self.output_shape = (self.out_channels, self.final_spatial, self.final_spatial)
        G = self.groups
        enc = self.visual_encoder = _Holder()
        enc.backbone = _Holder()
        enc.backbone.conv1 = nn.Sequential(nn.Conv2d(1, baseplanes, 7, 2, 3, bias=False), nn.GroupNorm(G, baseplanes), nn.ReLU(True))
        cin = baseplanes
        for i, blocks in enumerate(self.layers):
            planes, stride = baseplanes << i, 1 if i == 0 else 2
            stage = [_Bottleneck(cin, planes, G, stride, True)]
            cin = 4 * planes
            stage += [_Bottleneck(cin, planes, G, 1, False) for _ in range(blocks - 1)]
            setattr(enc.backbone, f"layer{i + 1}", nn.Sequential(*stage))
        enc.compression = nn.Sequential(_conv(cin, self.out_channels, 3), nn.GroupNorm(1, self.out_channels), nn.ReLU(True))
        if not gn_shape_ok(self.out_channels, 1):
            raise ValueError(f"DepthResNetEncoder: {self.out_channels} compression channels unsupported")
        for p in self.parameters():
            p.requires_grad_(False)
        self._c = None
        self.eval()

    def _blocks(self):
        for i in range(4):
            yield from getattr(self.visual_encoder.backbone, f"layer{i + 1}")

    def _load_from_state_dict(self, *args, **kwargs):
        """New weights retire the compute-dtype operands finalize() built from the old ones (load_state_dict visits this
        module first; load_ddppo_state_dict, which loads the child, retires them itself)."""
        self._c = None
        return super()._load_from_state_dict(*args, **kwargs)

    def load_ddppo_state_dict(self, sd):
        """The reference's rule for a DD-PPO checkpoint's ['state_dict'] (resnet_encoders.py:41-47): split every key on '.',
        drop the first two parts, keep the entries whose next part is 'visual_encoder', strip it, load strictly."""
        own = {}
        for k, v in sd.items():
            parts = k.split(".")[2:]
            if parts and parts[0] == "visual_encoder":
                own[".".join(parts[1:])] = v.float()
        self._c = None
        return self.visual_encoder.load_state_dict(own, strict=True)

    # ------------------------------------------------------------------------------------------------------------------
    def finalize(self, device, compute_dtype=torch.float32, max_images=NUM_VIEWS):
        """Move the parameters to ``device``, build the GEMM operands in the compute dtype (a 1x1 weight as (out, in), a 3x3
        weight permuted to (out, ky, kx, in), the stem weight as (49, 32) fp32) and allocate the intermediates of up to
        ``max_images`` images once: the raw stem output, two block inputs / outputs, the normalised activation, the gathered
        rows, four statistics slots and their chunk scratch.  The outputs of the library GEMMs come from torch's caching
        allocator (ops.linear owns them), and so does the result, which belongs to the caller: after the first call nothing
        is taken from the device and nothing synchronises.  Loading other weights retires what finalize built."""
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("compute dtype must be float32 or bfloat16")
        self.to(device)
        for p in self.parameters():
            p.requires_grad_(False)
        cd, dev, M, G = compute_dtype, torch.device(device), int(max_images), self.groups

        def c1(conv):
            return conv.weight.detach().reshape(conv.weight.shape[0], -1).to(cd).contiguous()

        def c3(conv):
            return conv.weight.detach().permute(0, 2, 3, 1).reshape(conv.weight.shape[0], -1).to(cd).contiguous()
        bb = self.visual_encoder.backbone
        cc = {"dtype": cd, "max_images": M, "stem": stem_weight(bb.conv1[0].weight), "comp": c3(self.visual_encoder.compression[0]),
              "blocks": []}
        S = self.input_size // 4                       # spatial size after the stem convolution
        hw = (S // 2) ** 2                             # ... after the max pool
        x_el, h_el, col_el, part = hw * self.baseplanes, 0, 0, gn_chunks(S * S, self.baseplanes)
        for blk in self._blocks():
            cc["blocks"].append({"w1": c1(blk.convs[0]), "w2": c3(blk.convs[3]), "w3": c1(blk.convs[6]),
                                 "wd": c1(blk.downsample[0]) if blk.downsample is not None else None})
            hw_out = hw // blk.stride ** 2
            h_el = max(h_el, hw * blk.planes)
            col_el = max(col_el, hw_out * 9 * blk.planes, hw_out * blk.cin if blk.stride == 2 else 0)
            x_el = max(x_el, hw_out * 4 * blk.planes)
            part = max(part, gn_chunks(hw, blk.planes), gn_chunks(hw_out, 4 * blk.planes))
            hw = hw_out
        col_el = max(col_el, hw * 9 * self.final_channels)
        f32 = torch.float32
        cc["stem_raw"] = torch.empty(M * S * S * self.baseplanes, dtype=f32, device=dev)
        cc["x"] = [torch.empty(M * x_el, dtype=cd, device=dev) for _ in range(2)]
        cc["h"] = torch.empty(M * h_el, dtype=cd, device=dev)
        cc["cols"] = torch.empty(M * col_el, dtype=cd, device=dev)
        cc["stats"] = [(torch.empty(M * G, dtype=f32, device=dev), torch.empty(M * G, dtype=f32, device=dev)) for _ in range(4)]
        cc["partial"] = torch.empty(M * part * G * 2, dtype=f32, device=dev)
        self._c = cc
        self.eval()
        return self

    def _ready(self, n):
        if self.training:
            raise RuntimeError("DepthResNetEncoder is forward-only (the reference keeps it frozen in eval mode): call .eval()")
        if self._c is None:
            raise RuntimeError("DepthResNetEncoder: call finalize(device, compute_dtype, max_images) first -- there is no CPU path")
        if n > self._c["max_images"]:
            raise ValueError(f"DepthResNetEncoder: {n} images, finalize() allocated for {self._c['max_images']}")
        return self._c

    def encode(self, depth, view_map=None):
        """The hot path: depth (n_src, H, W, 1) fp32 in [0, 1] -> (N, 128, 4, 4) for 256 x 256 views, contiguous NCHW in the
        compute dtype.  ``view_map`` (int32, device): output image i is the encoding of input image view_map[i]."""
        if not torch.is_tensor(depth) or depth.dim() != 4:
            raise ValueError("DepthResNetEncoder: depth (N, H, W, 1) float32 expected")
        N = depth.shape[0] if view_map is None else view_map.numel()
        c = self._ready(N)
        if tuple(depth.shape[1:]) != (self.input_size, self.input_size, 1):
            raise ValueError(f"DepthResNetEncoder: ({self.input_size}, {self.input_size}, 1) depth images expected, got "
                             f"{tuple(depth.shape[1:])}")
        G, cd = self.groups, c["dtype"]
        bb = self.visual_encoder.backbone
        S = self.input_size // 4
        part = c["partial"]

        def stats(raw, n_hw, C, slot, groups=G):
            st = (c["stats"][slot][0][:N * groups].view(N, groups), c["stats"][slot][1][:N * groups].view(N, groups))
            return group_norm_stats(raw.view(N, n_hw, C), groups, GN_EPS, part, st)

        with torch.no_grad():
            raw = stem_conv(depth, c["stem"], view_map, out=c["stem_raw"][:N * S * S * self.baseplanes].view(N, S, S, self.baseplanes))
            gn = bb.conv1[1]
            st = stats(raw, S * S, self.baseplanes, 0)
            side, C, cur = S // 2, self.baseplanes, 0
            x = group_norm_relu_maxpool(raw, st, gn.weight, gn.bias, G, cd, out=c["x"][cur][:N * side * side * C].view(N, side, side, C))
            for blk, w in zip(self._blocks(), c["blocks"]):
                p, hw = blk.planes, side * side
                so = side // blk.stride
                hwo = so * so
                g1, g2, g3 = blk.convs[1], blk.convs[4], blk.convs[7]
                a = ops.linear(x.view(N * hw, C), blk.convs[0].weight, None, w_c=w["w1"])
                h = group_norm_apply(a.view(N, hw, p), stats(a, hw, p, 0), g1.weight, g1.bias, G, out=c["h"][:N * hw * p].view(N, hw, p))
                cols = gather_rows(h.view(N, side, side, p), 3, blk.stride, out=c["cols"][:N * hwo * 9 * p].view(N * hwo, 9 * p))
                b = ops.linear(cols, blk.convs[3].weight, None, w_c=w["w2"])
                h = group_norm_apply(b.view(N, hwo, p), stats(b, hwo, p, 1), g2.weight, g2.bias, G, out=c["h"][:N * hwo * p].view(N, hwo, p))
                y = ops.linear(h.view(N * hwo, p), blk.convs[6].weight, None, w_c=w["w3"])
                st3 = stats(y, hwo, 4 * p, 2)
                out = c["x"][1 - cur][:N * hwo * 4 * p].view(N, hwo, 4 * p)
                if blk.downsample is not None:
                    xin = x.view(N * hw, C) if blk.stride == 1 else \
                        gather_rows(x, 1, blk.stride, out=c["cols"][:N * hwo * C].view(N * hwo, C))
                    d = ops.linear(xin, blk.downsample[0].weight, None, w_c=w["wd"])
                    gd = blk.downsample[1]
                    group_norm_apply(y.view(N, hwo, 4 * p), st3, g3.weight, g3.bias, G,
                                     other=(d.view(N, hwo, 4 * p), stats(d, hwo, 4 * p, 3), gd.weight, gd.bias), out=out)
                else:
                    group_norm_apply(y.view(N, hwo, 4 * p), st3, g3.weight, g3.bias, G, residual=x.view(N, hw, C), out=out)
                side, C, cur = so, 4 * p, 1 - cur
                x = out.view(N, side, side, C)
            comp, gc = self.visual_encoder.compression, self.visual_encoder.compression[1]
            Co, hw = self.out_channels, side * side
            cols = gather_rows(x, 3, 1, out=c["cols"][:N * hw * 9 * C].view(N * hw, 9 * C))
            y = ops.linear(cols, comp[0].weight, None, w_c=c["comp"])
            res = group_norm_apply(y.view(N, hw, Co), stats(y, hw, Co, 0, 1), gc.weight, gc.bias, 1, nchw=True)
        return res.view(N, Co, side, side)

    def forward(self, observations):
        """The reference's signature (resnet_encoders.py:76-86): observations["depth"] (N, H, W, 1) fp32 -> (N, 128, 4, 4);
        observations["depth_features"], when present, is handed back as it is."""
        if "depth_features" in observations:
            return observations["depth_features"]
        return self.encode(observations["depth"].contiguous())


def encode_observations(rgb_encoder, depth_encoder, rgb_u8, depth, embeds_dtype=None):
    """Mode 'waypoint' in front of the predictor, both backbones: rgb_u8 (B, 12, R, R, 3) uint8 and depth (B, 12, H, W, 1)
    fp32 in the simulator's counter-clockwise view order -> {"rgb_embeds" (B * 12, 512), "rgb_grid" (B, 12, 196, 768) fp32,
    "depth_grid" (B, 12, 14, 14) fp32, "depth_embeds" (B * 12, 128, 4, 4)} in the reference's clockwise order; the embeddings
    are in the encoders' compute dtype and are what waypoint_step takes as they are.  One clockwise_view_map serves every
    stage.  Both encoders are finalized with max_images >= B * 12.  ``embeds_dtype`` is encode_panorama's: the dtype of
    "rgb_embeds" (None: the RGB encoder's compute dtype, fp32 for a float16 encoder)."""
    rgb_embeds, rgb_grid, depth_grid = encode_panorama(rgb_encoder, rgb_u8, depth, embeds_dtype)
    B = rgb_u8.shape[0]
    depth_embeds = depth_encoder.encode(depth.reshape((B * NUM_VIEWS,) + tuple(depth.shape[2:])),
                                        clockwise_view_map(B, depth.device))
    return {"rgb_embeds": rgb_embeds, "rgb_grid": rgb_grid, "depth_grid": depth_grid, "depth_embeds": depth_embeds}
