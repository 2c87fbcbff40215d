"""Device-side CLIP vision transformer: the image encoder of the continuous-environment (CE) agent's panorama views.

In mode 'waypoint' the reference pushes the 12 views of every environment through CLIPEncoderB16
(bevbert_ce/vlnce_baselines/models/encoders/resnet_encoders.py:280-314): uint8 RGB -> ConvertImageDtype + Normalize ->
VisionTransformer (ViT-B/16, encoders/clip/model.py:202-237), which returns the projected class vectors and the
14 x 14 x 768 patch grid; the depth images are pooled to the same grid (Policy_ViewSelection_BEV.py:127,190).  Here the
stage is a fixed sequence of launches on one stream with fixed shapes and no host synchronisation, so it can be captured
in a hipGraph in front of waypoint_step / CEGraphMap:

    ClipVisionTransformer   VisionTransformer, forward only, same constructor and state_dict
    ClipRGBEncoder          CLIPEncoderB16: .model.visual is the transformer, forward(observations)
    depth_grid_pool         AdaptiveAvgPool2d((14, 14)) of the depth images
    encode_panorama         both, with the reference's clockwise re-ordering of the views folded into the first kernels

Arithmetic: the residual stream is fp32 (csrc/vit.hip), the GEMM and attention operands are in the compute dtype (fp32,
bf16 or fp16); GEMMs go through ops.linear (hipBLASLt, cached plans), attention through ops.attention_self with batch =
images.  float16 is the operand precision the reference itself runs (convert_weights): its attention is the forward-only
instance of csrc/attn_fwd2.hip, and since the predictor takes fp32 / bf16 only, encode_panorama widens the fp16 class vectors.
The depth ResNet encoder is depth_resnet.py (encode_observations there runs both on one view map).
Not built: CLIP's text tower, an fp16 depth encoder or predictor, any backward.
"""
import ctypes

import torch
import torch.nn as nn

from . import ops
from .lib import dtype_code, ptr, stream

NUM_VIEWS = 12
GRID = 14
# transforms.Normalize of CLIPEncoder / CLIPEncoderB16 (resnet_encoders.py:266,302)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_MEAN_STD = (ctypes.c_float * 6)(*CLIP_MEAN, *CLIP_STD)
LN_EPS = 1e-5
# operand dtypes of the GEMMs and the attention; float16 is what the reference runs (clip/model.py convert_weights)
COMPUTE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class _Holder(nn.Module):
    """Bare container: gives parameters the reference's dotted names."""


class _LN(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(width))
        self.bias = nn.Parameter(torch.zeros(width))


class _Attn(nn.Module):
    """nn.MultiheadAttention's parameters: in_proj_weight is the packed q|k|v that ops.attention_self takes."""

    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.zeros(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)


class _Block(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.attn = _Attn(width)
        self.ln_1 = _LN(width)
        self.mlp = _Holder()
        self.mlp.c_fc = nn.Linear(width, 4 * width)
        self.mlp.c_proj = nn.Linear(4 * width, width)
        self.ln_2 = _LN(width)


def patchify(images_u8, patch_size, dtype, view_map=None, out=None):
    """uint8 (n_src, R, R, 3) -> normalised patch rows (N * g * g, 3 * P * P) in ``dtype``, column order (c, ky, kx);
    output image i reads input image view_map[i] (int32, device; None: the identity)."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3 or \
            images_u8.shape[1] != images_u8.shape[2] or not images_u8.is_contiguous():
        raise ValueError(f"patchify: contiguous uint8 (N, R, R, 3) expected, got {images_u8.dtype} {tuple(images_u8.shape)}")
    n_src, R, P = images_u8.shape[0], images_u8.shape[1], int(patch_size)
    if P not in (16, 32) or R % P:
        raise ValueError(f"patchify: patch size 16 or 32 dividing the resolution expected, got R={R} P={P}")
    if view_map is not None and (view_map.dtype != torch.int32 or not view_map.is_contiguous()):
        raise ValueError("patchify: view_map is a contiguous int32 tensor")
    N = n_src if view_map is None else view_map.numel()
    g = R // P
    if out is None:
        out = torch.empty(N * g * g, 3 * P * P, dtype=dtype, device=images_u8.device)
    ops.call("bevbert_vit_patchify", ptr(images_u8), ptr(view_map), ptr(out), N, n_src, R, P, _MEAN_STD, dtype_code(out),
             stream())
    return out


def _want(fn, name, t, dtype, shape):
    """The row kernels take raw pointers: a tensor of another dtype, shape or layout would be read or written out of bounds."""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)}" + ("" if t.is_contiguous() else " (not contiguous)") if torch.is_tensor(t) else type(t)
        raise ValueError(f"{fn}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {got}")


def _want_compute(fn, name, t):
    if not torch.is_tensor(t) or t.dtype not in COMPUTE_DTYPES or t.dim() != 2:
        raise ValueError(f"{fn}: {name} must be a float32, bfloat16 or float16 (rows, width) tensor")


def embed_prenorm(conv_out, class_embedding, pos, ln_pre, ln_1, L, z32=None, y=None, eps=LN_EPS):
    """Token assembly + ln_pre -> z32 (fp32 stream), ln_1 of the first block on it -> y (conv_out's dtype).  conv_out
    (N * (L - 1), H); class_embedding (H), pos (L, H), ln_pre / ln_1 = (weight, bias) of width H, all fp32."""
    fn, f32 = "embed_prenorm", torch.float32
    _want_compute(fn, "conv_out", conv_out)
    H = conv_out.shape[1]
    if L < 2 or conv_out.shape[0] % (L - 1):
        raise ValueError(f"{fn}: conv_out has {conv_out.shape[0]} rows, not a multiple of L - 1 = {L - 1}")
    N = conv_out.shape[0] // (L - 1)
    if z32 is None:
        z32 = torch.empty(N * L, H, dtype=f32, device=conv_out.device)
    if y is None:
        y = torch.empty(N * L, H, dtype=conv_out.dtype, device=conv_out.device)
    _want(fn, "conv_out", conv_out, conv_out.dtype, (N * (L - 1), H))
    _want(fn, "class_embedding", class_embedding, f32, (H,))
    _want(fn, "pos", pos, f32, (L, H))
    for name, t in (("ln_pre weight", ln_pre[0]), ("ln_pre bias", ln_pre[1]), ("ln_1 weight", ln_1[0]), ("ln_1 bias", ln_1[1])):
        _want(fn, name, t, f32, (H,))
    _want(fn, "z32", z32, f32, (N * L, H))
    _want(fn, "y", y, conv_out.dtype, (N * L, H))
    ops.call("bevbert_vit_embed_prenorm", ptr(conv_out), ptr(class_embedding), ptr(pos), ptr(ln_pre[0]), ptr(ln_pre[1]),
             ptr(ln_1[0]), ptr(ln_1[1]), ptr(z32), ptr(y), N, L, H, eps, dtype_code(conv_out), stream())
    return z32, y


def _want_residual(fn, z32, x, bias, gamma, beta):
    _want_compute(fn, "x", x)
    rows, H = x.shape
    _want(fn, "x", x, x.dtype, (rows, H))
    _want(fn, "z32", z32, torch.float32, (rows, H))
    for name, t in (("bias", bias), ("gamma", gamma), ("beta", beta)):
        _want(fn, name, t, torch.float32, (H,))
    return rows, H


def bias_residual_prenorm(z32, x, bias, gamma, beta, y=None, eps=LN_EPS):
    """z32 (rows, H) fp32 += x + bias in place; returns y = LayerNorm(z32) in x's dtype; bias, gamma, beta (H) fp32."""
    fn = "bias_residual_prenorm"
    rows, H = _want_residual(fn, z32, x, bias, gamma, beta)
    if y is None:
        y = torch.empty(rows, H, dtype=x.dtype, device=x.device)
    _want(fn, "y", y, x.dtype, (rows, H))
    ops.call("bevbert_vit_bias_residual_prenorm", ptr(z32), ptr(x), ptr(bias), ptr(gamma), ptr(beta), ptr(y), None, rows, 1,
             H, eps, 0, dtype_code(x), stream())
    return y


def bias_residual_final(z32, x, bias, gamma, beta, L, x_patch=None, cls_out=None, eps=LN_EPS):
    """The closing form: (x_patch (N, L - 1, H) fp32 = the patch rows of z32 + x + bias, cls_out (N, H) = ln_post of the
    class rows in x's dtype).  z32 itself is left as it was."""
    fn = "bias_residual_final"
    rows, H = _want_residual(fn, z32, x, bias, gamma, beta)
    if L < 2 or rows % L:
        raise ValueError(f"{fn}: {rows} rows are not a whole number of images of L = {L} tokens")
    N = rows // L
    if x_patch is None:
        x_patch = torch.empty(N, L - 1, H, dtype=torch.float32, device=x.device)
    if cls_out is None:
        cls_out = torch.empty(N, H, dtype=x.dtype, device=x.device)
    _want(fn, "x_patch", x_patch, torch.float32, (N, L - 1, H))
    _want(fn, "cls_out", cls_out, x.dtype, (N, H))
    ops.call("bevbert_vit_bias_residual_prenorm", ptr(z32), ptr(x), ptr(bias), ptr(gamma), ptr(beta), ptr(cls_out),
             ptr(x_patch), rows, L, H, eps, 1, dtype_code(x), stream())
    return x_patch, cls_out


def bias_quickgelu(x, bias, out=None):
    """(x + bias) * sigmoid(1.702 (x + bias)) over (rows, C) in x's dtype, fp32 math; bias (C) fp32, C a multiple of 4."""
    fn = "bias_quickgelu"
    _want_compute(fn, "x", x)
    rows, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    _want(fn, "x", x, x.dtype, (rows, C))
    _want(fn, "bias", bias, torch.float32, (C,))
    _want(fn, "out", out, x.dtype, (rows, C))
    ops.call("bevbert_vit_bias_quickgelu", ptr(x), ptr(bias), ptr(out), rows, C, dtype_code(x), stream())
    return out


def depth_grid_pool(depth, view_map=None, grid=GRID, out=None):
    """AdaptiveAvgPool2d((grid, grid)) of depth images (n_src, Hd, Wd, 1) fp32 -> (N, grid, grid) fp32; view_map as in
    patchify."""
    if depth.dtype != torch.float32 or depth.dim() != 4 or depth.shape[3] != 1 or not depth.is_contiguous():
        raise ValueError(f"depth_grid_pool: contiguous float32 (N, Hd, Wd, 1) expected, got {depth.dtype} {tuple(depth.shape)}")
    if view_map is not None and (view_map.dtype != torch.int32 or not view_map.is_contiguous()):
        raise ValueError("depth_grid_pool: view_map is a contiguous int32 tensor")
    n_src = depth.shape[0]
    N = n_src if view_map is None else view_map.numel()
    if out is None:
        out = torch.empty(N, grid, grid, dtype=torch.float32, device=depth.device)
    ops.call("bevbert_depth_grid_pool", ptr(depth), ptr(view_map), ptr(out), N, n_src, depth.shape[1], depth.shape[2], grid,
             stream())
    return out


class ClipVisionTransformer(nn.Module):
    """encoders/clip/model.py VisionTransformer: same constructor, same state_dict keys and shapes (strict=True loads the
    ``visual.*`` part of a CLIP checkpoint), forward only.  Frozen and always eval in the reference
    (resnet_encoders.py:295-297); a call in training mode raises.  ``finalize`` builds the compute-dtype operands and every
    intermediate this module owns; there is no CPU path."""

    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        if width % 256 or not 256 <= width <= 1024:
            raise ValueError(f"ClipVisionTransformer: width {width} unsupported: the row kernels take a multiple of 256 up to 1024")
        if heads * 64 != width:
            raise ValueError(f"ClipVisionTransformer: width / heads must be 64 (the attention kernels' head size), got "
                             f"{width} / {heads}")
        if patch_size not in (16, 32) or input_resolution % patch_size:
            raise ValueError("ClipVisionTransformer: patch size 16 or 32 dividing the input resolution expected")
        self.input_resolution, self.patch_size, self.width = input_resolution, patch_size, width
        self.layers, self.heads, self.output_dim = layers, heads, output_dim
        self.grid = input_resolution // patch_size
        self.tokens = self.grid ** 2 + 1
        self.conv1 = nn.Conv2d(3, width, patch_size, patch_size, bias=False)
        # every parameter is loaded (strict=True): the module is frozen and has no initialisation of its own
        self.class_embedding = nn.Parameter(torch.zeros(width))
        self.positional_embedding = nn.Parameter(torch.zeros(self.tokens, width))
        self.ln_pre = _LN(width)
        self.transformer = _Holder()
        self.transformer.resblocks = nn.ModuleList([_Block(width) for _ in range(layers)])
        self.ln_post = _LN(width)
        self.proj = nn.Parameter(torch.zeros(width, output_dim))
        for p in self.parameters():
            p.requires_grad_(False)
        self._c = None
        self.eval()

    def _load_from_state_dict(self, *args, **kwargs):
        """New weights retire the compute-dtype operands finalize() built from the old ones: the next call asks for
        finalize() instead of running old GEMM operands with new biases."""
        self._c = None
        return super()._load_from_state_dict(*args, **kwargs)

    # ------------------------------------------------------------------------------------------------------------------
    def finalize(self, device, compute_dtype=torch.float32, max_images=NUM_VIEWS):
        """Move the parameters to ``device``, build the compute-dtype GEMM operands (conv1.weight as (width, 3 P P), the
        packed in_proj_weight as it is, proj transposed) and allocate the intermediates of up to ``max_images`` images
        once (patch rows, the fp32 stream, the LayerNorm output, the MLP activation, the normalised class rows).  The
        outputs of the library GEMMs and of the attention come from torch's caching allocator (ops.linear /
        ops.attention_self own them), and so do the two results, which belong to the caller: after the first call nothing
        is taken from the device and nothing synchronises.  Loading other weights retires what finalize built: call it
        again."""
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError("compute dtype must be float32, bfloat16 or float16")
        self.to(device)
        for p in self.parameters():
            p.requires_grad_(False)
        cd, dev = compute_dtype, torch.device(device)
        W, L, M = self.width, self.tokens, int(max_images)

        def c(t):
            return t.detach().to(cd).contiguous()
        cc = {"dtype": cd, "max_images": M, "conv": c(self.conv1.weight.view(W, -1)), "proj_t": c(self.proj.t()), "layers": []}
        for blk in self.transformer.resblocks:
            cc["layers"].append({"qkv": c(blk.attn.in_proj_weight), "qkv_b": c(blk.attn.in_proj_bias),
                                 "out": c(blk.attn.out_proj.weight), "fc": c(blk.mlp.c_fc.weight),
                                 "proj": c(blk.mlp.c_proj.weight)})
        cc["patches"] = torch.empty(M * (L - 1), 3 * self.patch_size ** 2, dtype=cd, device=dev)
        cc["z32"] = torch.empty(M * L, W, dtype=torch.float32, device=dev)
        cc["y"] = torch.empty(M * L, W, dtype=cd, device=dev)
        cc["act"] = torch.empty(M * L, 4 * W, dtype=cd, device=dev)
        cc["cls"] = torch.empty(M, W, dtype=cd, device=dev)
        self._c = cc
        self.eval()
        return self

    def _ready(self, n):
        if self.training:
            raise RuntimeError("ClipVisionTransformer is forward-only (the reference keeps it frozen in eval mode): call .eval()")
        if self._c is None:
            raise RuntimeError("ClipVisionTransformer: call finalize(device, compute_dtype, max_images) first -- there is no CPU path")
        if n > self._c["max_images"]:
            raise ValueError(f"ClipVisionTransformer: {n} images, finalize() allocated for {self._c['max_images']}")
        return self._c

    def _encode_patches(self, patches, N):
        """Patch rows (N * g * g, 3 P P) in the compute dtype -> (x (N, output_dim) compute dtype, x_patch (N, g * g, width)
        fp32)."""
        c = self._c
        W, L, nh = self.width, self.tokens, self.heads
        rows = N * L
        z32, y, act = c["z32"][:rows], c["y"][:rows], c["act"][:rows]
        blocks = self.transformer.resblocks
        with torch.no_grad():
            conv = ops.linear(patches, self.conv1.weight, None, w_c=c["conv"])
            embed_prenorm(conv, self.class_embedding, self.positional_embedding, (self.ln_pre.weight, self.ln_pre.bias),
                          (blocks[0].ln_1.weight, blocks[0].ln_1.bias), L, z32, y)
            for i, (blk, lc) in enumerate(zip(blocks, c["layers"])):
                qkv = ops.linear(y, blk.attn.in_proj_weight, blk.attn.in_proj_bias, w_c=lc["qkv"], b_c=lc["qkv_b"])
                a = ops.attention_self(qkv.view(N, L, 3 * W), None, None, nh)
                o = ops.linear(a.view(rows, W), blk.attn.out_proj.weight, None, w_c=lc["out"])
                bias_residual_prenorm(z32, o, blk.attn.out_proj.bias, blk.ln_2.weight, blk.ln_2.bias, y)
                h = ops.linear(y, blk.mlp.c_fc.weight, None, w_c=lc["fc"])
                bias_quickgelu(h, blk.mlp.c_fc.bias, act)
                o = ops.linear(act, blk.mlp.c_proj.weight, None, w_c=lc["proj"])
                if i + 1 < len(blocks):
                    nxt = blocks[i + 1].ln_1
                    bias_residual_prenorm(z32, o, blk.mlp.c_proj.bias, nxt.weight, nxt.bias, y)
            x_patch, cls = bias_residual_final(z32, o, blocks[-1].mlp.c_proj.bias, self.ln_post.weight, self.ln_post.bias, L,
                                               cls_out=c["cls"][:N])
            x = ops.linear(cls, self.proj, None, w_c=c["proj_t"])
        return x, x_patch

    def encode_u8(self, images_u8, view_map=None):
        """The fused entry: uint8 (n_src, R, R, 3) images -> (x, x_patch); ConvertImageDtype + Normalize happen inside the
        patch kernel.  ``view_map`` (int32, device): output image i is the encoding of input image view_map[i]."""
        N = images_u8.shape[0] if view_map is None else view_map.numel()
        c = self._ready(N)
        if images_u8.shape[1] != self.input_resolution:
            raise ValueError(f"ClipVisionTransformer: {self.input_resolution} x {self.input_resolution} images expected")
        rows = N * (self.tokens - 1)
        patches = patchify(images_u8, self.patch_size, c["dtype"], view_map, out=c["patches"][:rows])
        return self._encode_patches(patches, N)

    def forward(self, x):
        """The reference's signature: normalised float images (N, 3, R, R) -> (x (N, output_dim), x_patch (N, g * g,
        width)).  The patch rows are cut with torch views (one copy); the hot path is encode_u8."""
        N, P, g = x.shape[0], self.patch_size, self.grid
        c = self._ready(N)
        if tuple(x.shape[1:]) != (3, self.input_resolution, self.input_resolution):
            raise ValueError(f"ClipVisionTransformer: (N, 3, {self.input_resolution}, {self.input_resolution}) expected")
        rows = x.reshape(N, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N * g * g, 3 * P * P).to(c["dtype"])
        return self._encode_patches(rows, N)


class ClipRGBEncoder(nn.Module):
    """CLIPEncoderB16 (resnet_encoders.py:280-314): ``.model.visual`` is the vision transformer (ViT-B/16 by default), the
    uint8 transform is part of the first kernel.  The reference builds it with clip.load("ViT-B/16"), which downloads the
    checkpoint; here the weights come from ``load_clip_state_dict``."""

    def __init__(self, input_resolution=224, patch_size=16, width=768, layers=12, heads=12, output_dim=512):
        super().__init__()
        self.model = _Holder()
        self.model.visual = ClipVisionTransformer(input_resolution, patch_size, width, layers, heads, output_dim)
        self.eval()

    def load_clip_state_dict(self, sd):
        """Load the vision tower from a full CLIP state dict: the ``visual.*`` keys are taken (strict=True on them), every
        other key -- the text tower's transformer.*, token_embedding, positional_embedding, ln_final, text_projection,
        logit_scale and the input_resolution / context_length / vocab_size entries of the published files -- is ignored."""
        vis = {k[len("visual."):]: v.float() for k, v in sd.items() if k.startswith("visual.")}
        if not vis:
            raise KeyError("load_clip_state_dict: no visual.* keys in the state dict")
        return self.model.visual.load_state_dict(vis, strict=True)

    def finalize(self, device, compute_dtype=torch.float32, max_images=NUM_VIEWS):
        self.model.visual.finalize(device, compute_dtype, max_images)
        return self

    def forward(self, observations):
        """observations["rgb"]: uint8 (N, H, W, 3) -> (rgb_vector (N, output_dim), rgb_grid (N, g * g, width)), both fp32."""
        rgb_vector, rgb_grid = self.model.visual.encode_u8(observations["rgb"].contiguous())
        return rgb_vector.float(), rgb_grid.float()


_VIEW_MAPS = {}


def clockwise_view_map(B, device):
    """int32 (B * 12): slot s of environment b reads view (12 - s) % 12 of it -- the simulator hands the views over
    counter-clockwise, the reference re-orders them clockwise (Policy_ViewSelection_BEV.py:176-185: view a -> slot
    (12 - a) % 12)."""
    key = (B, torch.device(device))
    t = _VIEW_MAPS.get(key)
    if t is None:
        s = torch.arange(NUM_VIEWS)
        m = torch.arange(B)[:, None] * NUM_VIEWS + ((NUM_VIEWS - s) % NUM_VIEWS)[None]
        t = _VIEW_MAPS[key] = m.reshape(-1).to(torch.int32).to(device)
    return t


def encode_panorama(encoder, rgb_u8, depth, embeds_dtype=None):
    """Mode 'waypoint' in front of the predictor: rgb_u8 (B, 12, R, R, 3) uint8 and depth (B, 12, Hd, Wd, 1) fp32 in the
    simulator's counter-clockwise view order -> (rgb_embeds (B * 12, output_dim), rgb_grid (B, 12, g * g, width) fp32,
    depth_grid (B, 12, 14, 14) fp32) in the reference's clockwise order: what waypoint_step and CEGraphMap.remember_pano
    take as they are.  ``encoder``: a finalized ClipRGBEncoder or ClipVisionTransformer with max_images >= B * 12.  The
    re-ordering is an index map read by the patch and pooling kernels, not a copy.  ``embeds_dtype``: the dtype of
    rgb_embeds; None = the compute dtype of an fp32 / bf16 encoder, and fp32 for an fp16 encoder (the predictor takes fp32
    and bf16 only; fp16 -> fp32 is exact, one elementwise launch over B * 12 x output_dim values, no synchronisation)."""
    vit = encoder.model.visual if isinstance(encoder, ClipRGBEncoder) else encoder
    if rgb_u8.dim() != 5 or rgb_u8.shape[1] != NUM_VIEWS or depth.dim() != 5 or tuple(depth.shape[:2]) != tuple(rgb_u8.shape[:2]):
        raise ValueError("encode_panorama: rgb (B, 12, R, R, 3) uint8 and depth (B, 12, Hd, Wd, 1) float32 expected")
    B = rgb_u8.shape[0]
    vmap = clockwise_view_map(B, rgb_u8.device)
    x, x_patch = vit.encode_u8(rgb_u8.reshape((B * NUM_VIEWS,) + tuple(rgb_u8.shape[2:])), vmap)
    dgrid = depth_grid_pool(depth.reshape((B * NUM_VIEWS,) + tuple(depth.shape[2:])), vmap)
    if embeds_dtype is None and x.dtype == torch.float16:
        embeds_dtype = torch.float32
    if embeds_dtype is not None and x.dtype != embeds_dtype:
        x = x.to(embeds_dtype)
    return x,x_patch.view(B, NUM_VIEWS, x_patch.shape[1], x_patch.shape[2]), dgrid.view(B, NUM_VIEWS, GRID, GRID)
