"""Plain-torch CPU restatement of the CLIP vision tower (encoders/clip/model.py VisionTransformer) and of the uint8
transform in front of it (resnet_encoders.py:299-312), written from the math; it runs in fp32 or fp64.  Pinned to the
reference's recorded outputs by tests/test_clip_vit_host.py; the GPU tests use it for shapes the golden does not hold.
Also the one place for the weight rule and the seeded inputs that tests/golden/make_clip_vit_golden.py and the tests share.
"""
import numpy as np
import torch

from vln_bevbert_amd import weights

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
QK_SCALE = 4.0      # the q and k rows of in_proj_weight / in_proj_bias are multiplied by this: attention is not uniform

# case -> ((input_resolution, patch_size, width, layers, heads, output_dim), images, image seed)
CASES = {"b16_l2": ((224, 16, 768, 2, 12, 512), 3, 101),
         "b16_l12": ((224, 16, 768, 12, 12, 512), 12, 102),
         "b32_l2": ((224, 32, 768, 2, 12, 512), 2, 103)}
KEYS_CONFIG = CASES["b16_l12"][0]          # the configuration tests/golden/clip_vit_keys.txt lists (ViT-B/16)
COL_STRIDE = 48                            # x_patch sample: every token at columns 0, 48, ...
def sample_tokens(n_patch):                # ... and every column at these tokens (first and last patch token included)
    return sorted({0, 1, n_patch // 2, n_patch - 2, n_patch - 1})


def shapes(cfg):
    """state_dict keys and shapes of VisionTransformer(*cfg), in the module's own order."""
    R, P, W, layers, heads, out = cfg
    s = {"class_embedding": (W,), "positional_embedding": ((R // P) ** 2 + 1, W), "proj": (W, out),
         "conv1.weight": (W, 3, P, P), "ln_pre.weight": (W,), "ln_pre.bias": (W,)}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        s.update({p + "attn.in_proj_weight": (3 * W, W), p + "attn.in_proj_bias": (3 * W,),
                  p + "attn.out_proj.weight": (W, W), p + "attn.out_proj.bias": (W,),
                  p + "ln_1.weight": (W,), p + "ln_1.bias": (W,),
                  p + "mlp.c_fc.weight": (4 * W, W), p + "mlp.c_fc.bias": (4 * W,),
                  p + "mlp.c_proj.weight": (W, 4 * W), p + "mlp.c_proj.bias": (W,),
                  p + "ln_2.weight": (W,), p + "ln_2.bias": (W,)})
    s.update({"ln_post.weight": (W,), "ln_post.bias": (W,)})
    return s


def fill(key, shape):
    """weights.fill_tensor("visual." + key) with two overrides: ln_*.weight -> 1 + 5 * fill = 1 + 0.1 N(0, 1) (the rule's
    LayerNorm pattern does not match CLIP's names), and the q and k rows of in_proj_* times QK_SCALE."""
    t = weights.fill_tensor("visual." + key, shape)
    name = key.rsplit(".", 2)
    if key.endswith(".weight") and name[-2].startswith("ln_"):
        return 1.0 + 5.0 * t
    if "in_proj_" in key:
        t = t.clone()
        t[:2 * shape[0] // 3] *= QK_SCALE
    return t


def state_dict(cfg):
    return {k: fill(k, s) for k, s in shapes(cfg).items()}


def images(seed, n, res=224):
    """Seeded uint8 (n, res, res, 3): smooth low-frequency content plus noise, so that patches differ from each other."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (n, res // 16, res // 16, 3)).astype(np.float32)
    up = np.repeat(np.repeat(coarse, 16, 1), 16, 2)
    noise = rng.integers(-48, 49, (n, res, res, 3)).astype(np.float32)
    return torch.from_numpy(np.clip(up + noise, 0, 255).astype(np.uint8))


def transform(u8):
    """ConvertImageDtype(torch.float) + Normalize(MEAN, STD) on (N, H, W, 3) uint8 -> (N, 3, H, W) fp32, restated in
    torch (torchvision's two lines: image.to(float32) / 255, then tensor.sub_(mean).div_(std) with fp32 mean / std)."""
    x = u8.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    return x.sub(mean).div(std)


def unfold(x, P):
    """(N, 3, R, R) -> patch rows (N * g * g, 3 * P * P), column order (c, ky, kx): conv1 as a GEMM operand."""
    N, C, R, _ = x.shape
    g = R // P
    return x.reshape(N, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N * g * g, C * P * P)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def quickgelu(t):
    return t * torch.sigmoid(1.702 * t)


def forward(sd, cfg, x, dtype=torch.float32):
    """VisionTransformer.forward on normalised (N, 3, R, R) images: (x (N, output_dim), x_patch (N, g * g, width))."""
    R, P, W, layers, heads, _ = cfg
    sd = {k: v.to(dtype) for k, v in sd.items()}
    N = x.shape[0]
    L = (R // P) ** 2 + 1
    h = unfold(x.to(dtype), P) @ sd["conv1.weight"].reshape(W, -1).t()
    h = torch.cat([sd["class_embedding"].expand(N, 1, W), h.view(N, L - 1, W)], 1) + sd["positional_embedding"]
    h = _ln(h, sd["ln_pre.weight"], sd["ln_pre.bias"])
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        y = _ln(h, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        qkv = y @ sd[p + "attn.in_proj_weight"].t() + sd[p + "attn.in_proj_bias"]
        q, k, v = (t.view(N, L, heads, W // heads).transpose(1, 2) for t in qkv.split(W, -1))
        a = torch.softmax(q @ k.transpose(-1, -2) / (W // heads) ** 0.5, -1) @ v
        a = a.transpose(1, 2).reshape(N, L, W)
        h = h + (a @ sd[p + "attn.out_proj.weight"].t() + sd[p + "attn.out_proj.bias"])
        y = _ln(h, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
        t = quickgelu(y @ sd[p + "mlp.c_fc.weight"].t() + sd[p + "mlp.c_fc.bias"])
        h = h + (t @ sd[p + "mlp.c_proj.weight"].t() + sd[p + "mlp.c_proj.bias"])
    return _ln(h[:, 0], sd["ln_post.weight"], sd["ln_post.bias"]) @ sd["proj"], h[:, 1:]


def attention_row_max(sd, cfg, x):
    """Mean over (image, head, query) of the largest attention probability in block 0 (the generator's guard against a
    uniform attention, under which a wrong key padding could hide)."""
    R, P, W, layers, heads, _ = cfg
    N, L = x.shape[0], (R // P) ** 2 + 1
    h = unfold(x, P) @ sd["conv1.weight"].reshape(W, -1).t()
    h = torch.cat([sd["class_embedding"].expand(N, 1, W), h.view(N, L - 1, W)], 1) + sd["positional_embedding"]
    h = _ln(h, sd["ln_pre.weight"], sd["ln_pre.bias"])
    p = "transformer.resblocks.0."
    qkv = _ln(h, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"]) @ sd[p + "attn.in_proj_weight"].t() + sd[p + "attn.in_proj_bias"]
    q, k, _ = (t.view(N, L, heads, W // heads).transpose(1, 2) for t in qkv.split(W, -1))
    return float(torch.softmax(q @ k.transpose(-1, -2) / (W // heads) ** 0.5, -1).amax(-1).mean())


def sample(x_patch):
    """The stored sample of x_patch (N, n_patch, W): (every token at the strided columns, every column at sample_tokens)."""
    return x_patch[:, :, ::COL_STRIDE], x_patch[:, sample_tokens(x_patch.shape[1])]


def clockwise(t, B):
    """The reference's re-ordering (Policy_ViewSelection_BEV.py:176-185) of (B * 12, ...) rows: view a -> slot (12 - a) % 12."""
    v = t.reshape((B, 12) + tuple(t.shape[1:]))
    out = torch.empty_like(v)
    for a in range(12):
        out[:, (12 - a) % 12] = v[:, a]
    return out.reshape(t.shape)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-300)))


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
