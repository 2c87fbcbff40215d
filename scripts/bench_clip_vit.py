"""ms per panorama batch (12 * batch images) of the device-side CLIP ViT-B/16 encoder (vln_bevbert_amd.clip_vit), eager and
replayed from one hipGraph, with fp32, bf16 and fp16 operands, next to a plain-torch fp16 restatement of the same network
(F.scaled_dot_product_attention, fp16 stream, fp32 LayerNorm statistics: the arithmetic of the reference's GPU path) on the
same GPU in the same process, the variants taking turns.  Device events, after warm-up, at least a second of device work per
variant.  Also the algorithmic FLOP, the resulting TF/s, bytes / time / TB/s of the row kernels at the batch's rows, and the
attention call alone at the step's shape (batch * 12 images, 12 heads, 197 tokens): the fp16 kernel (csrc/attn_fwd2.hip) against
the kernel the dispatch plan gives bf16, in turns.

    python scripts/bench_clip_vit.py [--batch 16] [--seconds 1.0] [--out profiles/clip_vit_bench.txt [--append]]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vln_bevbert_amd import clip_vit as V  # noqa: E402
from vln_bevbert_amd import lib, ops, weights  # noqa: E402

CFG = (224, 16, 768, 12, 12, 512)
MODES = (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16))


def algorithmic_flop(cfg, n):
    R, P, W, layers, _, out = cfg
    g2 = (R // P) ** 2
    L = g2 + 1
    per_layer = 2 * L * W * 3 * W + 2 * 2 * L * L * W + 2 * L * W * W + 2 * 2 * L * W * 4 * W
    return n * (2 * g2 * 3 * P * P * W + layers * per_layer + 2 * W * out)


class TorchFp16:
    """The same network in plain torch: fp16 weights (the reference's convert_weights rule: LayerNorm parameters and the
    two embeddings stay fp32), fp16 residual stream, LayerNorm computed in fp32.  conv1 is applied as unfold + matmul."""

    def __init__(self, sd, cfg, dev):
        self.cfg = cfg
        keep32 = lambda k: "ln_" in k or k in ("class_embedding", "positional_embedding")   # noqa: E731
        self.p = {k: v.to(dev, torch.float32 if keep32(k) else torch.float16) for k, v in sd.items()}
        self.mean = torch.tensor(V.CLIP_MEAN, device=dev).view(1, 3, 1, 1)
        self.std = torch.tensor(V.CLIP_STD, device=dev).view(1, 3, 1, 1)

    def _ln(self, x, name):
        return F.layer_norm(x.float(), (x.shape[-1],), self.p[name + ".weight"], self.p[name + ".bias"], 1e-5).to(x.dtype)

    @torch.no_grad()
    def __call__(self, u8):
        R, P, W, layers, heads, _ = self.cfg
        p = self.p
        N, g = u8.shape[0], R // P
        x = ((u8.permute(0, 3, 1, 2).float() / 255 - self.mean) / self.std).half()
        x = x.reshape(N, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N, g * g, 3 * P * P)
        x = x @ p["conv1.weight"].view(W, -1).t()
        x = torch.cat([p["class_embedding"].half().expand(N, 1, W), x], 1) + p["positional_embedding"].half()
        x = self._ln(x, "ln_pre")
        L = x.shape[1]
        for i in range(layers):
            b = f"transformer.resblocks.{i}."
            qkv = F.linear(self._ln(x, b + "ln_1"), p[b + "attn.in_proj_weight"], p[b + "attn.in_proj_bias"])
            q, k, v = (t.view(N, L, heads, 64).transpose(1, 2) for t in qkv.split(W, -1))
            a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(N, L, W)
            x = x + F.linear(a, p[b + "attn.out_proj.weight"], p[b + "attn.out_proj.bias"])
            h = F.linear(self._ln(x, b + "ln_2"), p[b + "mlp.c_fc.weight"], p[b + "mlp.c_fc.bias"])
            x = x + F.linear(h * torch.sigmoid(1.702 * h), p[b + "mlp.c_proj.weight"], p[b + "mlp.c_proj.bias"])
        return self._ln(x[:, 0], "ln_post") @ p["proj"], x[:, 1:].float()


def _ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def take_turns(variants, seconds):
    """{name: ms per call}: the variants run in turns, rounds of a few calls each, until each has `seconds` of device time."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    total, calls = {k: 0.0 for k in variants}, {k: 0 for k in variants}
    while min(total.values()) < seconds * 1e3:
        for k, fn in variants.items():
            if total[k] < seconds * 1e3:
                total[k] += _ms(fn, 3)
                calls[k] += 3
    return {k: total[k] / calls[k] for k in variants}, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.batch * 12
    R, P, W, layers, heads, _ = CFG
    g = torch.Generator().manual_seed(0)
    ref = V.ClipVisionTransformer(*CFG)
    sd = weights.fill_state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()})
    sd.update({k: 1 + 5 * v for k, v in sd.items() if "ln_" in k and k.endswith(".weight")})     # gains around 1
    u8 = torch.randint(0, 256, (n, R, R, 3), generator=g, dtype=torch.uint8).to(dev)
    variants, graphs = {}, []
    for tag, dt in MODES:
        m = V.ClipVisionTransformer(*CFG)
        m.load_state_dict(sd, strict=True)
        m.finalize(dev, dt, n)
        for _ in range(2):
            m.encode_u8(u8)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            m.encode_u8(u8)
        graphs.append((m, graph))
        variants[f"hip {tag} eager"] = (lambda m=m: m.encode_u8(u8))
        variants[f"hip {tag} hipGraph replay"] = graph.replay
    variants["torch fp16 restatement"] = (lambda t=TorchFp16(sd, CFG, dev): t(u8))
    ms, calls = take_turns(variants, a.seconds)
    flop = algorithmic_flop(CFG, n)
    lines = [f"CLIP ViT-B/16 image encoder, batch {a.batch} = {n} images of {R} x {R}, {n * ((R // P) ** 2 + 1)} token rows, "
             f"{torch.cuda.get_device_name(0)}",
             f"  algorithmic work: {flop / 1e12:.3f} TFLOP per batch ({flop / n / 1e9:.2f} GFLOP per image)"]
    for k, v in ms.items():
        lines.append(f"  {k:28s} {v:9.3f} ms / batch   {flop / v / 1e9:7.1f} TF/s   ({calls[k]} calls timed)")
    base = ms["torch fp16 restatement"]
    for k in ("hip bf16 hipGraph replay", "hip fp16 hipGraph replay", "hip fp32 hipGraph replay"):
        lines.append(f"  torch fp16 restatement / {k}: {base / ms[k]:.2f}")
    lines.append(f"  hip fp16 hipGraph replay / hip bf16 hipGraph replay: "
                 f"{ms['hip fp16 hipGraph replay'] / ms['hip bf16 hipGraph replay']:.3f}")

    # the attention call alone at the step's shape, the two 16-bit kernels in turns
    L = (R // P) ** 2 + 1
    qkv = torch.randn(n, L, 3 * W, generator=g).to(dev)
    attn, paths = {}, {}
    with torch.no_grad():
        for tag, dt in MODES[1:]:
            t = qkv.to(dt)
            ops.attention_self(t, None, None, heads)
            paths[tag] = lib.load().bevbert_attn_last_path(0).decode() if dt == torch.bfloat16 else "attn_fwd2_f16"
            attn[f"attention {tag} ({paths[tag]})"] = (lambda t=t: ops.attention_self(t, None, None, heads))
        ams, acalls = take_turns(attn, a.seconds / 4)
    aflop = 2 * 2 * n * heads * L * L * 64
    lines.append(f"  attention alone, {n} images x {heads} heads x {L} tokens (packed qkv, event-timed, in turns):")
    for k, v in ams.items():
        lines.append(f"    {k:34s} {v * 1e3:8.1f} us / call   {aflop / v / 1e9:7.1f} TF/s   ({acalls[k]} calls timed)")
    fp16_name, bf16_name = [k for k in ams if " fp16 " in k][0], [k for k in ams if " bf16 " in k][0]
    lines.append(f"    fp16 kernel / bf16 kernel: {ams[fp16_name] / ams[bf16_name]:.3f}; {layers} calls per batch")

    # the row kernels on their own, at the batch's rows
    rows, prow, C4 = n * ((R // P) ** 2 + 1), n * (R // P) ** 2, 4 * W
    lines.append(f"  row kernels at {rows} token rows ({prow} patch rows), bytes moved / time / rate:")
    gen = torch.Generator().manual_seed(1)
    vec = lambda k: torch.randn(k, generator=gen).to(dev)      # noqa: E731
    for tag, dt in MODES:
        e = 4 if dt == torch.float32 else 2
        patches = torch.empty(prow, 3 * P * P, dtype=dt, device=dev)
        conv = torch.randn(prow, W, device=dev).to(dt)
        x = torch.randn(rows, W, device=dev).to(dt)
        z32, y = torch.randn(rows, W, device=dev), torch.empty(rows, W, dtype=dt, device=dev)
        h = torch.randn(rows, C4, device=dev).to(dt)
        act = torch.empty_like(h)
        pos, cls, bias, bias4 = torch.randn(rows // n, W, device=dev), vec(W), vec(W), vec(C4)
        ln = (vec(W), vec(W))
        kernels = {
            "vit_patchify": (lambda: V.patchify(u8, P, dt, out=patches), n * R * R * 3 + prow * 3 * P * P * e),
            "vit_embed_prenorm": (lambda: V.embed_prenorm(conv, cls, pos, ln, ln, rows // n, z32, y),
                                  prow * W * e + rows * W * (4 + e)),
            "vit_bias_residual_prenorm": (lambda: V.bias_residual_prenorm(z32, x, bias, ln[0], ln[1], y), rows * W * (8 + 2 * e)),
            "vit_bias_quickgelu": (lambda: V.bias_quickgelu(h, bias4, act), rows * C4 * 2 * e)}
        for name, (fn, nbytes) in kernels.items():
            for _ in range(3):
                fn()
            t = _ms(fn, 20) / 20
            lines.append(f"    {name + ' ' + tag:34s} {nbytes / 1e6:8.1f} MB  {t * 1e3:8.1f} us  {nbytes / t / 1e9:6.2f} TB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(("\n" if a.append else "") + text + "\n")


if __name__ == "__main__":
    main()
