"""ms per panorama batch (12 * batch depth views of 256 x 256) of the device-side depth ResNet encoder
(vln_bevbert_amd.depth_resnet), eager and replayed from one hipGraph, with bf16 and with fp32 operands, next to a plain-torch
channels-last bf16 run of the same network (the library convolution plus F.group_norm) on the same GPU in the same process,
the variants taking turns.  Device events, after warm-up, at least `--seconds` of device work per variant.  Also the
algorithmic FLOP, the bytes the stage's own launches read and write (from the shapes), and the launch count.

    python scripts/bench_depth_resnet.py [--batch 16] [--seconds 1.0] [--out profiles/depth_resnet_bench.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vln_bevbert_amd import depth_resnet as D  # noqa: E402
from vln_bevbert_amd import ops_gemm  # noqa: E402

SIZE = 256


def seeded_state_dict(model):
    """Convolutions N(0, 2 / fan_in), gamma = 1 + 0.1 N(0, 1), beta = 0.1 N(0, 1)."""
    gen = torch.Generator().manual_seed(0)
    sd = {}
    for k, v in model.state_dict().items():
        r = torch.randn(v.shape, generator=gen)
        sd[k] = r * (2.0 / v[0].numel()) ** 0.5 if v.dim() == 4 else (1 + 0.1 * r if k.endswith(".weight") else 0.1 * r)
    return sd


class Census:
    """Counts the launches of one eager call and adds up, from the shapes, the FLOP of its GEMMs and the bytes every launch
    reads and writes (a GEMM: both operands and the product; a kernel: its tensor arguments)."""

    def __init__(self):
        self.launches, self.flop, self.bytes, self.gemms = 0, 0, 0, 0

    def run(self, model, depth):
        call, linear = D.ops.call, D.ops.linear

        def counted_linear(x, weight, bias=None, w_c=None, b_c=None):
            y = linear(x, weight, bias, w_c=w_c, b_c=b_c)
            self.launches += 1
            self.gemms += 1
            self.flop += 2 * x.shape[0] * w_c.shape[0] * w_c.shape[1]
            self.bytes += (x.numel() + w_c.numel() + y.numel()) * x.element_size()
            return y

        def counted_call(name, *args):
            self.launches += 1
            return call(name, *args)
        wrappers = {}
        for fn in ("stem_conv", "group_norm_stats", "group_norm_apply", "group_norm_relu_maxpool", "gather_rows"):
            wrappers[fn] = getattr(D, fn)
            setattr(D, fn, self._sized(fn, wrappers[fn]))
        D.ops.call, D.ops.linear = counted_call, counted_linear
        try:
            model.encode(depth)
        finally:
            D.ops.call, D.ops.linear = call, linear
            for fn, f in wrappers.items():
                setattr(D, fn, f)
        return self

    def _sized(self, name, f):
        def g(*args, **kw):
            out = f(*args, **kw)
            tensors = [t for t in list(args) + list(kw.values()) if torch.is_tensor(t) and t.dim() >= 3]
            for extra in (kw.get("other"),):
                if extra is not None:
                    tensors.append(extra[0])
            if name == "group_norm_stats":
                x = args[0]
                self.launches += D.gn_chunks(x.shape[1], x.shape[2]) > 1        # the combine launch
                self.bytes += x.numel() * x.element_size()
            else:
                res = out if torch.is_tensor(out) else out[0]
                seen = {t.data_ptr(): t for t in tensors if t.data_ptr() != res.data_ptr()}
                self.bytes += sum(t.numel() * t.element_size() for t in seen.values()) + res.numel() * res.element_size()
            return out
        return g


def algorithmic_flop(model, n):
    """2 * output pixels * taps * input channels * output channels over every convolution."""
    side = SIZE // 4
    flop = side * side * 49 * 32
    side //= 2
    for blk in model._blocks():
        so = side // blk.stride
        flop += side * side * blk.cin * blk.planes + so * so * 9 * blk.planes ** 2 + so * so * blk.planes * 4 * blk.planes
        if blk.downsample is not None:
            flop += so * so * blk.cin * 4 * blk.planes
        side = so
    flop += side * side * 9 * model.final_channels * model.out_channels
    return 2 * flop * n


class TorchChannelsLast:
    """The same network in plain torch: bf16 weights and activations in channels-last layout, F.conv2d (the convolution
    library) and F.group_norm."""

    def __init__(self, model, dev):
        self.m = model
        self.p = {k: (v.to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last) if v.dim() == 4
                      else v.to(dev, torch.bfloat16)) for k, v in model.state_dict().items()}

    def _gn(self, x, key, groups):
        return F.group_norm(x, groups, self.p[key + ".weight"], self.p[key + ".bias"], 1e-5)

    @torch.no_grad()
    def __call__(self, depth):
        p, G, pre = self.p, self.m.groups, "visual_encoder.backbone."
        x = F.avg_pool2d(depth.permute(0, 3, 1, 2), 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x = F.relu(self._gn(F.conv2d(x, p[pre + "conv1.0.weight"], None, 2, 3), pre + "conv1.1", G))
        x = F.max_pool2d(x, 3, 2, 1)
        for i, blocks in enumerate(self.m.layers):
            for b in range(blocks):
                k = f"{pre}layer{i + 1}.{b}."
                stride = 2 if (b == 0 and i > 0) else 1
                h = F.relu(self._gn(F.conv2d(x, p[k + "convs.0.weight"]), k + "convs.1", G))
                h = F.relu(self._gn(F.conv2d(h, p[k + "convs.3.weight"], None, stride, 1), k + "convs.4", G))
                h = self._gn(F.conv2d(h, p[k + "convs.6.weight"]), k + "convs.7", G)
                if b == 0:
                    x = self._gn(F.conv2d(x, p[k + "downsample.0.weight"], None, stride), k + "downsample.1", G)
                x = F.relu(h + x)
        x = F.conv2d(x, p["visual_encoder.compression.0.weight"], None, 1, 1)
        return F.relu(self._gn(x, "visual_encoder.compression.1", 1)).contiguous()


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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.batch * 12
    ref = D.DepthResNetEncoder(SIZE)
    sd = seeded_state_dict(ref)
    ref.load_state_dict(sd, strict=True)
    depth = torch.rand(n, SIZE, SIZE, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    variants, keep, census = {}, [], {}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        m = D.DepthResNetEncoder(SIZE)
        m.load_state_dict(sd, strict=True)
        m.finalize(dev, dt, n)
        for _ in range(2):
            m.encode(depth)
        torch.cuda.synchronize()
        census[tag] = Census().run(m, depth)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            m.encode(depth)
        keep.append((m, graph))
        variants[f"hip {tag} eager"] = (lambda m=m: m.encode(depth))
        variants[f"hip {tag} hipGraph replay"] = graph.replay
    torch_note = None
    try:
        t = TorchChannelsLast(ref, dev)
        t(depth)
        torch.cuda.synchronize()
        variants["torch bf16 channels-last"] = (lambda: t(depth))
    except Exception as e:                                        # the convolution library found no kernel
        torch_note = f"  plain-torch bf16 channels-last run not available on this machine: {type(e).__name__}: {str(e)[:200]}"
    ms, calls = take_turns(variants, a.seconds)
    flop = algorithmic_flop(ref, n)
    lines = [f"depth ResNet-50 (GroupNorm, 32 base planes) encoder, batch {a.batch} = {n} depth views of {SIZE} x {SIZE}, "
             f"{torch.cuda.get_device_name(0)}",
             f"  algorithmic work: {flop / 1e9:.1f} GFLOP per batch ({flop / n / 1e9:.3f} GFLOP per image)"]
    for tag, c in census.items():
        lines.append(f"  hip {tag}: {c.launches} launches per batch ({c.gemms} GEMMs, {c.flop / 1e9:.1f} GFLOP in them), "
                     f"{c.bytes / 1e9:.2f} GB read + written by the launches")
    for k, v in ms.items():
        lines.append(f"  {k:28s} {v:9.3f} ms / batch   {flop / v / 1e9:7.1f} TF/s   ({calls[k]} calls timed)")
    if torch_note:
        lines.append(torch_note)
    else:
        base = ms["torch bf16 channels-last"]
        for k in ("hip bf16 hipGraph replay", "hip fp32 hipGraph replay"):
            lines.append(f"  torch bf16 channels-last / {k}: {base / ms[k]:.2f}")
    lines.append(f"  GEMMs that went through torch instead of the direct hipBLASLt path: {dict(ops_gemm.GEMM_FALLBACKS) or 'none'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
