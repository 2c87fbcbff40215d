"""Regenerate tests/golden/clip_vit.npz and tests/golden/clip_vit_keys.txt from the reference's own code.

Build machine only: python tests/golden/make_clip_vit_golden.py <root of the reference checkout> (or BEVBERT_REFERENCE);
the reference is read from there, imported -- not copied:
  * bevbert_ce/vlnce_baselines/models/encoders/clip/model.py is loaded BY FILE PATH: the package __init__ wants ftfy and
    torchvision, model.py alone needs torch and numpy;
  * the two-line uint8 transform of CLIPEncoderB16 (torchvision's ConvertImageDtype + Normalize, not installed here) is
    restated in torch (tests/clip_ref.py transform);
  * weights by rule, nothing downloaded: tests/clip_ref.py fill() over the module's own key / shape list.
Per case of clip_ref.CASES: VisionTransformer(*cfg) in eval mode on the seeded uint8 images, fp32, CPU.  Stored: the
full x, a sample of x_patch (clip_ref.sample), and the reference's OWN reduced-precision distance from that fp32 run for
each stored tensor -- once with its convert_weights (fp16, the arithmetic of its GPU path) and once with the same
parameters cast to bfloat16 instead -- as rel-L2 and max-abs / absmax.  The bf16 gate of tests/test_gpu_clip_vit.py is a multiple
of the recorded bfloat16 figure.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BEVBERT_REFERENCE", "")     # root of the reference checkout
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def _load_model_py():
    path = os.path.join(REF, "bevbert_ce", "vlnce_baselines", "models", "encoders", "clip", "model.py")
    spec = importlib.util.spec_from_file_location("ref_clip_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _to_bfloat16(model):
    """The bfloat16 counterpart of the reference's fp16 conversion, stated by parameter name: every parameter goes to
    bfloat16 except the LayerNorm ones (ln_*) and the two embeddings, which stay fp32 (asserted in main() to be exactly the
    set the reference's own function leaves in fp32)."""
    for name, p in model.named_parameters():
        if not _stays_fp32(name):
            p.data = p.data.to(torch.bfloat16)


def _stays_fp32(name):
    return "ln_" in name or name in ("class_embedding", "positional_embedding")


def main():
    assert REF and os.path.isdir(REF), "give the root of the reference checkout (argument or BEVBERT_REFERENCE)"
    from tests import clip_ref as R
    M = _load_model_py()
    torch.manual_seed(0)
    out = {}
    for case, (cfg, n, seed) in R.CASES.items():
        net = M.VisionTransformer(*cfg)
        own = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert list(own.items()) == list(R.shapes(cfg).items()), "clip_ref.shapes() differs from the reference's state_dict"
        if cfg == R.KEYS_CONFIG:
            with open(os.path.join(HERE, "clip_vit_keys.txt"), "w") as f:
                for k, s in own.items():
                    f.write(f"{k} {s}\n")
        sd = R.state_dict(cfg)
        net.load_state_dict(sd, strict=True)
        net.eval()
        u8 = R.images(seed, n, cfg[0])
        x_in = R.transform(u8)
        row_max = R.attention_row_max(sd, cfg, x_in)
        assert row_max >= 0.2, (case, row_max)
        with torch.no_grad():
            x, xp = net(x_in)
        cols, toks = R.sample(xp)
        out[case + "_x"], out[case + "_xp_cols"], out[case + "_xp_toks"] = x.numpy(), cols.numpy(), toks.numpy()
        out[case + "_attn_row_max"] = np.array(row_max)
        report = [f"{case}: attention row-max {row_max:.3f}, |x| max {float(x.abs().max()):.2f}, |x_patch| max "
                  f"{float(xp.abs().max()):.2f}"]
        for tag, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            low = M.VisionTransformer(*cfg)
            low.load_state_dict(sd, strict=True)
            low.eval()
            if dt == torch.float16:
                M.convert_weights(low)                       # the reference's own function
                assert all((p.dtype == torch.float32) == _stays_fp32(k) for k, p in low.named_parameters())
            else:
                _to_bfloat16(low)
            with torch.no_grad():
                xl, xpl = low(x_in.to(dt))
            cl, tl = R.sample(xpl.float())
            for name, got, want in (("x", xl.float(), x), ("xp_cols", cl, cols), ("xp_toks", tl, toks)):
                out[f"{case}_{tag}_rel_l2_{name}"] = np.array(R.rel_l2(got.numpy(), want.numpy()))
                out[f"{case}_{tag}_max_rel_{name}"] = np.array(R.max_rel(got.numpy(), want.numpy()))
                report.append(f"  {tag} {name}: rel-L2 {R.rel_l2(got.numpy(), want.numpy()):.3e} max-abs/absmax "
                              f"{R.max_rel(got.numpy(), want.numpy()):.3e}")
        print("\n".join(report), flush=True)
    path = os.path.join(HERE, "clip_vit.npz")
    np.savez_compressed(path, **out)
    print("clip_vit.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
