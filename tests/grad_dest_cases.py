"""Shared by tests/test_grad_dest_host.py (CPU, stubbed C ABI) and tests/test_gpu_grad_dest.py: one module that holds the
parameters of every op that produces a parameter gradient, the smallest inputs that still reach every branch, and one
runner per op.  Nothing here touches the library.

Shapes: 33 rows (three 10-row blocks of the column kernels and a short fourth), H = 256 (the narrowest width the row kernels
are instantiated for), C = 40 activations (the 4-wide path) and a 3-wide bias (bevbert_colsum_any), K = 7 for the small-K
projection, 5-row tables, a 5-node graph bias over 2 samples, 2 layers and 2 heads.  The activation, embedding, small-K and
graph inputs are the generators of tests/body_cases.py and tests/smallk_cases.py at these shapes, so their gates apply as
stated there (which fixes the small-K table at smallk_cases.TABLE_ROWS = 4 rows and the BertEmbeddings tables at 11 / 14 /
2 rows)."""
import torch
from torch import nn

from tests import body_cases as bc
from tests import smallk_cases as sk

ROWS, H, C, K, TROWS, KIN = 33, 256, 40, 7, 5, 16
B, LAYERS, G, NH = 2, 2, 5, 2
EMB = (11, H, 3, 11)                 # V, H, B, L of body_cases.embed_case: 33 rows
EPS = 1e-12
ROW = 1                              # the table row RowOfTable names


class Params(nn.Module):
    def __init__(self, dtype):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.ln, self.ln_in, self.typ5 = nn.LayerNorm(H), nn.Parameter(torch.zeros(H)), nn.Embedding(TROWS, H)
        self.gelu_b, self.relu_b = nn.Parameter(torch.zeros(C)), nn.Parameter(torch.zeros(C))
        self.lin, self.lin3 = nn.Linear(KIN, H), nn.Linear(KIN, 3)
        self.query, self.key, self.value = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)
        self.kv = nn.ModuleList(nn.ModuleDict({"key": nn.Linear(H, H), "value": nn.Linear(H, H)}) for _ in range(LAYERS))
        e = bc.embed_case(*EMB)
        self.word, self.pos, self.typ = (nn.Embedding(*e[k].shape) for k in ("word", "pos", "typ"))
        self.eln = nn.LayerNorm(H)
        self.loc, self.loc_ln, self.nav = nn.Linear(K, H), nn.LayerNorm(H), nn.Embedding(sk.TABLE_ROWS, H)
        self.sprel = nn.Linear(1, 1)
        self.scalar = nn.Parameter(torch.zeros(1))
        s = sk.case(ROWS, K, H, dtype)
        fixed = {"word.weight": e["word"], "pos.weight": e["pos"], "typ.weight": e["typ"], "eln.weight": e["gamma"],
                 "eln.bias": e["beta"], "loc.weight": s["W"], "loc.bias": s["b"], "loc_ln.weight": s["gamma"],
                 "loc_ln.bias": s["beta"], "nav.weight": s["table"], "gelu_b": bc.gelu_case(ROWS, C, dtype)[1],
                 "relu_b": bc.gelu_case(ROWS, C, dtype, seed=1)[1]}
        with torch.no_grad():
            for n, p in self.named_parameters():
                if n in fixed:
                    p.copy_(fixed[n])
                else:
                    p.copy_((1.0 if n in ("ln.weight",) else 0.0) + (0.05 if p.dim() == 2 and p.shape[1] > 1 else 0.3)
                            * torch.randn(p.shape, generator=g))


QKV_W, QKV_B = [f"{k}.weight" for k in ("query", "key", "value")], [f"{k}.bias" for k in ("query", "key", "value")]
KV_W = [f"kv.{i}.{k}.weight" for i in range(LAYERS) for k in ("key", "value")]
KV_B = [f"kv.{i}.{k}.bias" for i in range(LAYERS) for k in ("key", "value")]
GROUPS = [QKV_W, QKV_B, KV_W, KV_B]


def inputs(dtype, device):
    """Every runner's inputs, values of ``dtype`` (the small-K features, the distances and the graph gradients fp32)."""
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)
    e, s = bc.embed_case(*EMB), sk.case(ROWS, K, H, dtype)
    dbias, dists = bc.graph_case(LAYERS, B, NH, G)
    xg, _, dg = bc.gelu_case(ROWS, C, dtype)
    xr, _, dr = bc.gelu_case(ROWS, C, dtype, seed=1)
    i = {"x": rn(ROWS, H), "res": rn(ROWS, H), "dy": rn(ROWS, H), "dz": rn(ROWS, H), "xg": xg, "dg": dg, "xr": xr, "dr": dr,
         "xl": rn(ROWS, KIN), "dl": rn(ROWS, H), "dl3": rn(ROWS, 3), "dqkv": rn(ROWS, 3 * H), "ctx": rn(3, 11, H),
         "dkv": [rn(3, 11, 2 * H) for _ in range(LAYERS)], "ids": e["ids"], "type_index": e["type_index"],
         "de": e["dy"].to(dtype), "feat": s["feat"], "post1": s["post1"], "nav_idx": s["idx"], "dsk": s["dy"],
         "dists": dists, "dbias": dbias, "vec": rn(8).float(), "dvec": rn(8).float(),
         "look": torch.randint(0, TROWS - 1, (ROWS,), generator=g)}           # (the last table row is never looked up)
    return {k: ([t.to(device) for t in v] if isinstance(v, list) else v.to(device) if torch.is_tensor(v) else v)
            for k, v in i.items()}


def _leaf(t):
    return t.clone().requires_grad_(True)


def _packed(ops, m, wn, bn, shape):
    by = dict(m.named_parameters())
    wc, wg = m.arena.packed(wn, shape)
    bc_, bg = m.arena.packed(bn, shape[:1])
    return ops._PackedParam([by[n] for n in wn], wc, wg), ops._PackedParam([by[n] for n in bn], bc_, bg)


def _graph(ops, m, i):
    outs = ops.graph_bias(i["dists"], m.sprel.weight, m.sprel.bias, LAYERS, NH)
    if not i["dists"].is_cuda:                   # no attention to fill the holder: the gradients arrive at the views
        return outs, [i["dbias"][l].sum(1) for l in range(LAYERS)]
    holder = outs[0]._dbias_slot[0]              # as the attention backward leaves them: in the holder, a dummy to autograd
    for l in range(LAYERS):
        holder.slot(l, B, G, i["dists"].device).copy_(i["dbias"][l])
    return outs, [holder.dummy] * LAYERS


def _lookup(ops, m, i):
    from vln_bevbert_amd.vilmodel import embedding_lookup
    return [embedding_lookup(m.typ5, i["look"])], [i["dy"]]


# op -> ({label: [parameter names]}, needs an arena, runner(ops, m, inputs) -> (outputs, their gradients))
OPS = {
    "layernorm": ({"gamma": ["ln.weight"], "beta": ["ln.bias"]}, False,
                  lambda ops, m, i: ([ops.layernorm(_leaf(i["x"]), m.ln.weight, m.ln.bias, EPS)], [i["dy"]])),
    "bdrl": ({"gamma": ["ln.weight"], "beta": ["ln.bias"], "bias": ["ln_in"]}, False,
             lambda ops, m, i: ([ops.bias_dropout_residual_layernorm(_leaf(i["x"]), m.ln_in, i["res"], m.ln.weight, m.ln.bias,
                                                                     EPS)], [i["dy"]])),
    "bdrl_row": ({"gamma": ["ln.weight"], "beta": ["ln.bias"], "bias": ["typ5.weight"]}, True,
                 lambda ops, m, i: ([ops.bias_dropout_residual_layernorm(_leaf(i["x"]), ops.RowOfTable(m.typ5.weight, ROW),
                                                                         i["res"], m.ln.weight, m.ln.bias, EPS)], [i["dy"]])),
    "prenorm": ({"gamma": ["ln.weight"], "beta": ["ln.bias"], "bias": ["ln_in"]}, False,
                lambda ops, m, i: (list(ops.bias_dropout_residual_prenorm(_leaf(i["x"]), m.ln_in, i["res"], m.ln.weight,
                                                                          m.ln.bias, EPS)), [i["dy"], i["dz"]])),
    "gelu": ({"bias": ["gelu_b"]}, False, lambda ops, m, i: ([ops.bias_gelu(_leaf(i["xg"]), m.gelu_b)], [i["dg"]])),
    "relu": ({"bias": ["relu_b"]}, False, lambda ops, m, i: ([ops.bias_relu(_leaf(i["xr"]), m.relu_b)], [i["dr"]])),
    "linear": ({"weight": ["lin.weight"], "bias": ["lin.bias"]}, False,
               lambda ops, m, i: ([ops.linear(_leaf(i["xl"]), m.lin.weight, m.lin.bias)], [i["dl"]])),
    "linear3": ({"weight": ["lin3.weight"], "bias": ["lin3.bias"]}, False,
                lambda ops, m, i: ([ops.linear(_leaf(i["xl"]), m.lin3.weight, m.lin3.bias)], [i["dl3"]])),
    "linear_packed": ({"weight": QKV_W, "bias": QKV_B}, True,
                      lambda ops, m, i: ([ops.linear_packed(_leaf(i["x"]), *_packed(ops, m, QKV_W, QKV_B, (3 * H, H)))],
                                         [i["dqkv"]])),
    "hoisted_kv": ({"weight": KV_W, "bias": KV_B}, True,
                   lambda ops, m, i: (list(ops.hoisted_kv(_leaf(i["ctx"]), *_packed(ops, m, KV_W, KV_B, (LAYERS * 2 * H, H)),
                                                          LAYERS)), i["dkv"])),
    "embed_ln": ({"word": ["word.weight"], "pos": ["pos.weight"], "typ": ["typ.weight"], "gamma": ["eln.weight"],
                  "beta": ["eln.bias"]}, False,
                 lambda ops, m, i: ([ops.embed_sum_layernorm(i["ids"], m.word.weight, m.pos.weight, m.typ.weight, m.eln.weight,
                                                             m.eln.bias, EPS, i["type_index"])], [i["de"]])),
    "smallk": ({"W": ["loc.weight"], "b": ["loc.bias"], "gamma": ["loc_ln.weight"], "beta": ["loc_ln.bias"],
                "table": ["nav.weight"]}, True,
               lambda ops, m, i: ([ops.smallk_linear_layernorm_plus(i["feat"], m.loc, m.loc_ln, EPS, _leaf(i["post1"]), m.nav,
                                                                    i["nav_idx"])], [i["dsk"]])),
    "graph_bias": ({"weight": ["sprel.weight"], "bias": ["sprel.bias"]}, True, _graph),
    "use_param": ({"p": ["scalar"]}, False, lambda ops, m, i: ([ops.use_param(m.scalar) * i["vec"]], [i["dvec"]])),
    "lookup": ({"table": ["typ5.weight"]}, False, _lookup),
}


def freeze(m, names):
    for n, p in m.named_parameters():
        p.requires_grad_(n not in names)
