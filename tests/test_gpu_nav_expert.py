"""csrc/nav_expert.hip against the reference: expert targets and _eval_item metrics from golden nav_expert.npz (made by
tests/golden/make_nav_expert_golden.py with the reference's own _teacher_action_r4r / _eval_item), the action step
against torch and a host restatement of agent.py:523-612, the IL loss against F.cross_entropy(ignore_index=-100)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vln_bevbert_amd import nav_expert as NE
from vln_bevbert_amd.nav_expert import ScanGraphs

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "nav_expert.npz"))


@pytest.fixture(scope="module")
def graphs(gold, tmp_path_factory):
    raw = np.load(os.path.join(GOLDEN, "nav_scans.npz"))
    d = tmp_path_factory.mktemp("connectivity")
    paths = {}
    for s in gold["scans"]:
        s = str(s)
        ids, inc, un, pose = (raw[f"{s}/{k}"] for k in ("ids", "included", "unobstructed", "pose"))
        paths[s] = str(d / f"{s}_connectivity.json")
        with open(paths[s], "w") as f:
            json.dump([{"image_id": str(i), "included": bool(a), "unobstructed": [bool(x) for x in u],
                        "pose": [float(p) for p in po]} for i, a, u, po in zip(ids, inc, un, pose)], f)
    return ScanGraphs.from_connectivity(paths)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------- expert
@pytest.mark.parametrize("case", range(6))
def test_expert_targets_equal_the_reference(gold, graphs, case):
    p = f"exp{case}_"
    policy = str(gold[p + "policy"])
    traj = gold[p + "traj"]
    got = NE.expert_targets(graphs, _t(gold[p + "scan"]), _t(gold[p + "cur"]), _t(gold[p + "cand"]),
                            _t(gold[p + "visited"]), _t(gold[p + "ended"]), _t(gold[p + "gt"]), _t(gold[p + "gt_len"]),
                            int(gold[p + "t"]), policy, _t(traj), _t(gold[p + "traj_len"]))
    want = gold[p + "target"]
    assert (want == NE.IGNOREID).any()
    assert got.cpu().numpy().tolist() == want.tolist(), policy


def test_dtw_over_several_lane_blocks_is_bit_equal_to_the_reference(gold, graphs):
    # reference paths of 65..100 nodes: the DP crosses one or two 64-lane block edges
    assert gold["long_gt_len"].min() > 64
    B = gold["long_gt_len"].shape[0]
    items, _ = NE.nav_metrics(graphs, np.full(B, 2, dtype=np.int64), _t(gold["long_path"]).long(),
                              gold["long_path_len"], np.zeros(B, dtype=np.int64), _t(gold["long_gt"]), gold["long_gt_len"])
    it = items.cpu().numpy()
    want = gold["long_DTW_nDTW_CLS"]
    assert np.array_equal(it[:, 8], want[:, 0])
    np.testing.assert_allclose(it[:, [9, 11]], want[:, 1:], rtol=1e-12, atol=0)


def test_int64_and_strided_inputs_are_converted(gold, graphs):
    p = "exp2_"
    c64 = _t(gold[p + "cand"]).long()
    cand = torch.zeros(c64.shape[0], 2 * c64.shape[1], dtype=torch.int64, device=DEV)[:, ::2]
    cand.copy_(c64)
    assert not cand.is_contiguous()
    got = NE.expert_targets(graphs, _t(gold[p + "scan"]).long(), _t(gold[p + "cur"]).long(), cand,
                            _t(gold[p + "visited"]), _t(gold[p + "ended"]), _t(gold[p + "gt"]).long(),
                            _t(gold[p + "gt_len"]).long(), 0, "ndtw", _t(gold[p + "traj"]).long(),
                            _t(gold[p + "traj_len"]).long())
    assert got.cpu().numpy().tolist() == gold[p + "target"].tolist()
    with pytest.raises(NE.lib.BevBertHipError):
        NE.expert_targets(graphs, _t(gold[p + "scan"]), _t(gold[p + "cur"]), _t(gold[p + "cand"]), None,
                          _t(gold[p + "ended"]), _t(gold[p + "gt"]), _t(gold[p + "gt_len"])[:-1], 0, "spl")


def test_metrics_of_an_unknown_scan_are_nan(gold, graphs):
    items, _ = NE.nav_metrics(graphs, torch.tensor([7, int(gold["met_scan"][1])], device=DEV), _t(gold["met_path"][:2]),
                              _t(gold["met_path_len"][:2]), _t(gold["met_action_steps"][:2]), _t(gold["met_gt"][:2]),
                              _t(gold["met_gt_len"][:2]))
    assert bool(items[0].isnan().all()) and not bool(items[1].isnan().any())


# ---------------------------------------------------------------------------------------------------- metrics
def test_eval_item_and_eval_metrics_match_the_reference(gold, graphs):
    items, avg = NE.nav_metrics(graphs, _t(gold["met_scan"]), _t(gold["met_path"]), _t(gold["met_path_len"]),
                                _t(gold["met_action_steps"]), _t(gold["met_gt"]), _t(gold["met_gt_len"]))
    av, per = NE.metrics_dicts(items, avg)
    for k in NE.METRIC_FIELDS:
        want = gold[f"met_item_{k}"]
        got = np.asarray(per[k], dtype=np.float64)
        if k in ("action_steps", "trajectory_steps", "success", "oracle_success"):
            assert np.array_equal(got, want), k
        elif k == "DTW":
            assert np.array_equal(got, want), k           # the DP adds distances in the reference's order
        else:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=k)
    for k, v in av.items():
        np.testing.assert_allclose(v, float(gold[f"met_avg_{k}"]), rtol=1e-12, atol=0, err_msg=k)
    np.testing.assert_allclose(per["CLS"], gold["met_calcls"], rtol=1e-12, atol=0)
    assert 0 < np.mean(per["success"]) < 1


# ---------------------------------------------------------------------------------------------------- action step
def _state(B, N, device=DEV):
    return dict(ended=torch.zeros(B, dtype=torch.uint8, device=device),
                stop_scores=torch.zeros(B, N, dtype=torch.float32, device=device),
                stop_order=torch.full((B, N), -1, dtype=torch.int32, device=device),
                n_stop=torch.zeros(B, dtype=torch.int32, device=device))


def _logits(B, C, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * 2
    mask = torch.rand(B, C, generator=g) < 0.3
    mask[:, 0] = False
    mask[:, 1] = False
    x[mask] = -math.inf
    return x.to(DEV, dtype), (~mask).to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_argmax_and_teacher_actions_match_torch(dtype):
    B, C, N = 37, 23, 40
    x, _ = _logits(B, C, 1, dtype)
    cand = torch.randint(0, N, (B, C), device=DEV, dtype=torch.int32)
    cur = torch.randint(0, N, (B,), device=DEV, dtype=torch.int32)
    goal = torch.randint(0, N, (B,), device=DEV, dtype=torch.int32)
    st = _state(B, N)
    o = NE.action_step(x, "argmax", 0, 15, cand=cand, cur=cur, goal=goal, **st)
    want = x.float().max(1)[1]
    assert torch.equal(o["a_t"], want)
    stop = want == 0
    assert torch.equal(o["node"].long(), torch.where(stop, -1, cand.gather(1, want[:, None].int().long())[:, 0].long()))
    probs = torch.softmax(x.float(), 1)
    torch.testing.assert_close(st["stop_scores"].gather(1, cur[:, None].long())[:, 0], probs[:, 0], rtol=2e-6, atol=1e-7)
    ent = torch.distributions.Categorical(probs).entropy()
    torch.testing.assert_close(o["entropy"], ent, rtol=1e-5, atol=1e-6)

    tgt = torch.randint(0, C, (B,), device=DEV)
    tgt[3] = NE.IGNOREID
    st = _state(B, N)
    st["ended"][3] = 1
    o = NE.action_step(x, "teacher", 2, 15, targets=tgt, cand=cand, cur=cur, goal=goal, **st)
    assert torch.equal(o["a_t"], tgt)
    at_goal = cur == goal
    at_goal[3] = True
    nodes = cand.gather(1, tgt.clamp(min=0)[:, None])[:, 0]
    assert torch.equal(o["node"], torch.where(at_goal, -1, nodes))
    assert o["just_ended"][3].item() == 0 and st["n_stop"][3].item() == 0     # ended samples record nothing


def test_sample_draws_are_salted_and_follow_the_categorical_distribution():
    from vln_bevbert_amd.ops_core import RT
    C, B, N = 7, 65536, 4
    row = torch.tensor([[0.3, -1.0, 1.2, -math.inf, 0.0, 2.0, -0.5]], device=DEV)
    x = row.expand(B, C).contiguous()
    cand = torch.zeros(B, C, dtype=torch.int32, device=DEV)
    cur = torch.zeros(B, dtype=torch.int32, device=DEV)
    goal = torch.ones(B, dtype=torch.int32, device=DEV)
    RT.new_step(11)
    st = _state(B, N)
    a1 = NE.action_step(x, "sample", 0, 15, cand=cand, cur=cur, goal=goal, **st)["a_t"].clone()
    st = _state(B, N)
    a2 = NE.action_step(x, "sample", 0, 15, cand=cand, cur=cur, goal=goal, **st)["a_t"].clone()
    assert torch.equal(a1, a2)
    counts = torch.bincount(a1, minlength=C).cpu().numpy().astype(np.float64)
    p = torch.softmax(row, 1)[0].double().cpu().numpy()
    assert counts[3] == 0
    keep = p > 0
    chi2 = float((((counts - B * p) ** 2)[keep] / (B * p[keep])).sum())
    assert keep.sum() - 1 == 5
    assert chi2 < 25.7448, (chi2, counts, B * p)      # the 1 - 1e-4 quantile of chi-square with 5 degrees of freedom

    # captured once, replayed under two salts: the replays draw anew, the same salt draws the same
    xs = x[:256].clone()
    outs = {k: v.clone() for k, v in NE.action_step(xs, "sample", 0, 15, cand=cand[:256], cur=cur[:256],
                                                     goal=goal[:256], **_state(256, N)).items()}
    st = _state(256, N)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            NE.action_step(xs, "sample", 0, 15, cand=cand[:256], cur=cur[:256], goal=goal[:256], outs=outs, **st)
    torch.cuda.current_stream().wait_stream(s)
    draws = []
    for seed in (21, 22, 21):
        RT.new_step(seed)
        st["ended"].zero_()
        g.replay()
        torch.cuda.synchronize()
        draws.append(outs["rand"].clone())
    assert not torch.equal(draws[0], draws[1])
    assert torch.equal(draws[0], draws[2])


def test_expl_sample_explores_at_the_configured_rate_inside_the_mask():
    from vln_bevbert_amd.ops_core import RT
    RT.new_step(5)
    B, C, N = 65536, 9, 4
    x, _ = _logits(B, C, 3)
    g = torch.Generator().manual_seed(4)
    masks = (torch.rand(B, C, generator=g) < 0.5).to(torch.uint8).to(DEV)
    masks[:, 1] = 1
    cand = torch.zeros(B, C, dtype=torch.int32, device=DEV)
    cur = torch.zeros(B, dtype=torch.int32, device=DEV)
    o = NE.action_step(x, "expl_sample", 0, 15, cand=cand, cur=cur, goal=cur, masks=masks, expl_max_ratio=0.6,
                       **_state(B, N))
    explore = o["rand"] > 0.6
    rate = explore.double().mean().item()
    sd = math.sqrt(0.4 * 0.6 / B)
    assert abs(rate - 0.4) < 5 * sd, rate
    amax = x.max(1)[1]
    assert torch.equal(o["a_t"][~explore], amax[~explore])
    picked = masks[explore].gather(1, o["a_t"][explore][:, None])
    assert bool((picked == 1).all())
    assert (o["a_t"][explore] != amax[explore]).any()


def _host_twin(steps, feedback, max_len, cand, cur_seq, goal):
    """agent.py:523-534,581-612 for one sample: stop-score dict, stop rule, stop-node pick."""
    scores, ended, out = {}, False, []
    for t, (logits, a) in enumerate(steps):
        if ended:
            out.append(None)
            continue
        cur = cur_seq[t]
        p = torch.softmax(logits.float(), 0)
        scores[cur] = float(p[0])
        stop = cur == goal if feedback in ("teacher", "sample") else a == 0
        if stop or t == max_len - 1:
            best, node = -math.inf, None
            for k, v in scores.items():
                if v > best:
                    best, node = v, k
            out.append(("stop", node))
            ended = True
        else:
            out.append(("go", int(cand[t][a])))
    return out


def test_stop_scores_stop_rule_and_stop_node_follow_the_reference_loop():
    B, C, N, T = 8, 6, 12, 6
    torch.manual_seed(0)
    cand = torch.randint(0, N, (T, B, C), dtype=torch.int32, device=DEV)
    cur = torch.randint(0, 4, (T, B), dtype=torch.int32, device=DEV)     # few nodes: revisits overwrite scores
    goal = torch.full((B,), 3, dtype=torch.int32, device=DEV)
    logits = torch.randn(T, B, C, device=DEV)
    logits[:, :, 0] -= 1.0
    st = _state(B, N)
    got = [[None] * T for _ in range(B)]
    acts = []
    for t in range(T):
        o = NE.action_step(logits[t], "argmax", t, T, cand=cand[t], cur=cur[t], goal=goal, **st)
        acts.append(o["a_t"].cpu())
        for b in range(B):
            if o["just_ended"][b]:
                got[b][t] = ("stop", int(o["stop_node"][b]))
            elif o["node"][b] >= 0:
                got[b][t] = ("go", int(o["node"][b]))
    for b in range(B):
        steps = [(logits[t, b].cpu(), int(acts[t][b])) for t in range(T)]
        want = _host_twin(steps, "argmax", T, cand[:, b].cpu().numpy(), cur[:, b].cpu().numpy().tolist(), 3)
        assert got[b] == want, b
    assert bool(st["ended"].all())


# ---------------------------------------------------------------------------------------------------- IL loss
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_il_loss_and_gradient_equal_cross_entropy_with_ignore_index(dtype):
    B, C = 37, 29
    x, _ = _logits(B, C, 7, dtype)
    tgt = torch.randint(0, 2, (B,), device=DEV)
    tgt[::5] = NE.IGNOREID
    xa = x.clone().requires_grad_(True)
    loss = NE.il_loss(xa, tgt)
    (loss * 0.75).backward()
    xb = x.float().clone().requires_grad_(True)
    want = F.cross_entropy(xb, tgt, ignore_index=-100, reduction="sum")
    (want * 0.75).backward()
    torch.testing.assert_close(loss, want.detach(), rtol=1e-5, atol=1e-5)
    tol = dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else dict(rtol=1e-2, atol=4e-3)
    torch.testing.assert_close(xa.grad.float(), xb.grad, **tol)
    assert bool((xa.grad[::5] == 0).all())


def test_a_none_action_ends_the_sample_in_place_without_a_stop_pick():
    # teacher target = slot 0 ([stop], no viewpoint) away from the goal: agent.py:615 ends the sample (its action is
    # None), but just_ended stays 0, so there is no stop-node pick
    B, C, N = 3, 5, 8
    x = torch.randn(B, C, device=DEV)
    cand = torch.tensor([[-1, 4, 5, 6, 7]] * B, dtype=torch.int32, device=DEV)
    cur = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)
    goal = torch.tensor([3, 3, 3], dtype=torch.int32, device=DEV)
    st = _state(B, N)
    o = NE.action_step(x, "teacher", 0, 15, targets=torch.tensor([0, 2, 1], device=DEV), cand=cand, cur=cur, goal=goal,
                       **st)
    assert o["node"].tolist() == [-1, 5, -1]
    assert o["just_ended"].tolist() == [0, 0, 1]           # sample 2 is at its goal: a stop
    assert o["stop_node"].tolist() == [-1, -1, 3]
    assert st["ended"].tolist() == [1, 0, 1]


def _floyd_point(rng, n):
    """FloydGraph (graph_utils.py:44-94) of a random connected graph: next-hop table, -1 = direct edge."""
    d = np.full((n, n), np.inf)
    np.fill_diagonal(d, 0)
    edges = [(i, int(rng.integers(i))) for i in range(1, n)] + [tuple(rng.choice(n, 2, replace=False)) for _ in range(n)]
    for i, j in edges:
        w = float(rng.uniform(1, 3))
        d[i, j] = d[j, i] = min(d[i, j], w)
    point = np.full((n, n), -1, dtype=np.int32)
    for k in range(n):
        for i in range(n):
            for j in range(n):
                if d[i, k] + d[k, j] < d[i, j]:
                    d[i, j] = d[i, k] + d[k, j]
                    point[i, j] = k
    return point


def test_trajectory_record_expands_the_map_path_like_devicegraphmap():
    rng = np.random.default_rng(3)
    B, Nm, Lt = 6, 24, 200
    point = np.stack([_floyd_point(rng, Nm) for _ in range(B)])
    node_scan = rng.permutation(300)[:B * Nm].reshape(B, Nm).astype(np.int32)

    def host_path(b, i, j):                      # DeviceGraphMap.path's recursion
        k = int(point[b, i, j])
        return [int(node_scan[b, j])] if k < 0 else host_path(b, i, k) + host_path(b, k, j)

    traj = torch.full((B, Lt), -1, dtype=torch.int32, device=DEV)
    traj[:, 0] = torch.from_numpy(node_scan[:, 0]).to(DEV)
    traj_len = torch.ones(B, dtype=torch.int32, device=DEV)
    n_seg = torch.zeros(B, dtype=torch.int32, device=DEV)
    overflow = torch.zeros(1, dtype=torch.int32, device=DEV)
    want = [[int(node_scan[b, 0])] for b in range(B)]
    cur = np.zeros(B, dtype=np.int64)
    for step in range(5):
        nxt = rng.integers(Nm, size=B)
        live = rng.random(B) < 0.8
        NE.traj_append(_t(point), _t(node_scan), _t(cur), _t(nxt), _t(live.astype(np.uint8)), traj, traj_len, n_seg,
                       overflow)
        for b in range(B):
            if live[b]:
                want[b] += [] if cur[b] == nxt[b] else host_path(b, int(cur[b]), int(nxt[b]))
                cur[b] = nxt[b]
    got = [traj[b, :traj_len[b]].tolist() for b in range(B)]
    assert got == want
    assert overflow.item() == 0
    # a record that is too short flags the overflow
    small = torch.zeros(B, 2, dtype=torch.int32, device=DEV)
    sl = torch.ones(B, dtype=torch.int32, device=DEV)
    far = torch.from_numpy(np.array([int(np.argmax([len(host_path(b, 0, j)) for j in range(Nm)])) for b in range(B)]))
    NE.traj_append(_t(point), _t(node_scan), torch.zeros(B, dtype=torch.int32, device=DEV), far.to(DEV),
                   torch.ones(B, dtype=torch.uint8, device=DEV), small, sl, torch.zeros_like(sl), overflow)
    assert overflow.item() == 1


def test_captured_step_supervision_equals_the_eager_one(gold, graphs):
    """expert + IL loss (+ its gradient) + action step captured in one hipGraph give the eager results bit for bit."""
    from vln_bevbert_amd.ops_core import RT
    p = "exp2_"
    B, C = gold[p + "cand"].shape
    ins = {k: _t(gold[p + k]) for k in ("scan", "cur", "cand", "visited", "ended", "gt", "gt_len", "traj", "traj_len")}
    logits = torch.randn(B, C, device=DEV)
    logits[:, C - 1] = -math.inf
    N = graphs.n_max

    def step(x, st, outs=None):
        tg = NE.expert_targets(graphs, ins["scan"], ins["cur"], ins["cand"], ins["visited"], ins["ended"], ins["gt"],
                               ins["gt_len"], 0, "ndtw", ins["traj"], ins["traj_len"], out=st["tg"])
        loss = NE.il_loss(x, tg)
        (g,) = torch.autograd.grad(loss, x)
        o = NE.action_step(x.detach(), "sample", 0, 20, cand=ins["cand"], cur=ins["cur"],
                           goal=ins["gt"][torch.arange(B, device=DEV), ins["gt_len"].long() - 1],
                           ended=st["ended"], stop_scores=st["sc"], stop_order=st["so"], n_stop=st["ns"], outs=outs)
        return tg, loss, g, o

    def fresh():
        return {"tg": torch.empty(B, dtype=torch.int64, device=DEV), "ended": ins["ended"].clone(),
                "sc": torch.zeros(B, N, device=DEV), "so": torch.zeros(B, N, dtype=torch.int32, device=DEV),
                "ns": torch.zeros(B, dtype=torch.int32, device=DEV)}

    RT.new_step(3)
    x = logits.clone().requires_grad_(True)
    e_tg, e_loss, e_g, e_o = step(x, fresh())
    e = [e_tg.clone(), e_loss.detach().clone(), e_g.clone()] + [v.clone() for v in e_o.values()]

    st = fresh()
    xs = logits.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(xs, fresh())                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c_tg, c_loss, c_g, c_o = step(xs, st)
    st["ended"].copy_(ins["ended"])
    st["ns"].zero_()
    RT.new_step(3)
    g.replay()
    torch.cuda.synchronize()
    c = [c_tg, c_loss.detach(), c_g] + list(c_o.values())
    for a, b in zip(e, c):
        assert torch.equal(a, b)
    assert e_tg.cpu().tolist() == gold[p + "target"].tolist()
