"""Training through the device ghost-node map of the continuous-environment (CE) agent (csrc/ce_train.hip).

In the reference the panorama embeddings reach the loss through the map and nowhere else: ``GraphMap.node_embeds`` /
``ghost_embeds`` hold live tensors (ss_trainer_BEV.py:1060-1066), ``_nav_gmap_variable`` stacks them (:552-556,589),
``rollout('train')`` sums the steps' cross entropies (:1094), divides by ``total_actions`` (:1257) and calls backward
once (:694-698).  ``ce_map.CEGraphMap`` keeps the embeddings in raw device arrays and takes them detached, so on its own
it gives the panorama encoder no gradient at all.  This module adds what a training rollout needs:

    CEMapTape       records what every ``update`` did and connects ``nav_gmap_variable``'s ``gmap_img_fts`` to the
                    ``avg_pano_embeds`` / ``pano_embeds`` of every recorded step    -> bevbert_ce_tape_record, bevbert_ce_embeds_bwd
    sample_action   Categorical(nav_probs).sample() with the teacher override (:1097-1100)  -> bevbert_ce_sample_action
    train_step      one step of the reference's training rollout (:1018-1100,1110-1179) from the existing device stages
    finish          ml_weight * loss / total_actions

Wiring of the tape.  Step s's update is an autograd node ``write_s(pano_s, avg_s, tok_{s-1}) -> tok_s`` and step t's
listing a node ``read_t(tok_t) -> gmap_img_fts_t``; the tokens carry no values, only the dependency.  Backward of
``read_t`` launches bevbert_ce_embeds_bwd ONCE: it adds the step's d gmap_img_fts into the fp32 accumulators
``d_avg[s]`` / ``d_pano[s]`` of every s <= t.  ``write_s`` can only run after ``read_s`` and ``write_{s+1}``, hence after
every ``read_t`` with t >= s, and hands ``d_pano[s]`` / ``d_avg[s]`` over, cast once to the inputs' dtype.  T launches per
rollout, no atomics, and a fixed summation order: an accumulator row receives the consumer steps in the order backward
visits them -- for a loss summed over the steps, from the last step to the first.  One backward per episode: a second
one would add into the same accumulators (``begin_episode`` clears them).

The simulator stays with the caller, as in ce_map.py: poses, the live mask and goal distances come in, ``to_reference``
actions go out.  Training steps run eagerly; nothing here synchronises.
"""
import torch

from . import lib
from . import nav_expert
from . import waypoint


class _Write(torch.autograd.Function):
    """write_s: the map took (a detached copy of) pano / avg at tape step s."""

    @staticmethod
    def forward(ctx, pano, avg, tok, tape, s):
        ctx.tape, ctx.s, ctx.episode = tape, s, tape.episode
        ctx.dtypes = (pano.dtype, avg.dtype)
        return tok.new_empty(1)                     # carries the dependency only; nobody reads it

    @staticmethod
    def backward(ctx, dtok):
        tape, s = ctx.tape, ctx.s
        tape._check(ctx.episode)
        need = ctx.needs_input_grad
        return (tape.d_pano[s].to(ctx.dtypes[0], copy=True) if need[0] else None,
                tape.d_avg[s].to(ctx.dtypes[1], copy=True) if need[1] else None,
                tape._zero if need[2] else None, None, None)


class _Read(torch.autograd.Function):
    """read_t: the listing of tape step t; its gmap_img_fts depends on every write so far."""

    @staticmethod
    def forward(ctx, tok, tape, t):
        ctx.tape, ctx.t, ctx.episode = tape, t, tape.episode
        tape._nav = tape.map.nav_gmap_variable()
        return tape._nav["gmap_img_fts"]

    @staticmethod
    def backward(ctx, dG):
        tape = ctx.tape
        tape._check(ctx.episode)
        tape.embeds_bwd(ctx.t, dG)
        return tape._zero, None, None


class CEMapTape:
    """The record of one episode of ``map`` (a ``ce_map.CEGraphMap``) and the accumulators of its adjoint.

    ``max_steps`` T updates per episode, ``cand_capacity`` C candidates per step (waypoint_step: 5), ``pano_rows`` L rows of
    ``pano_embeds``.  Per-episode device stores: cur (T,B) i32, live (T,B) u8, slot / row (T,B,C) i32, ids (T,B,G) i64,
    cnt (T,B,Gh) i32 and the fp32 accumulators d_avg (T,B,H), d_pano (T,B,L,H) (include/bevbert_hip.h)."""

    def __init__(self, map, max_steps, cand_capacity, pano_rows):
        T, C, L = int(max_steps), int(cand_capacity), int(pano_rows)
        if not (T >= 1 and 1 <= C <= 16 and L >= 1):
            raise ValueError(f"CEMapTape: max_steps {T} (>= 1), cand_capacity {C} (1..16), pano_rows {L} (>= 1)")
        self.map, self.T, self.C, self.L = map, T, C, L
        B, dev = map.B, map.device

        def z(shape, dt):
            return torch.zeros(shape, dtype=dt, device=dev)
        i32 = torch.int32
        self.cur, self.live = z((T, B), i32), z((T, B), torch.uint8)
        self.slot, self.row = z((T, B, C), i32), z((T, B, C), i32)
        self.ids, self.cnt = z((T, B, map.G), torch.int64), z((T, B, map.Gh), i32)
        self.d_avg, self.d_pano = z((T, B, map.H), torch.float32), z((T, B, L, map.H), torch.float32)
        self._last_cur = z((B,), i32)
        self._zero = z((1,), torch.float32)          # the first token, and the (defined, zero) gradient of every token
        self.episode = 0
        self.begin_episode()

    def begin_episode(self):
        """Empty the map (``CEGraphMap.reset``) and the tape for the next batch of episodes: fills on the current stream."""
        self.map.reset()
        for x in (self.live, self.ids, self.cnt, self.d_avg, self.d_pano):
            x.zero_()
        for x in (self.cur, self.slot, self.row, self._last_cur):
            x.fill_(-1)
        self.episode += 1              # autograd nodes of an earlier episode refuse to run against the new record
        self.n, self._tok, self._nav = 0, None, None

    def _check(self, episode):
        if episode != self.episode:
            raise lib.BevBertHipError("CEMapTape: backward of an episode whose tape was cleared by begin_episode()")

    def update(self, step_id, cand_count, cand_angles, cand_distances, avg_pano_embeds, pano_embeds, nav_types,
               cur_pos=None, heading=None, live=None):
        """``CEGraphMap.update`` (same arguments, same cand_slot, the same bits in the map) recorded as tape step
        ``n`` = the number of updates since ``begin_episode``; ``avg_pano_embeds`` / ``pano_embeds`` stay in the autograd
        graph: what a later ``nav_gmap_variable`` lists of them carries their gradient."""
        m, s = self.map, self.n
        if s >= self.T:
            raise lib.BevBertHipError(f"CEMapTape: more than max_steps = {self.T} updates in one episode")
        if tuple(pano_embeds.shape[1:2]) != (self.L,) or cand_angles.shape[1] != self.C:
            raise ValueError(f"CEMapTape.update: pano_embeds (B,{self.L},H) and {self.C} candidates per step expected")
        slot = m.update(step_id, cand_count, cand_angles, cand_distances, avg_pano_embeds, pano_embeds, nav_types,
                        cur_pos=cur_pos, heading=heading, live=live)
        lib.call("bevbert_ce_tape_record", lib.ptr(m.t["cur_vp"]), m._live, lib.ptr(slot), lib.ptr(nav_types.contiguous()),
                 m.B, m.N, self.C, self.L, lib.ptr(self._last_cur), lib.ptr(self.cur[s]), lib.ptr(self.live[s]),
                 lib.ptr(self.slot[s]), lib.ptr(self.row[s]), lib.stream())
        self.n = s + 1
        if torch.is_grad_enabled() and (pano_embeds.requires_grad or avg_pano_embeds.requires_grad or
                                        (self._tok is not None and self._tok.requires_grad)):
            self._tok = _Write.apply(pano_embeds, avg_pano_embeds, self._zero if self._tok is None else self._tok, self, s)
        return slot

    def nav_gmap_variable(self):
        """``CEGraphMap.nav_gmap_variable``'s dict with the same bits; ``gmap_img_fts`` is an autograd output connected to
        the embeddings of every recorded step.  Records the listing (gmap_ids, the ghosts' observation counts) as the
        last update's step."""
        if self.n == 0:
            raise lib.BevBertHipError("CEMapTape.nav_gmap_variable: no update recorded yet")
        t = self.n - 1
        if self._tok is not None and self._tok.requires_grad and torch.is_grad_enabled():
            fts = _Read.apply(self._tok, self, t)
            o = dict(self._nav)
            o["gmap_img_fts"] = fts
        else:
            o = self.map.nav_gmap_variable()
        self._nav = None
        self.ids[t].copy_(o["gmap_ids"])
        self.cnt[t].copy_(self.map.t["g_npos"])
        return o

    def embeds_bwd(self, t, dG):
        """Add d gmap_img_fts of tape step t, ``dG`` (B,G,H) in the map's dtype, into d_avg[s] / d_pano[s] of every
        s <= t (one launch; autograd calls this)."""
        m = self.map
        if tuple(dG.shape) != (m.B, m.G, m.H) or dG.dtype != m.dtype:
            raise ValueError(f"CEMapTape.embeds_bwd: d gmap_img_fts ({m.B},{m.G},{m.H}) {m.dtype} expected")
        dG = dG.contiguous()
        lib.call("bevbert_ce_embeds_bwd", lib.ptr(dG), lib.dtype_code(dG), int(t), self.T, m.B, m.N, m.Gh, self.C, self.L, m.H,
                 lib.ptr(self.cur), lib.ptr(self.live), lib.ptr(self.slot), lib.ptr(self.row), lib.ptr(self.ids),
                 lib.ptr(self.cnt), lib.ptr(self.d_avg), lib.ptr(self.d_pano), lib.stream())


def sample_action(logits, teacher, sample_ratio, seed, t):
    """ss_trainer_BEV.py:1097-1100: ``Categorical(softmax(logits)).sample()``, the teacher's action where
    ``rand <= sample_ratio``.  logits (B,G) fp32 / bf16 with -inf on masked slots, teacher (B) int64 (-100 passes
    through).  Returns (a_t (B) int64, u0 (B) f32 the draw of the sample, u1 (B) f32 the draw of the override); the
    draws are hashed from (seed, t) and the step salt under a domain of their own (csrc/common.h)."""
    if not (logits.is_cuda and logits.dim() == 2 and logits.dtype in (torch.float32, torch.bfloat16)):
        raise lib.BevBertHipError("sample_action: (B,G) fp32 / bf16 device logits only")
    B, G = logits.shape
    if teacher.dtype != torch.int64 or tuple(teacher.shape) != (B,) or teacher.device != logits.device:
        raise ValueError("sample_action: teacher (B) int64 on the logits' device")
    a_t = torch.empty(B, dtype=torch.int64, device=logits.device)
    u0, u1 = (torch.empty(B, dtype=torch.float32, device=logits.device) for _ in range(2))
    lib.call("bevbert_ce_sample_action", lib.ptr(logits.detach().contiguous()), lib.dtype_code(logits), B, G,
             lib.ptr(teacher.contiguous()), float(sample_ratio), int(seed) & 0xFFFFFFFF, int(t), lib.ptr(a_t), lib.ptr(u0),
             lib.ptr(u1), lib.stream())
    return a_t, u0, u1


def pano_embed(model, vp_inputs):
    """Mode 'panorama' and its masked mean (ss_trainer_BEV.py:1027-1033), in autograd: (pano_embeds (B,L,H), avg (B,H))."""
    pano, pm = model.img_embeddings.embed(vp_inputs["rgb_fts"], vp_inputs["loc_fts"], vp_inputs["nav_types"],
                                          vp_inputs["view_lens"], model.embeddings.token_type_embeddings,
                                          view_dep_fts=vp_inputs["dep_fts"])
    avg = (pano * pm.unsqueeze(2)).sum(1) / pm.sum(1, keepdim=True)
    return pano, avg


def train_step(model, predictor, tape, step_id, txt_embeds, txt_masks, rgb_embeds, depth_embeds, rgb_grid, depth_grid,
               cur_pos, heading, live, cur_dist_to_goal, ghost_goal_dist, loss_sum=None, sample_ratio=0.75, seed=0,
               last_step=False, waypoint_aug=False, consume_ghost=True, pano_grad=True):
    """One step of the reference's training rollout (ss_trainer_BEV.py:1018-1100,1110-1179) on the device:
    waypoint_step, the panorama embed and its masked mean, ``tape.update``, ``remember_pano``,
    ``tape.nav_gmap_variable``, ``bev_inputs``, ``forward_navigation_per_step(sap_fusion=...)``, ``record_stop_scores``,
    ``teacher_index``, ``nav_expert.il_loss`` added to ``loss_sum``, the action draw, ``act``.

    ``step_id`` is the reference's stepk + 1 (>= 1; the draws use step_id - 1 as their t); rgb_embeds (B*12, 512) /
    depth_embeds (B*12, 128, 4, 4) are the waypoint backbones' outputs, rgb_grid (B,12,hw*hw,C) / depth_grid (B,12,hw,hw)
    the frozen grid features and depths of the panorama; cur_pos (B,3), heading (B), live (B) are host values;
    cur_dist_to_goal (B) and ghost_goal_dist (B,Gh) device float64, measured by the caller.  Returns a dict: loss_sum (the
    running sum, in autograd), a_t, rec (``map.to_reference(rec)`` gives the simulator's actions and is the caller's one
    read-back), fused_logits, teacher, cand_slot, u0, u1, pano, avg, nav, bev.  ``pano_grad=False`` takes this step's
    panorama pass as a constant (backpropagation through the map truncated at this step); the forward values are the
    same.  Nothing here synchronises."""
    m = tape.map
    t = int(step_id) - 1
    wp = waypoint.waypoint_step(predictor, rgb_embeds, depth_embeds, in_train=waypoint_aug, seed=seed, t=t)
    vp = wp["vp_inputs"]
    pano, avg = pano_embed(model, vp)
    if not pano_grad:
        pano, avg = pano.detach(), avg.detach()
    slot = tape.update(step_id, wp["cand_count"], wp["cand_angles"], wp["cand_distances"], avg, pano, vp["nav_types"],
                       cur_pos=cur_pos, heading=heading, live=live)
    m.remember_pano(rgb_grid, depth_grid)
    nav = tape.nav_gmap_variable()
    bev = m.bev_inputs()
    out = model.forward_navigation_per_step(
        txt_embeds=txt_embeds, txt_masks=txt_masks, gmap_img_embeds=nav["gmap_img_fts"], gmap_step_ids=nav["gmap_step_ids"],
        gmap_pos_fts=nav["gmap_pos_fts"], gmap_masks=nav["gmap_masks"], gmap_pair_dists=nav["gmap_pair_dists"],
        gmap_visited_masks=nav["gmap_visited_masks"], gmap_vpids=None, bev_fts=bev["bev_fts"], bev_pos_fts=bev["bev_pos_fts"],
        bev_masks=bev["bev_masks"], bev_nav_masks=bev["bev_nav_masks"], bev_cand_idxs=bev["bev_cand_idxs"],
        bev_cand_vpids=None, obj_embeds=None, obj_masks=None, sap_fusion=(bev["src"], bev["vis_c"]))
    logits = out["fused_logits"]
    m.record_stop_scores(torch.softmax(logits.detach().float(), 1)[:, 0])
    teacher = m.teacher_index(cur_dist_to_goal, ghost_goal_dist)
    loss = nav_expert.il_loss(logits, teacher)
    loss_sum = loss if loss_sum is None else loss_sum + loss
    a_t, u0, u1 = sample_action(logits, teacher, sample_ratio, seed, t)
    rec = m.act(a_t, last_step=last_step, consume_ghost=consume_ghost, gmap_ids=nav["gmap_ids"])
    return {"loss_sum": loss_sum, "a_t": a_t, "rec": rec, "fused_logits": logits, "teacher": teacher, "cand_slot": slot,
            "u0": u0, "u1": u1, "pano": pano, "avg": avg, "nav": nav, "bev": bev}


def finish(loss_sum, total_actions, ml_weight=1.0):
    """ss_trainer_BEV.py:1257 and :694: the rollout's loss, ``ml_weight * loss_sum / total_actions`` (total_actions = the
    number of environments summed over the steps taken)."""
    return ml_weight * loss_sum / total_actions
