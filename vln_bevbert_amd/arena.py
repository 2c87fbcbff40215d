"""Flat parameter / gradient / optimiser-state arenas (memory laid out for one 288 GB HBM3E stack).

The reference keeps 567 separate parameter tensors, lets autograd allocate a gradient per tensor, copies them
into DDP buckets for NCCL, and steps a Python-loop AdamW over every tensor (pretrain_src/optim/adamw.py:53-112,
pretrain_src/utils/misc.py:64-77).  Here every parameter is a view into ONE fp32 buffer; gradients, Adam moments
and (in mixed precision) the bf16 compute copy are parallel buffers with the same offsets:

    params  fp32 [N]   masters            (N = 238.8 M + padding for the R2R model: 0.96 GB)
    grads   fp32 [N]   accumulation target of every backward kernel; the all-reduce runs on slices of it in place
    exp_avg, exp_avg_sq fp32 [N]
    shadow  bf16 [N]   refreshed by the AdamW kernel in the same pass that updates the masters

Tensors start on 1024-element boundaries so the optimiser kernel can use one flag byte per 1024-element chunk
(bit0 weight decay, bit1 "has had a gradient": the reference skips parameters whose .grad is None).  Parameters
listed in a *group* (packed QKV / KV projections) are laid out back to back so the group is one GEMM operand.
"""
import math

import torch

from . import lib
from .lib import ptr, stream
from .ops_core import call          # the traced C-ABI call (bench.py's kernel-timing pass)

CHUNK = 1024
NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")   # optim/misc.py:14 (substring match)


def _round_up(n, m):
    return (n + m - 1) // m * m


class ParamArena:
    _serial = 0          # arenas made so far in this process (fold_key)

    def __init__(self, module, device, compute_dtype=torch.float32, groups=()):
        """groups: iterable of lists of parameter names to lay out contiguously (same decay class)."""
        self.device = torch.device(device)
        self.compute_dtype = compute_dtype
        named = [(n, p) for n, p in module.named_parameters()]
        by_name = dict(named)
        in_group = {}
        for gi, g in enumerate(groups):
            for n in g:
                in_group[n] = gi
        layout, seen_groups = [], set()
        for n, p in named:
            if n in in_group:
                gi = in_group[n]
                if gi in seen_groups:
                    continue
                seen_groups.add(gi)
                layout.append(list(groups[gi]))
            else:
                layout.append([n])
        self.slices = {}
        off = 0
        seg_meta = []   # (start, end_padded, decay)
        for seg in layout:
            start = off
            decays = set()
            for n in seg:
                k = by_name[n].numel()
                self.slices[n] = (off, k)
                off += k
                decays.add(not any(nd in n for nd in NO_DECAY))
            assert len(decays) == 1, f"group {seg} mixes weight-decay classes"
            off = _round_up(off, CHUNK)
            seg_meta.append((start, off, decays.pop(), seg))
        self.numel = off
        self.n_params = sum(p.numel() for _, p in named)
        dev = self.device
        self.params = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(off, dtype=torch.float32, device=dev)
        self.exp_avg = None
        self.exp_avg_sq = None
        self.shadow = torch.zeros(off, dtype=compute_dtype, device=dev) if compute_dtype != torch.float32 else None
        self._flags_host = torch.zeros(off // CHUNK, dtype=torch.uint8)
        self._seg_of = {}
        for start, end, decay, seg in seg_meta:
            if decay:
                self._flags_host[start // CHUNK:end // CHUNK] |= 1
            for n in seg:
                self._seg_of[n] = (start // CHUNK, end // CHUNK)
        self.flags = self._flags_host.to(dev)
        self.chunk_steps = torch.zeros(off // CHUNK, dtype=torch.int32, device=dev)   # per-parameter state["step"]
        self._touched = set()
        self._flags_dirty = False
        # torch-API bridge (see publish_grads below)
        self.publish_grads = True
        self.allreduce_group = None        # set by train.ArenaDataParallel: gradients are averaged over it when published
        self.defer_allreduce = False       # ArenaDataParallel.no_sync()
        self._cb_queued = False
        self._fresh = []                   # parameters written during the running backward pass
        self._published = []               # parameters whose .grad currently aliases the arena
        self._param_versions = None
        self.step_count = 0
        self._scalars = torch.zeros(4, dtype=torch.float32, device=dev)       # [grad norm, clip multiplier, lr, -]
        self._partials = torch.zeros(1024, dtype=torch.float32, device=dev)
        # re-point every parameter at its arena view
        self.named = named
        for n, p in named:
            o, k = self.slices[n]
            view = self.params[o:o + k].view(p.shape)
            view.copy_(p.data.to(dev, torch.float32))
            p.data = view
            p.main_grad = self.grads[o:o + k].view(p.shape)
            p.compute = self.shadow[o:o + k].view(p.shape) if self.shadow is not None else p.data
            p.arena = self
            p.arena_name = n
        self._index = {n: i for i, (n, _) in enumerate(named)}
        # Fused fold (ops.ReduceQueue.store_ok): element ranges whose gradient only split-K folds write -- parameters with
        # >= 2 dimensions that are not the weight of an nn.Embedding (embedding_grad_kernel read-modify-writes those rows;
        # a decoder tied to the word embeddings IS that parameter).  Neighbours in a packed group merge into one range.
        # ``fold_store`` is the owner's switch: a trainer that zeroes the arena before every backward and exchanges no
        # gradients between the fold and the optimiser sets it (train.PretrainTrainer); everybody else never stores.
        self.fold_store = False
        ParamArena._serial += 1
        self.fold_key = ("arena", ParamArena._serial)       # context part of ReduceQueue's table-cache key
        tables = {id(m.weight) for m in module.modules() if isinstance(m, torch.nn.Embedding)}
        self._fold_ranges = []
        for o, k, _ in sorted((*self.slices[n], n) for n, p in named if p.dim() >= 2 and id(p) not in tables):
            if self._fold_ranges and self._fold_ranges[-1][1] == o:
                self._fold_ranges[-1][1] = o + k
            else:
                self._fold_ranges.append([o, o + k])
        self._fold_starts = [a for a, _ in self._fold_ranges]
        self._fold_comp = {}
        self.sync_shadow()
        # the compute copy matches the masters as of now: a later write through the parameters (load_state_dict after
        # wrap_model, as map_nav_src/r2r/agent_base.py does; a torch optimiser) moves a version counter and the next
        # forward refreshes the copy (maybe_refresh_shadow) -- also when that write happens before the FIRST forward
        self._param_versions = sum(p._version for _, p in named)

    # ---- views over contiguous groups --------------------------------------------------------
    def packed(self, names, shape):
        """(compute view, fp32 grad view) over consecutive parameters ``names`` reshaped to ``shape``."""
        o0, _ = self.slices[names[0]]
        total = 0
        for n in names:
            o, k = self.slices[n]
            assert o == o0 + total, f"{names} are not contiguous in the arena"
            total += k
        assert total == math.prod(shape)
        src = self.shadow if self.shadow is not None else self.params
        return src[o0:o0 + total].view(shape), self.grads[o0:o0 + total].view(shape)

    # ---- bookkeeping -------------------------------------------------------------------------
    def touch(self, param):
        n = param.arena_name
        if n not in self._touched:
            self._touched.add(n)
            a, b = self._seg_of[n]
            self._flags_host[a:b] |= 2
            self._flags_dirty = True
        if self.publish_grads:
            self._note_backward_write(param)

    # ---- torch-API bridge: the reference's loops run unchanged ---------------------------------
    # train_r2r.py:263-313 and map_nav_src/r2r/agent_base.py:174-217 do
    #     loss.backward(); [scaler.unscale_(opt)]; clip_grad_norm_(model.parameters(), 5.0); optimizer.step(); optimizer.zero_grad()
    # on ``p.grad`` with a torch optimiser.  Backward kernels here write into ``grads`` (``p.main_grad``) behind autograd's
    # back, so with ``publish_grads`` (default; PretrainTrainer turns it off and drives the arena itself):
    #   * the first gradient write of a backward pass queues an autograd-engine callback; at the end of that pass it issues
    #     the deferred weight-gradient work, joins the side streams (``sync``), averages over ``allreduce_group`` if one is
    #     set, and points ``p.grad`` of every parameter written so far at its arena view -- parameters that never received
    #     a gradient keep ``.grad is None`` exactly as under the reference (its AdamW skips them, optim/adamw.py:66);
    #   * ``optimizer.zero_grad()`` (set_to_none, torch's default) leaves stale sums in the arena: the next forward sees
    #     ``.grad is None`` on a published parameter and zeroes the arena first (``maybe_lazy_zero``, called from the model's
    #     forward entry); with set_to_none=False torch zeroes the views in place and nothing is needed;
    #   * a torch optimiser updates the fp32 masters through ``p``: the bf16 compute copy is refreshed at the next
    #     forward when any parameter's version counter moved (``maybe_refresh_shadow``).
    def _note_backward_write(self, param):
        if not self._cb_queued:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(self._publish)
            except RuntimeError:           # not inside a backward pass (a test touching parameters by hand)
                return
            self._cb_queued = True
        self._fresh.append(param)

    def _publish(self):
        self._cb_queued = False
        self.sync()
        # end of a backward pass in a caller-owned loop (nobody calls arena.zero_grad there): every queued reduction has
        # been issued and the current stream waits for the side streams, so the scratch ring may start over
        if self.device.type == "cuda":
            from . import ops
            ops.RT.scratch.reset()
        fresh = self._fresh
        if self.allreduce_group is not None and not self.defer_allreduce:
            import torch.distributed as dist
            dist.all_reduce(self.grads, group=self.allreduce_group)
            self.grads.div_(dist.get_world_size(self.allreduce_group))
            # DistributedDataParallel(find_unused_parameters=True) hands the reduced gradient of a parameter to EVERY
            # rank when any rank used it; a rank that did not use it locally must publish it too, or its optimiser
            # skips the update the other ranks make and the replicas drift apart: exchange the touched set (MAX)
            used = torch.zeros(len(self.named), dtype=torch.int32, device=self.grads.device)
            if fresh:
                used[torch.tensor(sorted({self._index[p.arena_name] for p in fresh}), device=used.device)] = 1
            dist.all_reduce(used, op=dist.ReduceOp.MAX, group=self.allreduce_group)
            mine = {id(p) for p in fresh}
            fresh = list(fresh) + [self.named[i][1] for i in used.nonzero().flatten().tolist()
                                   if id(self.named[i][1]) not in mine]
        for p in fresh:
            if p.grad is None:
                p.grad = p.main_grad
                self._published.append(p)
        self._fresh.clear()

    def maybe_lazy_zero(self):
        """Zero the gradient arena if the caller dropped published gradients (zero_grad(set_to_none=True)) -- of ANY
        published parameter: an optimiser that owns only some of them clears only those."""
        if self._published and any(p.grad is None for p in self._published):
            for p in self._published:
                p.grad = None
            self._published.clear()
            self.zero_grad()

    def maybe_refresh_shadow(self):
        """Rebuild the bf16 compute copy if a torch-API optimiser (or load_state_dict, or a DDP-style broadcast) wrote
        the fp32 masters through the parameters since the last look."""
        if self.shadow is None or not self.publish_grads:
            return
        v = 0
        for _, p in self.named:
            v += p._version
        if v != self._param_versions:
            if self._param_versions is not None:
                self.sync_shadow()
            self._param_versions = v

    def sync_shadow(self):
        if self.shadow is not None:
            call("bevbert_cast_f32", ptr(self.params), ptr(self.shadow), self.numel, lib.dtype_code(self.compute_dtype),
                 stream())

    def sync(self):
        """Make the current stream wait for the side streams that carry work of this step (weight-gradient stream,
        model branches).  Backward kernels write parameter gradients straight into ``grads`` as a side effect autograd
        does not see, so whoever reads or overwrites the arena next (optimiser, all-reduce, zero_grad, a test) must
        order itself after them.  Streams without pending work are left alone: inside a graph capture a wait on a
        stream that is not part of the capture would be an error."""
        if self.device.type == "cuda":
            from . import ops
            ops.WgradStream.flush_all()
            cur = torch.cuda.current_stream(self.device)
            for side in ops.Branches.side_streams():
                if ops.Branches.enabled or side not in ops.WgradStream.streams or ops.WgradStream.dirty:
                    cur.wait_stream(side)
            ops.WgradStream.dirty = False
            ops.WgradStream.release()

    # ---- fused fold: store-mode split-K folds that carry the clip norm (ops.ReduceQueue) --------------------------
    def store_ok(self, sink_ptr, n):
        """ReduceQueue's predicate: [sink_ptr, sink_ptr + 4 n) lies inside one range of fold-only parameters."""
        import bisect
        off, rem = divmod(sink_ptr - self.grads.data_ptr(), 4)
        if rem or off < 0 or off + n > self.numel:
            return False
        i = bisect.bisect_right(self._fold_starts, off) - 1
        return i >= 0 and off + n <= self._fold_ranges[i][1]

    def _arm_fold(self):
        """zero_grad: the arena is zero from here until the backward kernels write it, so the step's first accumulate-flush
        may store (and carry the clip norm) if the owner allows it; the record of the step before is void."""
        from . import ops
        ops.ReduceQueue.store_ok = self.store_ok if self.fold_store else None
        ops.ReduceQueue.fold_norm = None

    def _name_at(self, sink_ptr):
        off = (sink_ptr - self.grads.data_ptr()) // 4
        return next((n for n, (o, k) in self.slices.items() if o <= off < o + k), f"arena offset {off}")

    def fold_check_zero(self, stores):
        """Warm-up self-check (a): every (sink_ptr, n) about to be STOREd over reads exactly zero."""
        base = self.grads.data_ptr()
        views = [self.grads[(p - base) // 4:(p - base) // 4 + n] for p, n in stores]
        counts = torch.stack([torch.count_nonzero(v) for v in views]).tolist()
        bad = [(self._name_at(p), c) for (p, _), c in zip(stores, counts) if c]
        if bad:
            raise lib.BevBertHipError(
                "store-mode fold: the gradient of " + ", ".join(f"{n} ({c} non-zero elements)" for n, c in bad[:4])
                + " is not zero before the step's fold -- something other than the split-K fold writes it, or the arena "
                "was not zeroed for this step (BEVBERT_FOLD_STORE=0 turns the store mode off)")

    def _fold_complement(self, entry):
        """(device table, records, bytes) of bevbert_sumsq_tasks over every arena range no NORM task of ``entry`` covers;
        its slots follow the entry's.  Built in a warm-up step, kept with the arena."""
        ent = self._fold_comp.get(id(entry))
        if ent is not None and ent[0] is entry:
            return ent[1:]
        if torch.cuda.is_current_stream_capturing():
            raise lib.BevBertHipError("fold-norm complement table missing during graph capture (warm-up steps build it)")
        import numpy as np
        base, recs, pos = self.grads.data_ptr(), [], 0
        for p, n, _ in sorted(entry["norm_jobs"]) + [(base + 4 * self.numel, 0, 0)]:
            o = (p - base) // 4
            for a in range(pos, o, 16384):                  # (tensors start on 1024-element boundaries; n % 4 == 0)
                recs.append((base + 4 * a, (min(a + 16384, o) - a) // 4))
            pos = o + n
            assert pos % 4 == 0, "fold sinks are float4-aligned"
        from . import ops
        if entry["nslots"] + len(recs) > ops.ReduceQueue.SLOT_CAPACITY:
            return None
        t = np.zeros(len(recs), dtype=np.dtype([("ptr", "<u8"), ("n4", "<u4"), ("slot", "<u4")]))
        if recs:
            t["ptr"], t["n4"] = zip(*recs)
        t["slot"] = entry["nslots"] + np.arange(len(recs))
        dev = torch.from_numpy(t.view(np.uint8).copy()).to(self.device)
        if len(self._fold_comp) > 64:
            self._fold_comp.clear()
        self._fold_comp[id(entry)] = (entry, dev, len(recs), 16 * int(t["n4"].sum()))
        return dev, len(recs), 16 * int(t["n4"].sum())

    def _clip_from_fold(self, pre_scale, max_norm):
        """The fused form of bevbert_grad_norm_clip; False when this step's fold left no record (the caller falls back)."""
        from . import ops
        rec, ops.ReduceQueue.fold_norm = ops.ReduceQueue.fold_norm, None         # consumed once
        if rec is None or rec["owner"] is not self:
            return False
        entry = rec["entry"]
        comp = self._fold_complement(entry)
        if comp is None:
            return False
        table, ntasks, _ = comp
        slots = ops.ReduceQueue.register_slots(self.device)
        call("bevbert_sumsq_tasks", table.data_ptr(), ntasks, stream())
        call("bevbert_clip_from_slots", ptr(slots), entry["nslots"] + ntasks, pre_scale, max_norm, ptr(self._scalars),
             stream())
        if entry["fresh"] and not torch.cuda.is_current_stream_capturing():
            entry["fresh"] = False
            self._fold_check_norm(entry, slots, pre_scale)
        return True

    def _fold_check_norm(self, entry, slots, pre_scale):
        """Warm-up self-check (b), once per table: the fused norm equals the norm of the whole arena to 1e-5."""
        want = float(torch.linalg.vector_norm(self.grads, dtype=torch.float64)) * pre_scale
        got = float(self._scalars[0])
        if abs(got - want) <= 1e-5 * want or (got == 0.0 and want == 0.0):
            return
        base, culprit = self.grads.data_ptr(), "a range outside the folds"
        for p, n, s0 in entry["norm_jobs"]:
            o = (p - base) // 4
            w = float(self.grads[o:o + n].double().pow(2).sum())
            g = float(slots[s0:s0 + (n // 4 + 4095) // 4096].double().sum())
            if abs(g - w) > 1e-5 * max(w, 1e-30):
                culprit = self._name_at(p)
                break
        raise lib.BevBertHipError(
            f"fused gradient norm {got!r} differs from the arena's {want!r}: the gradient of {culprit} changed after the "
            "step's fold (BEVBERT_FOLD_STORE=0 turns the fused norm off)")

    def backward_done(self):
        """Call after ``loss.backward()`` when an external loop / optimiser reads the gradients: issues the deferred
        weight-gradient and reduction launches and makes the current stream wait for them (== ``sync``)."""
        self.sync()

    def zero_grad(self, overlap=False):
        """Zero the gradient arena.  ``overlap=True`` (the trainer's step): the 0.96 GB fill goes to a side stream, ordered
        behind everything enqueued so far (the previous step's AdamW reads the gradients), and runs beside the forward
        pass -- which is bound by the matrix cores and leaves HBM idle; ``wait_zero()`` joins it before backward."""
        self.sync()
        if self.device.type == "cuda":
            from . import ops
            ops.RT.scratch.reset()        # partial-sum addresses repeat from step to step (ops.ReduceQueue caches on them)
            self._arm_fold()
            if overlap:
                if getattr(self, "_zero_stream", None) is None:
                    from .hwqueues import side_stream
                    self._zero_stream = side_stream(self.device)
                self._zero_stream.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(self._zero_stream):
                    call("bevbert_zero", ptr(self.grads), self.grads.numel() * 4, stream())
                self._zero_pending = True
                return
            call("bevbert_zero", ptr(self.grads), self.grads.numel() * 4, stream())
            return
        self.grads.zero_()

    def wait_zero(self):
        """Order the current stream behind a ``zero_grad(overlap=True)`` (no-op otherwise)."""
        if getattr(self, "_zero_pending", False):
            torch.cuda.current_stream(self.device).wait_stream(self._zero_stream)
            self._zero_pending = False

    def load_state_dict_into(self, module, sd, strict=True):
        out = module.load_state_dict(sd, strict=strict)     # copies in place into the arena views
        self.sync_shadow()
        return out

    # ---- optimiser ---------------------------------------------------------------------------
    def set_lr(self, lr):
        """Learning rate of the next optimiser step, kept in device memory (one 4-byte fill on the stream): the AdamW
        kernel reads it there, so a step captured in a hipGraph follows the schedule without being re-captured."""
        self._scalars[2:3].fill_(float(lr))
        self._lr_set = True

    def upload_flags(self):
        """Host -> device copy of the per-chunk flags when a parameter was touched for the first time (never inside a
        graph capture: the copy reads pageable host memory)."""
        if self._flags_dirty:
            self.flags.copy_(self._flags_host, non_blocking=True)
            self._flags_dirty = False

    def clip_and_step(self, lr=None, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, max_norm=5.0, grad_pre_scale=1.0,
                      fused_norm=False):
        """clip_grad_norm_(max_norm) + AdamW.step (train_r2r.py:295-313) in three launches, no host sync.
        ``lr=None``: use the device-resident learning rate as set by ``set_lr`` (graph-captured steps).
        ``fused_norm``: the caller has not touched ``grads`` since the backward pass that followed ``zero_grad``: when that
        pass's single fold left its sums of squares behind (ops.ReduceQueue.fold_norm), the norm is taken from them and
        only the rest of the arena is read; in every other case, and by default, bevbert_grad_norm_clip reads it all."""
        self.sync()
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.params)
            self.exp_avg_sq = torch.zeros_like(self.params)
        if lr is not None:
            self.set_lr(lr)
        elif not getattr(self, "_lr_set", False):
            raise RuntimeError("clip_and_step(lr=None) reads the device-resident learning rate: call set_lr() first "
                               "(the slot starts at 0, which would silently turn AdamW and its weight decay into a no-op)")
        if not torch.cuda.is_current_stream_capturing():
            self.upload_flags()
        self.step_count += 1
        max_norm = float(max_norm if max_norm is not None else -1.0)
        if not (fused_norm and self._clip_from_fold(float(grad_pre_scale), max_norm)):
            call("bevbert_grad_norm_clip", ptr(self.grads), self.numel, float(grad_pre_scale), max_norm,
                 ptr(self._partials), ptr(self._scalars), stream())
        call("bevbert_adamw_step", ptr(self.params), ptr(self.grads), ptr(self.exp_avg), ptr(self.exp_avg_sq),
             ptr(self.shadow), ptr(self.flags), ptr(self.chunk_steps), self.numel, self._scalars[1:].data_ptr(),
             self._scalars[2:].data_ptr(), 0.0, float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
             stream())

    def grad_norm(self):
        """L2 norm computed by the last clip_and_step (device scalar; reading it syncs)."""
        return self._scalars[0]
