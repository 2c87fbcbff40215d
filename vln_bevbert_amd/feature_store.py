"""Device-resident store of the per-viewpoint grid features.

The reference reads, for every sample of every batch, the 12 x 14 x 14 CLIP patch features of the current viewpoint from
HDF5 (fp16 on disk), widens them to fp32, one-hot encodes the semantic ids in float64 and ships ~8 MB per sample to the
GPU (pretrain_src/data/dataset.py:110-118,397-440; 462 MB per step at batch 64).  R2R has 10 567 viewpoints:
12*196*768 fp16 = 3.6 MB each, 38 GB in all -- it fits in a corner of the MI355X's 288 GB.  So the store keeps

    rgbs    (N, 2352, 768) fp16      as on disk
    depths  (N, 12, 14, 14) fp32     stored / depth_scale, as on disk
    sems    (N, 2352)       uint8    class ids, as on disk

resident in HBM, a batch is described by B row numbers, and the splat kernel reads its points straight from the store
rows (``sample_rows`` of bevbert_bev_splat_mean): no per-step H2D traffic, no batch copy, and the fp16 -> fp32 widening
happens in the kernel's registers.
"""
import numpy as np
import torch


class GridFeatureStore:
    def __init__(self, keys, rgbs, depths, sems, device):
        """keys: N strings '<scan>_<viewpoint>' (the reference's HDF5 keys); rgbs (N, V, hw*hw | hw, hw, C) fp16/fp32;
        depths (N, V, hw, hw); sems (N, V, hw, hw) or (N, P) integer class ids."""
        keys = list(keys)
        N = len(keys)
        rgbs, depths, sems = (torch.as_tensor(np.asarray(t)) if not torch.is_tensor(t) else t for t in (rgbs, depths, sems))
        assert rgbs.shape[0] == N and depths.shape[0] == N and sems.shape[0] == N
        self.V, self.hw = int(depths.shape[1]), int(depths.shape[-1])
        self.C = int(rgbs.shape[-1])
        self.P = self.V * self.hw * self.hw
        self.row = {k: i for i, k in enumerate(keys)}
        assert len(self.row) == N, "duplicate keys"
        self.device = torch.device(device)
        self.rgbs = rgbs.reshape(N, self.P, self.C).to(self.device, torch.float16).contiguous()
        self.depths = depths.reshape(N, self.V, self.hw, self.hw).to(self.device, torch.float32).contiguous()
        self.sems = sems.reshape(N, self.P).to(self.device, torch.uint8).contiguous()

    def __len__(self):
        return len(self.row)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.rgbs, self.depths, self.sems))

    def rows(self, keys):
        """(B,) int32 device tensor of store rows for a list of '<scan>_<viewpoint>' keys (one small H2D copy)."""
        try:
            idx = [self.row[k] for k in keys]
        except KeyError as e:
            raise KeyError(f"viewpoint {e.args[0]!r} is not in the grid-feature store") from None
        return torch.tensor(idx, dtype=torch.int32).to(self.device, non_blocking=True)

    def attach(self, batch, keys):
        """Replace the per-batch grid tensors of a collated batch by references into the store:
        GlocalTextPathCMTPreTraining.lift_splat then reads 'grid_store' / 'grid_rows' instead of rgbs / depths / sems."""
        for k in ("rgbs", "depths", "sems"):
            batch.pop(k, None)
        batch["grid_store"] = self
        batch["grid_rows"] = self.rows(keys)
        return batch

    def gather(self, rows):
        """Materialised (rgbs fp16, depths, sems) of a batch -- what the zero-copy path avoids; used by the tests."""
        r = rows.long()
        return self.rgbs.index_select(0, r), self.depths.index_select(0, r), self.sems.index_select(0, r)


class ViewFeatureStore:
    """Resident panorama view features: (N, 36, Ds) fp16 as on disk (38 MB at R2R's 10 567 viewpoints and Ds = 768 + class
    probabilities: 1.2 GB).  The reference reads a viewpoint's 36 rows from HDF5, widens them to fp32, re-orders them per
    step and ships them (pretrain_src/data/dataset.py:460-469, :587-609); here a batch names its panoramas by store row and
    ``pano_rows`` (csrc/path_data.hip) gathers them.  Ds may exceed the model's image_feat_size: the reference slices
    ``[:, :image_feat_size]`` off rows that carry class probabilities behind the features, and so does the gather."""

    def __init__(self, keys, view_fts, device):
        """keys: N strings '<scan>_<viewpoint>'; view_fts (N, 36, Ds) fp16 / fp32 array or tensor."""
        self.keys = [str(k) for k in keys]
        self.row = {k: i for i, k in enumerate(self.keys)}
        assert len(self.row) == len(self.keys), "duplicate keys"
        fts = torch.as_tensor(np.asarray(view_fts)) if not torch.is_tensor(view_fts) else view_fts
        assert fts.dim() == 3 and fts.shape[0] == len(self.keys), tuple(fts.shape)
        self.device = torch.device(device)
        self.fts = fts.to(self.device, torch.float16).contiguous()
        self.device = self.fts.device           # with its index ('cuda' -> 'cuda:0'): tensors are compared against it
        self.n_views, self.Ds = int(fts.shape[1]), int(fts.shape[2])

    @classmethod
    def from_hdf5(cls, img_ft_file, device, keys=None, reader=None):
        """From the reference's view-feature file (one (36, Ds) dataset per '<scan>_<viewpoint>'), opened like
        feature_cache.convert_hdf5 opens the grid files.  ``keys``: the rows wanted, in order (default: the file's)."""
        from . import hdf5_reader
        with (reader or hdf5_reader.open_file)(img_ft_file) as f:
            keys = list(f.keys()) if keys is None else list(keys)
            fts = np.stack([np.asarray(f[k][...]).astype(np.float16) for k in keys])
        return cls(keys, fts, device)

    def __len__(self):
        return len(self.keys)

    def nbytes(self):
        return self.fts.numel() * self.fts.element_size()

    def rows(self, keys):
        """(T,) int32 device tensor of store rows for a list of '<scan>_<viewpoint>' keys (one small H2D copy)."""
        try:
            idx = [self.row[k] for k in keys]
        except KeyError as e:
            raise KeyError(f"viewpoint {e.args[0]!r} is not in the view-feature store") from None
        return torch.tensor(idx, dtype=torch.int32).to(self.device, non_blocking=True)


def check_pano_rows(view_store, pano_table, rows_host, Vp):
    """What the host refuses before ``pano_rows`` launches: tables that do not describe the store, rows outside it, a view
    axis narrower than a panorama.  ``rows_host``: the rows as a host array (-1 = dummy panorama)."""
    ok = pano_table.__dict__.setdefault("_stores_ok", set())        # table against store: once per pair, not per batch
    if id(view_store) not in ok:
        if pano_table.keys != view_store.keys:
            raise ValueError("the PanoTable and the ViewFeatureStore must list the same viewpoints in the same order")
        if int(pano_table.view_order.max(initial=0)) >= view_store.n_views:
            raise ValueError("the PanoTable names a view the store does not have")
        ok.add(id(view_store))
    rows_host = np.asarray(rows_host)
    if rows_host.size and (rows_host.min() < -1 or rows_host.max() >= len(view_store)):
        raise IndexError(f"panorama rows must be -1 or in [0, {len(view_store)}): got {int(rows_host.min())} .. "
                         f"{int(rows_host.max())}")
    real = rows_host[rows_host >= 0]
    need = int(pano_table.n_tokens[real].max()) if real.size else 1
    if Vp < need:
        raise ValueError(f"view axis Vp = {Vp} is narrower than a panorama of {need} tokens")


def pano_rows(view_store, pano_table, rows_host, rows_dev, img, loc, nav, lens):
    """bevbert_pd_pano_rows on torch's current stream: fill img (Tp, Vp, D) f32, loc (Tp, Vp, L) f32, nav (Tp, Vp) i64 and
    lens (Tp) i64 in place from the store and the device-resident PanoTable.  ``rows_dev`` (Tp,) int32 on the device holds
    what ``rows_host`` holds; the host copy is only checked."""
    from . import lib
    Tp, Vp, D = img.shape
    L = loc.shape[2]
    check_pano_rows(view_store, pano_table, rows_host, Vp)
    order, n_tok, loc_tab, nav_tab = pano_table.to(view_store.device)
    if D > view_store.Ds or L != loc_tab.shape[2] or len(rows_host) != Tp:
        raise ValueError(f"pano_rows: D = {D} of a store with {view_store.Ds} channels, L = {L} of a table with "
                         f"{loc_tab.shape[2]}, {len(rows_host)} rows for {Tp} panoramas")
    for t, dt, shape in ((img, torch.float32, (Tp, Vp, D)), (loc, torch.float32, (Tp, Vp, L)), (nav, torch.int64, (Tp, Vp)),
                         (lens, torch.int64, (Tp,)), (rows_dev, torch.int32, (Tp,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != view_store.device:
            raise ValueError(f"pano_rows: expected a contiguous {dt} tensor of shape {shape} on {view_store.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    # the stream is torch's current one of the calling thread, read directly: a launch-stream override another thread has
    # set for its own launches (ops.WgradStream) must not capture the loader's gather
    stream = torch.cuda.current_stream(view_store.device).cuda_stream
    lib.call("bevbert_pd_pano_rows", lib.ptr(view_store.fts), view_store.Ds, view_store.n_views, lib.ptr(order),
             lib.ptr(n_tok), lib.ptr(loc_tab), lib.ptr(nav_tab), lib.ptr(rows_dev), lib.ptr(img), lib.ptr(loc), lib.ptr(nav),
             lib.ptr(lens), len(view_store), order.shape[1], L, Tp, Vp, D, stream)
